"""MI355X-native line-by-line microwave forward operator (HATPRO TBs from radiosonde profiles).

Drop-in for the reference's pyrtlib hot path only
(python_src/proc/PyRTlib_processing.py:83-197): see DESIGN.md.
"""
__version__ = "0.1.0"

#: observation selection by information content (selection.py); resolved on first use, so that importing
#: the package does not import torch
_SELECTION = ("Selection", "select_observations", "rank_observations")
__all__ = list(_SELECTION)


def __getattr__(name):
    if name in _SELECTION:
        from . import selection
        return getattr(selection, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
