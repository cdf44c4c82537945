// mwrt_inst.hip -- one translation unit per frequency-chunk width (compile with -DMWRT_INST_NFC=8|14|16):
// the fused-kernel and absorption-kernel instantiations of that width and their launchers (declared in mwrt_args.hip.h).
#include "mwrt_fused.hip.h"
#include "mwrt_tau.hip.h"

#include <type_traits>

#ifndef MWRT_INST_NFC
#error "compile with -DMWRT_INST_NFC=8, 14 or 16"
#endif

namespace mwrt {

namespace {

constexpr int NFC = MWRT_INST_NFC;

template <class K, class Args>
hipError_t launch_with_lds(K k, const Args& a, dim3 grid, dim3 block, size_t lds, hipStream_t st) {
  hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k, grid, block, lds, st, a);
  return hipGetLastError();
}

// workgroup size class: 256 threads up to 256 levels; 512 threads get 256 VGPRs per lane (no scratch);
// only > 512 levels fall to the 1024-thread instantiation, whose 128-VGPR cap spills
// (profiles/r02_tall_profiles.txt).  `launch` is called with the class as a std::integral_constant; a kernel
// that has no 1024-thread instantiation passes TOP = 512.
template <int TOP = 1024, class F>
hipError_t by_size_class(unsigned threads, F launch) {
  if (threads <= 256) return launch(std::integral_constant<int, 256>{});
  if constexpr (TOP == 512) return launch(std::integral_constant<int, 512>{});
  else {
    if (threads <= 512) return launch(std::integral_constant<int, 512>{});
    return launch(std::integral_constant<int, 1024>{});
  }
}

template <bool OPT, bool EXTRAS, bool ALPHA = false>
hipError_t launch_by_size(const FusedArgs& a, dim3 grid, dim3 block, size_t lds, hipStream_t st) {
  return by_size_class(block.x, [&](auto maxt) {
    return launch_with_lds(k_tb_fused<NFC, NFK, decltype(maxt)::value, OPT, EXTRAS, ALPHA>, a, grid, block, lds, st);
  });
}

template <bool TAU>
hipError_t launch_absorb(const AbsorbArgs& a, dim3 grid, dim3 block, hipStream_t st) {
  return by_size_class(block.x, [&](auto maxt) {
    hipLaunchKernelGGL((k_absorb<NFC, decltype(maxt)::value, TAU>), grid, block, 0, st, a);
    return hipGetLastError();
  });
}

}  // namespace

#define MWRT_CAT2(a, b) a##b
#define MWRT_CAT(a, b) MWRT_CAT2(a, b)

hipError_t MWRT_CAT(launch_fused_nfc, MWRT_INST_NFC)(const FusedArgs& a, dim3 grid, dim3 block, size_t lds, hipStream_t st,
                                                      int variant) {
  switch (variant) {
    case FUSED_TB_ONLY: return launch_by_size<false, false>(a, grid, block, lds, st);
    case FUSED_OPT: return launch_by_size<true, false>(a, grid, block, lds, st);
    case FUSED_FROM_ALPHA: return launch_by_size<false, false, true>(a, grid, block, lds, st);
    default: return launch_by_size<true, true>(a, grid, block, lds, st);
  }
}

hipError_t MWRT_CAT(launch_absorb_nfc, MWRT_INST_NFC)(const AbsorbArgs& a, dim3 grid, dim3 block, hipStream_t st) {
  return launch_absorb<false>(a, grid, block, st);
}

#if MWRT_INST_NFC == 16
hipError_t launch_absorb_win(const AbsorbWinArgs& a, dim3 grid, dim3 block, hipStream_t st, bool tau) {
  // node sums in LDS: 16 (O2) + 8 (H2O) doubles per thread -- 36 KB at 192 threads: four workgroups per CU
  const size_t lds = sizeof(double) * (WIN_NODES + WIN_NODES_H) * block.x;
  return by_size_class<512>(block.x, [&](auto maxt) {
    constexpr int MAXT = decltype(maxt)::value;
    return tau ? launch_with_lds(k_absorb_win<MAXT, true>, a, grid, block, lds, st)
               : launch_with_lds(k_absorb_win<MAXT, false>, a, grid, block, lds, st);
  });
}

// K1 + layer step, every line at every frequency: zenith layer optical depth [nprof][nlev][fpitch]
hipError_t launch_absorb_tau(const AbsorbArgs& a, dim3 grid, dim3 block, hipStream_t st) {
  return launch_absorb<true>(a, grid, block, st);
}

namespace {
template <int NA>
hipError_t launch_rte_one(const RteTauArgs& a, dim3 grid, size_t lds, hipStream_t st) {
  hipLaunchKernelGGL((k_rte_tau<NA>), grid, dim3(RTE_THREADS), lds, st, a);
  return hipGetLastError();
}
}  // namespace

// RTE from layer optical depths; `na` elevations (a.a0 .. a.a0 + na - 1) per launch, na in 1..8 or 10
hipError_t launch_rte_tau(const RteTauArgs& a, dim3 grid, size_t lds, hipStream_t st, int na) {
  switch (na) {
    case 1: return launch_rte_one<1>(a, grid, lds, st);
    case 2: return launch_rte_one<2>(a, grid, lds, st);
    case 3: return launch_rte_one<3>(a, grid, lds, st);
    case 4: return launch_rte_one<4>(a, grid, lds, st);
    case 5: return launch_rte_one<5>(a, grid, lds, st);
    case 6: return launch_rte_one<6>(a, grid, lds, st);
    case 7: return launch_rte_one<7>(a, grid, lds, st);
    case 8: return launch_rte_one<8>(a, grid, lds, st);
    case 10: return launch_rte_one<10>(a, grid, lds, st);
    default: return hipErrorInvalidValue;
  }
}
#endif

}  // namespace mwrt
