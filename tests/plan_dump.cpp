// plan_dump -- what the library's launch planning (csrc/mwrt_plan.cpp, linked as is) answers, as JSON: one object per
// request line on stdin.  Built and run by tests/test_kernel_instantiations.py under ASan + UBSan; needs no GPU.
//
//   constants
//   fused NLEV NF NANG CHUNK_WIDTH LDS_MAX THREADS   pick_nfc, pick_nfc_fused, LDS bytes of the split (and at one segment per pass)
//   tau NLEV                                          tau_threads, lanes_for
//   winlds THREADS                                    absorb_win_lds_bytes
//   split NANG                                        elevations per k_rte_tau launch
//   eligible F...                                     windows_eligible
//   tables PATH                                       load a raw mwrt_model_desc for the requests that follow
//   blobs F...                                        chunk_masks at widths 8 / 14 / 16, build_windows + pack_windows
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "../mwr_fast_forward_operators_and_lbls_amd/csrc/mwrt_plan.h"

using namespace mwrt;

static std::vector<double> rest(std::istringstream& in) {
  std::vector<double> v;
  for (double x; in >> x;) v.push_back(x);
  return v;
}

int main() {
  static mwrt_model_desc tables;                   // zeroed until a `tables` request
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    if (cmd == "constants") {
      std::printf("{\"WAVE\": %d, \"NFK\": %d, \"TAU_NFC\": %d, \"WIN_CHUNKS\": %d, \"WIN_CHUNKS_MAX\": %d, \"WIN_NFC\": %d, "
                  "\"WIN_NODES\": %d, \"WIN_NODES_H\": %d, \"WIN_MAX_SPAN_GHZ\": %.17g, \"RTE_THREADS\": %d, \"MAX_MULTI\": %d, "
                  "\"MAX_LEVELS\": %d, \"MAX_ANGLES\": %d, \"ERR_UNSUPPORTED\": %d, \"sizeof_desc\": %zu}\n",
                  WAVE, NFK, TAU_NFC, WIN_CHUNKS, WIN_CHUNKS_MAX, WIN_NFC, WIN_NODES, WIN_NODES_H, WIN_MAX_SPAN_GHZ, RTE_THREADS,
                  MAX_MULTI, MWRT_MAX_LEVELS, MWRT_MAX_ANGLES, (int)MWRT_ERR_UNSUPPORTED, sizeof(mwrt_model_desc));
    } else if (cmd == "fused") {
      int nlev, nf, nang, width, lds_max, threads;
      in >> nlev >> nf >> nang >> width >> lds_max >> threads;
      const int nfc = pick_nfc_fused(width, lds_max, nlev, nf, nang);
      LaunchGeom g, gmin;
      size_t lds = 0, lds_min = 0;
      const bool fits = plan_fused(lds_max, nfc, nlev, nf, nang, &g, &lds, threads);
      (void)plan_fused(0, width ? width : pick_nfc(nf), nlev, nf, nang, &gmin, &lds_min, threads);   // shrunk to one segment per pass
      std::printf("{\"pick_nfc\": %d, \"nfc\": %d, \"fits\": %s, \"lds\": %zu, \"lds_min_wide\": %zu, \"nseg\": [%d, %d], "
                  "\"seglen\": [%d, %d], \"npart\": %d, \"ldrow\": %d}\n",
                  pick_nfc(nf), nfc, fits ? "true" : "false", lds, lds_min, g.nseg[0], g.nseg[1], g.seglen[0], g.seglen[1],
                  g.npart, g.ldrow);
    } else if (cmd == "tau") {
      int nlev; in >> nlev;
      std::printf("{\"tau_threads\": %d, \"lanes_for\": %d}\n", tau_threads(nlev), lanes_for(nlev));
    } else if (cmd == "winlds") {
      int threads; in >> threads;
      std::printf("{\"absorb_win_lds_bytes\": %zu}\n", absorb_win_lds_bytes(threads));
    } else if (cmd == "split") {
      int nang; in >> nang;
      std::printf("{\"split\": [");
      for (int rem = nang; rem > 0; rem -= rte_tau_angles(rem)) std::printf("%s%d", rem == nang ? "" : ", ", rte_tau_angles(rem));
      std::printf("]}\n");
    } else if (cmd == "eligible") {
      const std::vector<double> f = rest(in);
      std::printf("{\"eligible\": %s}\n", windows_eligible(f.data(), (int)f.size()) ? "true" : "false");
    } else if (cmd == "tables") {
      std::string path; in >> path;
      FILE* fp = std::fopen(path.c_str(), "rb");
      const size_t got = fp ? std::fread(&tables, 1, sizeof(tables), fp) : 0;
      const bool whole = fp && got == sizeof(tables) && std::fgetc(fp) == EOF;
      if (fp) std::fclose(fp);
      if (!whole) { std::fprintf(stderr, "plan_dump: %s is not one mwrt_model_desc\n", path.c_str()); return 2; }
      std::printf("{\"n_o2\": %d, \"n_h2o\": %d}\n", tables.n_o2, tables.n_h2o);
    } else if (cmd == "blobs") {
      const std::vector<double> f = rest(in);
      const int nf = (int)f.size();
      std::printf("{\"nchunks\": [");
      for (int nfc : {8, 14, 16}) {
        std::vector<LineMasks> masks;
        chunk_masks(tables, f.data(), nf, nfc, &masks);
        std::printf("%zu%s", masks.size(), nfc == 16 ? "]" : ", ");
      }
      WindowSet ws;
      build_windows(tables, f.data(), nf, &ws);
      std::vector<char> blob;
      pack_windows(ws, nf, &blob);
      const WindowLayout l = window_layout((int)ws.wins.size(), nf);
      int chunks = 0;
      for (const WinDesc& w : ws.wins) chunks += w.nchunks;
      WinDesc first;
      std::memcpy(&first, blob.data(), sizeof(first));
      std::printf(", \"nwin\": %zu, \"window_chunks\": %d, \"blob_bytes\": %zu, \"layout\": [%zu, %zu, %zu, %zu], \"flo\": %.17g}\n",
                  ws.wins.size(), chunks, blob.size(), l.off_lag, l.off_lagh, l.off_lagsd, l.total, first.flo);
    } else {
      std::fprintf(stderr, "plan_dump: unknown request '%s'\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
