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
//   windows F...                                      the whole window plan: every WinDesc in dispatch order with its two Lagrange
//                                                     blocks, lag_sd per chunk, the width-16 LineMasks of every chunk
#include <cmath>
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

// a double as JSON that reads back to the same bits; NaN / Infinity as Python's json module spells them
static void put(double x) {
  if (std::isnan(x)) std::printf("NaN");
  else if (std::isinf(x)) std::printf(x < 0 ? "-Infinity" : "Infinity");
  else std::printf("%.17g", x);
}

static void put_all(const double* x, size_t n) {
  std::printf("[");
  for (size_t i = 0; i < n; ++i) { if (i) std::printf(", "); put(x[i]); }
  std::printf("]");
}

static bool all_zero(const double* x, size_t n) {
  for (size_t i = 0; i < n; ++i) if (std::memcmp(&x[i], "\0\0\0\0\0\0\0\0", 8)) return false;
  return true;
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
    } else if (cmd == "windows") {
      const std::vector<double> f = rest(in);
      const int nf = (int)f.size();
      WindowSet ws;
      build_windows(tables, f.data(), nf, &ws);
      std::vector<LineMasks> masks;
      chunk_masks(tables, f.data(), nf, WIN_NFC, &masks);
      // the device image holds the same bytes, part by part
      std::vector<char> blob;
      pack_windows(ws, nf, &blob);
      const WindowLayout l = window_layout((int)ws.wins.size(), nf);
      const bool packed = !std::memcmp(blob.data(), ws.wins.data(), sizeof(WinDesc) * ws.wins.size()) &&
                          !std::memcmp(blob.data() + l.off_lag, ws.lag.data(), sizeof(double) * ws.lag.size()) &&
                          !std::memcmp(blob.data() + l.off_lagh, ws.lag_h.data(), sizeof(double) * ws.lag_h.size()) &&
                          !std::memcmp(blob.data() + l.off_lagsd, ws.lag_sd.data(), sizeof(double) * ws.lag_sd.size());
      const size_t perm = (size_t)WIN_CHUNKS_MAX * WIN_NFC;
      std::printf("{\"nf\": %d, \"packed\": %s, \"windows\": [", nf, packed ? "true" : "false");
      for (size_t w = 0; w < ws.wins.size(); ++w) {
        const WinDesc& d = ws.wins[w];
        const size_t used = (size_t)d.nchunks * WIN_NFC;
        const double* lag = ws.lag.data() + w * perm * WIN_NODES;
        const double* lagh = ws.lag_h.data() + w * perm * WIN_NODES_H;
        std::printf("%s{\"first_chunk\": %d, \"nchunks\": %d, \"flo\": ", w ? ", " : "", d.first_chunk, d.nchunks);
        put(d.flo); std::printf(", \"fhi\": "); put(d.fhi);
        std::printf(", \"fnode\": "); put_all(d.fnode, WIN_NODES);
        std::printf(", \"fnode_h\": "); put_all(d.fnode_h, WIN_NODES_H);
        std::printf(", \"o2_far\": %llu, \"h2o_far_both\": %u, \"h2o_far_res\": %u", d.o2_far, d.h2o_far_both, d.h2o_far_res);
        std::printf(", \"lag\": "); put_all(lag, used * WIN_NODES);             // [chunk][node][target]
        std::printf(", \"lag_h\": "); put_all(lagh, used * WIN_NODES_H);
        // what lies behind the window's own chunks in its WIN_CHUNKS_MAX-chunk block
        std::printf(", \"lag_rest_zero\": %s}", all_zero(lag + used * WIN_NODES, (perm - used) * WIN_NODES) &&
                                                  all_zero(lagh + used * WIN_NODES_H, (perm - used) * WIN_NODES_H) ? "true" : "false");
      }
      std::printf("], \"lag_sd\": [");                                          // [chunk][target][node]
      for (size_t ch = 0; ch < masks.size(); ++ch) {
        std::printf("%s", ch ? ", " : "");
        put_all(ws.lag_sd.data() + ch * SD_TARGETS * SD_NODES, (size_t)SD_TARGETS * SD_NODES);
      }
      std::printf("], \"masks\": [");
      for (size_t ch = 0; ch < masks.size(); ++ch) {
        const LineMasks& m = masks[ch];
        std::printf("%s{\"o2_far\": %llu, \"o2_vfar\": %llu, \"h2o_far\": %u, \"h2o_vfar\": %u, \"h2o_none\": %u, \"h2o_res\": %u, "
                    "\"h2o_sd\": %u, \"h2o_sdfar\": %u, \"h2o_sdint\": %u, \"vf_u0\": ", ch ? ", " : "", m.o2_far, m.o2_vfar, m.h2o_far,
                    m.h2o_vfar, m.h2o_none, m.h2o_res, m.h2o_sd, m.h2o_sdfar, m.h2o_sdint);
        put(m.vf_u0); std::printf(", \"vf_h\": "); put(m.vf_h); std::printf("}");
      }
      std::printf("]}\n");
    } else {
      std::fprintf(stderr, "plan_dump: unknown request '%s'\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
