// far_set_dump -- how many far lines of each species the fused kernel takes through its quad loop, per frequency chunk, as
// the library's own planning decides (csrc/mwrt_plan.cpp chunk_masks, linked as is).  Built and run by
// tests/test_far_line_groups.py; needs no GPU.
//
//   far_set_dump DESC_PATH CHUNK_WIDTH F...   ->   one line per chunk: "<o2 far, not very far> <h2o far, not very far>"
//
// The counts come from the set definitions the kernels themselves use (o2_quad_set / h2o_quad_set, csrc/mwrt_plan.h): far
// lines that are not very far (and, for water, neither resonant-only, speed-dependent within reach, nor beyond the cutoff).
// The kernel takes floor(count / 4) quads of them; a wave vote at run time may zero a line's numerator but never changes the
// count.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../mwr_fast_forward_operators_and_lbls_amd/csrc/mwrt_plan.h"

using namespace mwrt;

int main(int argc, char** argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: far_set_dump DESC_PATH CHUNK_WIDTH F...\n"); return 2; }
  static mwrt_model_desc tables;
  FILE* fp = std::fopen(argv[1], "rb");
  const size_t got = fp ? std::fread(&tables, 1, sizeof(tables), fp) : 0;
  if (fp) std::fclose(fp);
  if (got != sizeof(tables)) { std::fprintf(stderr, "far_set_dump: %s is not one mwrt_model_desc\n", argv[1]); return 2; }
  const int nfc = std::atoi(argv[2]);
  std::vector<double> f;
  for (int i = 3; i < argc; ++i) f.push_back(std::atof(argv[i]));
  std::vector<LineMasks> masks;
  chunk_masks(tables, f.data(), (int)f.size(), nfc, &masks);
  for (const LineMasks& lm : masks) {
    const unsigned long long o2_q = o2_quad_set(lm, o2_far_set(lm, o2_lines_all(tables.n_o2)), false);
    const unsigned h2o_q = h2o_quad_set(lm, h2o_far_set(lm, h2o_lines_all(tables.n_h2o)), false);
    std::printf("%d %d\n", __builtin_popcountll(o2_q), __builtin_popcount(h2o_q));
  }
  return 0;
}
