// mwrt_obs.hip.h -- the instrument operator (csrc/mwrt_obs.hip): argument record and launcher only, as the
// host unit reads them.  No kernel lives here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mwrt {
namespace obs {

constexpr int THREADS = 256;               // four waves per workgroup
constexpr int WAVE = 64;                   // a wave's lanes are 64 consecutive levels of one output row
constexpr int ITEMS = THREADS / WAVE;      // (profile, block, output row, level chunk) items per workgroup
constexpr int UNROLL = 8;                  // row loads in flight per lane

// out_b[p][o][l] = sum over e in [row_ptr[o], row_ptr[o + 1]) of w[e] * in_b[p][col[e]][l], b < nblk, in the stored order
struct ObsArgs {
  const int32_t* row_ptr;                   // [m_out + 1]
  const int32_t* col;                       // [nnz], each in 0 .. m_in - 1 (checked when the operator was created)
  const double* w;                          // [nnz]
  const double* in0; const double* in1; const double* in2; const double* in3;   // [nprof][m_in][nlev]
  double* out0; double* out1; double* out2; double* out3;                       // [nprof][m_out][nlev]
  int32_t m_in, m_out, nlev, nblk;
  int32_t nchunks;                          // ceil(nlev / WAVE)
  int64_t items;                            // nprof * nblk * m_out * nchunks
};

// hipGetLastError() of the launch; hipErrorInvalidValue when the grid would exceed 2^31 - 1 workgroups
hipError_t launch_obs_apply(const ObsArgs& a, hipStream_t st);

}  // namespace obs
}  // namespace mwrt
