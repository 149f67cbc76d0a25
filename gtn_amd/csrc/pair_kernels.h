// pair_kernels.h -- what the kernels that run one workgroup per (utterance, hypothesis) pair share (ctc_score.hip,
// ctc_token_align.hip, asg_score.hip, asg_token_align.hip; ctc_beam.hip takes the log-add, ctc_lattice.hip that and
// the barrier): the -inf, the log-add, the
// workgroup barrier of a width known at compile time, and the dispatch from ctc_score_config to a <width, states per
// lane> instantiation.
// For .hip files only; everything here is inlined, so a file's code object holds nothing it does not call.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace gtnx {

constexpr float NEG_INF = -__builtin_inff();

__device__ __forceinline__ float logadd(float x, float y) {
  if (x == NEG_INF) return y;
  if (y == NEG_INF) return x;
  const float m = fmaxf(x, y), n = fminf(x, y);
  return m + log1pf(expf(n - m));
}

// the workgroup's barrier; a workgroup of one wave needs its LDS and global accesses ordered, nothing more
template <int WG>
__device__ __forceinline__ void wg_sync() {
  if (WG > 64) {
    __syncthreads();
  } else {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
  }
}
// ... that also tells every lane whether any lane holds a non-zero `v`
template <int WG>
__device__ __forceinline__ bool wg_any(int v) {
  if (WG > 64) return __syncthreads_or(v) != 0;
  const bool r = __ballot(v != 0) != 0;
  wg_sync<WG>();
  return r;
}

// fn<WG, PER>(...) with the width and the states per lane ctc_score_config gives for max_length U: every kernel of
// ctc_score.hip's hypothesis form has these seven instantiations and no other
#define GTNX_CTC_SCORE_DISPATCH(U, fn, ...)                  \
  do {                                                       \
    int wg, per;                                             \
    ctc_score_config(U, &wg, &per);                          \
    if (wg == 64) fn<64, 1>(__VA_ARGS__);                    \
    else if (wg == 256 && per == 1) fn<256, 1>(__VA_ARGS__); \
    else if (wg == 256) fn<256, 3>(__VA_ARGS__);             \
    else if (per == 1) fn<1024, 1>(__VA_ARGS__);             \
    else if (per == 2) fn<1024, 2>(__VA_ARGS__);             \
    else if (per == 4) fn<1024, 4>(__VA_ARGS__);             \
    else fn<1024, 9>(__VA_ARGS__);                           \
  } while (0)

}  // namespace gtnx
