// padfill.hip -- zeros for the pad rows of a ragged [n][M][C] gradient.
//
// A LINEAR batch whose element b has rows[b] <= M rows (batch.h: Batch::rows) keeps the slab stride M*C, and the
// backward sweeps write rows [0, rows[b]) only.  What the caller receives must be 0 in rows [rows[b], M): this kernel
// stores those zeros and nothing else -- 4*C*sum(M - rows[b]) bytes in ONE launch for the whole batch, instead of a
// memset of the whole tensor in front of a sweep that overwrites most of it (at B=512, T=1000, C=256: 524 MB on a
// path that HBM bounds).
//
// The pad floats of all elements form one index space [0, prefix[n]); workgroup g owns the slice
// [g * kPadChunk, (g + 1) * kPadChunk) of it, wherever that falls: a long pad is shared by many workgroups, many short
// pads by one.  The slice is cut at element boundaries; every piece gets a scalar head up to the next 16-byte
// boundary, 16-byte stores, and a scalar tail (C = 9: neither the pad's start nor its length is a multiple of 4).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace gtnx {
namespace {

constexpr int kPadBlock = 256;
constexpr int64_t kPadChunk = 8192;  // floats per workgroup: 8 16-byte stores per thread

__global__ __launch_bounds__(kPadBlock) void pad_fill_kernel(PadFillArgs a) {
  const int64_t total = a.prefix[a.n];
  const int64_t g0 = int64_t(blockIdx.x) * kPadChunk;
  if (g0 >= total) return;
  const int64_t g1 = g0 + kPadChunk < total ? g0 + kPadChunk : total;
  // the last element whose pad starts at or before g0 (prefix[0] = 0 <= g0 < total = prefix[n]); elements without a
  // pad share their prefix with the next one and are passed over
  int lo = 0, hi = a.n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.prefix[mid] <= g0)
      lo = mid;
    else
      hi = mid;
  }
  const int tid = threadIdx.x;
  for (int b = lo; b < a.n; ++b) {
    const int64_t p0 = a.prefix[b], p1 = a.prefix[b + 1];
    if (p0 >= g1) break;
    const int64_t s = (g0 > p0 ? g0 : p0) - p0, e = (g1 < p1 ? g1 : p1) - p0;
    if (e <= s) continue;
    GTNX_G float* p = a.base + (a.offs ? a.offs[b] : int64_t(b) * a.stride) + int64_t(a.rows[b]) * a.C + s;
    const int64_t cnt = e - s;
    int64_t head = int64_t((4 - ((reinterpret_cast<uintptr_t>(p) >> 2) & 3)) & 3);
    if (head > cnt) head = cnt;
    if (tid < head) p[tid] = 0.0f;
    GTNX_G float4* v = reinterpret_cast<GTNX_G float4*>(p + head);
    const int64_t nv = (cnt - head) >> 2;
    for (int64_t i = tid; i < nv; i += kPadBlock) v[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const int64_t done = head + 4 * nv;
    if (tid < cnt - done) p[done + tid] = 0.0f;
  }
}

}  // namespace

void launch_pad_fill(const PadFillArgs& a, int64_t total_floats, hipStream_t st) {
  if (a.n <= 0 || total_floats <= 0) return;
  const int64_t grid = (total_floats + kPadChunk - 1) / kPadChunk;
  hipLaunchKernelGGL(pad_fill_kernel, dim3(static_cast<unsigned>(grid)), dim3(kPadBlock), 0, st, a);
}

}  // namespace gtnx
