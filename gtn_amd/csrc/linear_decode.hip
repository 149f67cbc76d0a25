// linear_decode.hip -- viterbiPath(emissions_b) of a whole padded [n][M][C] batch plus the CTC collapse, results left
// on the device (the decode a CTC model runs at inference: best path, merge repeats, drop blanks).
//
// shortestPath (shortest.cpp:190-272) on linearGraph(T, C) has a closed form: frame t takes the FIRST arc whose weight
// is strictly greater than everything before it, starting from -inf (the smallest label among equal maxima; NaN and
// -inf are never taken), the score is ((0 + m_0) + m_1) + ... + m_{T-1} in float32 in frame order, a frame without an
// entry above -inf means there is no path (empty graph, score -inf), and so do zero frames: linearGraph(0, C) is one
// start node that does not accept (creations.cpp:22).
//
// Two launches.
//   rows:      a pure stream.  A group of LPR lanes (8 / 16 / 32 / 64, by C) owns one row: scalar head up to the next
//              16-byte boundary, 16-byte loads, scalar tail (C = 29: neither a row's start nor its length is a multiple
//              of 4); per lane (max, argmax) by `v > m` from (-inf, -1) in rising index order; across lanes the larger
//              value, of equal values the smaller index.  The grid is (blocks of frames, utterance), so 8 utterances
//              still fill the machine.  The label goes straight into the caller's row, the maximum into scratch.
//              Rows from frames[b] on are never addressed.
//   collapse:  one wave per utterance.  Pass 1 adds the stored maxima in frame order (lane by lane through readlane:
//              the association is the contract, so no tree) and looks for a label of -1 (no path).  Pass 2 takes 64
//              frames at a time: keep = label != predecessor && label != blank, the predecessor of lane 0 carried from
//              lane 63 of the block before; a ballot and a prefix count give the position.  Then the -1 entries.
// Every store is a plain C++ store; there is no inline assembly.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace gtnx {
namespace {

constexpr float NEG_INF = -__builtin_inff();
constexpr int kRowBlock = 256;  // threads of a row-kernel workgroup
constexpr int kRowTrips = 4;    // rows each lane group takes, one after the other

__device__ __forceinline__ void take(float v, int i, float& m, int& mi) {
  if (v > m) {
    m = v;
    mi = i;
  }
}

template <int LPR>
__global__ __launch_bounds__(kRowBlock) void linear_decode_rows_kernel(LinearDecodeArgs a) {
  constexpr int GROUPS = kRowBlock / LPR;  // rows in flight per workgroup
  const int b = blockIdx.y;
  int T = a.frames[b];
  T = T < 0 ? 0 : (T > a.M ? a.M : T);  // (the engine has refused such counts: nothing outside the slab is addressed)
  const int C = a.C;
  const int lane = threadIdx.x % LPR, group = threadIdx.x / LPR;
  const int t0 = blockIdx.x * (GROUPS * kRowTrips);
  for (int trip = 0; trip < kRowTrips; ++trip) {
    const int t = t0 + trip * GROUPS + group;
    if (t >= T) break;  // (whole lane groups leave together: the shuffles below stay inside a group)
    const GTNX_G float* p = a.em + (int64_t(b) * a.M + t) * C;
    float m = NEG_INF;
    int mi = -1;
    int head = int((4 - ((reinterpret_cast<uintptr_t>(p) >> 2) & 3)) & 3);
    if (head > C) head = C;
    if (lane < head) take(p[lane], lane, m, mi);
    const GTNX_G gtnx_f4* v = reinterpret_cast<const GTNX_G gtnx_f4*>(p + head);
    const int nv = (C - head) >> 2;
    for (int i = lane; i < nv; i += LPR) {
      const gtnx_f4 x = v[i];
      const int c = head + 4 * i;
      take(x.x, c, m, mi);
      take(x.y, c + 1, m, mi);
      take(x.z, c + 2, m, mi);
      take(x.w, c + 3, m, mi);
    }
    const int done = head + 4 * nv;
    if (lane < C - done) take(p[done + lane], done + lane, m, mi);
    // the larger value; of equal values the smaller index (mi = -1 exactly where m = -inf, on both sides)
#pragma unroll
    for (int off = LPR / 2; off >= 1; off >>= 1) {
      const float om = __shfl_xor(m, off);
      const int oi = __shfl_xor(mi, off);
      if (om > m || (om == m && oi < mi)) {
        m = om;
        mi = oi;
      }
    }
    if (lane == 0) {
      a.labels[int64_t(b) * a.row_stride + t] = mi;
      a.rowmax[int64_t(b) * a.M + t] = m;
    }
  }
}

__global__ __launch_bounds__(64) void linear_decode_collapse_kernel(LinearDecodeArgs a) {
  const int b = blockIdx.x, l = threadIdx.x;
  const int M = a.M;
  int T = a.frames[b];
  T = T < 0 ? 0 : (T > M ? M : T);
  GTNX_G int* lrow = a.labels + int64_t(b) * a.row_stride;
  GTNX_G int* crow = a.collapsed ? a.collapsed + int64_t(b) * a.row_stride : nullptr;
  GTNX_G int* srow = a.starts ? a.starts + int64_t(b) * a.row_stride : nullptr;
  const GTNX_G float* mrow = a.rowmax + int64_t(b) * M;
  // ---- pass 1: the score, in frame order, and whether every frame found a label
  float score = 0.0f;
  bool none = T == 0;  // (a chain without frames has a start node that does not accept)
  for (int base = 0; base < T; base += 64) {
    const int idx = base + l;
    const float mv = idx < T ? mrow[idx] : 0.0f;
    const int lab = idx < T ? lrow[idx] : 0;
    none |= __builtin_amdgcn_ballot_w64(lab < 0) != 0;
    const int cnt = T - base < 64 ? T - base : 64;
    for (int k = 0; k < cnt; ++k) score += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mv), k));
  }
  if (none) {  // no path: every entry of every row -1
    for (int i = l; i < M; i += 64) {
      lrow[i] = -1;
      if (crow) crow[i] = -1;
      if (srow) srow[i] = -1;
    }
    if (l == 0) {
      if (a.scores) a.scores[b] = NEG_INF;
      if (a.lengths) a.lengths[b] = 0;
    }
    return;
  }
  for (int i = T + l; i < M; i += 64) lrow[i] = -1;
  if (l == 0 && a.scores) a.scores[b] = score;
  if (!crow) return;
  // ---- pass 2: merge repeats, drop blanks (labels of a path are >= 0, so -1 stands for "no predecessor")
  int count = 0, carry = -1;
  for (int base = 0; base < T; base += 64) {
    const int idx = base + l;
    const int v = idx < T ? lrow[idx] : -1;
    const int up = __shfl_up(v, 1);
    const int before = l == 0 ? carry : up;
    const bool keep = idx < T && v != before && v != a.blank;
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
    const int pos = count + __builtin_popcountll(mask & ((1ull << l) - 1ull));
    if (keep) {  // pos <= idx < M
      crow[pos] = v;
      if (srow) srow[pos] = idx;
    }
    count += __builtin_popcountll(mask);
    carry = __builtin_amdgcn_readlane(v, 63);
  }
  for (int i = count + l; i < M; i += 64) {
    crow[i] = -1;
    if (srow) srow[i] = -1;
  }
  if (l == 0 && a.lengths) a.lengths[b] = count;
}

template <int LPR>
void launch_rows(const LinearDecodeArgs& a, hipStream_t st) {
  const int per_block = (kRowBlock / LPR) * kRowTrips;
  const unsigned gx = static_cast<unsigned>((a.M + per_block - 1) / per_block);
  // (grid.y holds at most 65535 utterances per launch)
  for (int b0 = 0; b0 < a.n; b0 += 65535) {
    LinearDecodeArgs s = a;
    const int nb = a.n - b0 < 65535 ? a.n - b0 : 65535;
    s.em += int64_t(b0) * a.M * a.C;
    s.frames += b0;
    s.labels += int64_t(b0) * a.row_stride;
    s.rowmax += int64_t(b0) * a.M;
    hipLaunchKernelGGL(linear_decode_rows_kernel<LPR>, dim3(gx, static_cast<unsigned>(nb)), dim3(kRowBlock), 0, st, s);
  }
}

}  // namespace

void launch_linear_decode(const LinearDecodeArgs& a, int which, hipStream_t st) {
  if (a.n <= 0) return;
  if (which == 0) {
    if (a.M <= 0) return;
    // lanes per row: every lane of a group gets at least one 16-byte load where the row has that many
    if (a.C <= 32) launch_rows<8>(a, st);
    else if (a.C <= 64) launch_rows<16>(a, st);
    else if (a.C <= 128) launch_rows<32>(a, st);
    else launch_rows<64>(a, st);
    return;
  }
  hipLaunchKernelGGL(linear_decode_collapse_kernel, dim3(static_cast<unsigned>(a.n)), dim3(64), 0, st, a);
}

}  // namespace gtnx
