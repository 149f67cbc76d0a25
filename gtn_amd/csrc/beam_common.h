// beam_common.h -- what the two prefix beam searches share (ctc_beam.hip, asg_beam.hip): the top-K row stream, i.e.
// the body of their rows kernels, templated on the lanes per row and on whether a blank is appended to the set, and the
// small pieces of their search kernels that do not depend on a prefix's state (the score bits of a sort key, the prefix
// hash, the identity of two trie chains).  For .hip files only; everything here is inlined, so a file's code object
// holds nothing it does not call.
//
// A group of LPR lanes owns one row: scalar head up to the next 16-byte boundary, 16-byte loads, scalar tail; grid =
// (blocks of frames, utterance); rows from frames[b] on are never addressed.  Round r takes the first entry, in the
// order (value descending, label ascending), that comes after the entry of round r - 1: per lane `v > m` in rising
// label order among the entries still allowed, across lanes the larger value and of equal values the smaller label.
// NaN fails every comparison and -inf never exceeds the start value, so neither is chosen; a round that finds nothing
// ends the row.  The row is read again in every round (from the vector L1 after the first), which keeps any number of
// labels in one code path.  With BLANK, `a.blank` is then appended if no round took it and its entry is above -inf.
// Lane 0 of the group stores one 8-byte (value, label) entry per round and the count; a row's entries are
// topn + (BLANK ? 1 : 0) apart.
// Args: em, frames, ent_val, ent_cnt, M, C, topn (and blank with BLANK) as in CtcBeamArgs.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "pair_kernels.h"

namespace gtnx {

constexpr int kRowBlock = 256;  // threads of a row-kernel workgroup
constexpr int kRowTrips = 4;    // rows each lane group takes, one after the other

typedef int gtnx_i2 __attribute__((ext_vector_type(2)));  // 8 bytes: a member of a token set (value bits, label), a
                                                           // trie node (parent node, label)
__device__ __forceinline__ gtnx_i2 entry(float v, int c) {
  gtnx_i2 e;
  e.x = __float_as_int(v);
  e.y = c;
  return e;
}

// (value descending, label ascending): does (v, c) come after (pv, pc)?  False for NaN.
__device__ __forceinline__ bool after(float v, int c, float pv, int pc) { return v < pv || (v == pv && c > pc); }

__device__ __forceinline__ void take(float v, int c, float pv, int pc, float& m, int& mi) {
  if (after(v, c, pv, pc) && v > m) {
    m = v;
    mi = c;
  }
}

template <int LPR, bool BLANK, class Args>
__device__ __forceinline__ void beam_rows_body(const Args& a) {
  constexpr int GROUPS = kRowBlock / LPR;  // rows in flight per workgroup
  const int b = blockIdx.y;
  int T = a.frames[b];
  T = T < 0 ? 0 : (T > a.M ? a.M : T);  // (the engine has refused such counts: nothing outside the slab is addressed)
  const int C = a.C, K = a.topn;
  const int stride = BLANK ? K + 1 : K;
  [[maybe_unused]] int blank = -1;
  if constexpr (BLANK) blank = a.blank;
  const int lane = threadIdx.x % LPR, group = threadIdx.x / LPR;
  const int t0 = blockIdx.x * (GROUPS * kRowTrips);
  for (int trip = 0; trip < kRowTrips; ++trip) {
    const int t = t0 + trip * GROUPS + group;
    if (t >= T) break;  // (whole lane groups leave together: the shuffles below stay inside a group)
    const int64_t row = int64_t(b) * a.M + t;
    const GTNX_G float* p = a.em + row * C;
    GTNX_G gtnx_i2* out = reinterpret_cast<GTNX_G gtnx_i2*>(a.ent_val) + row * stride;
    int head = int((4 - ((reinterpret_cast<uintptr_t>(p) >> 2) & 3)) & 3);
    if (head > C) head = C;
    const GTNX_G gtnx_f4* v = reinterpret_cast<const GTNX_G gtnx_f4*>(p + head);
    const int nv = (C - head) >> 2;
    const int done = head + 4 * nv;
    float pv = __builtin_inff();  // the entry of the round before: everything below +inf comes after it
    int pc = -1;
    int count = 0;
    [[maybe_unused]] bool has_blank = false;
    for (int r = 0; r < K; ++r) {
      float m = NEG_INF;
      int mi = -1;
      if (lane < head) take(p[lane], lane, pv, pc, m, mi);
      for (int i = lane; i < nv; i += LPR) {
        const gtnx_f4 x = v[i];
        const int c = head + 4 * i;
        take(x.x, c, pv, pc, m, mi);
        take(x.y, c + 1, pv, pc, m, mi);
        take(x.z, c + 2, pv, pc, m, mi);
        take(x.w, c + 3, pv, pc, m, mi);
      }
      if (lane < C - done) take(p[done + lane], done + lane, pv, pc, m, mi);
      // the larger value; of equal values the smaller label (mi = -1 exactly where m = -inf, on both sides)
#pragma unroll
      for (int off = LPR / 2; off >= 1; off >>= 1) {
        const float om = __shfl_xor(m, off);
        const int oi = __shfl_xor(mi, off);
        if (om > m || (om == m && oi < mi)) {
          m = om;
          mi = oi;
        }
      }
      if (mi < 0) break;  // (the same in every lane of the group)
      if (lane == 0) out[r] = entry(m, mi);
      if constexpr (BLANK) has_blank |= mi == blank;
      pv = m;
      pc = mi;
      ++count;
    }
    if (lane == 0) {
      if constexpr (BLANK) {
        if (!has_blank) {
          const float xb = p[blank];
          if (xb > NEG_INF) out[count++] = entry(xb, blank);  // (false for NaN)
        }
      }
      a.ent_cnt[row] = count;
    }
  }
}

// ---- pieces of the search kernels ----
// a float as 32 bits that rise as the float falls (-0 counts as +0), and back
__device__ __forceinline__ uint32_t falling_bits(float f) {
  const uint32_t u = __float_as_uint(f + 0.0f);
  return ~(u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u));
}
__device__ __forceinline__ float from_falling_bits(uint32_t h) {
  const uint32_t m = ~h;
  return __uint_as_float((m & 0x80000000u) ? m ^ 0x80000000u : ~m);
}

// the hash of prefix + c from the hash of the prefix.  It only spares comparisons: identity is decided by the labels.
__device__ __forceinline__ unsigned long long grow_hash(unsigned long long h, int c) {
  h = (h ^ (static_cast<unsigned long long>(uint32_t(c)) + 0x9e3779b97f4a7c15ull)) * 0xff51afd7ed558ccdull;
  return h ^ (h >> 32);
}

// Do trie nodes x and y spell the same labels?  Both stand for prefixes of the same length.  Equal numbers are the
// same node; otherwise the chains are compared label by label towards the root until they meet.
__device__ __forceinline__ bool same_prefix(const GTNX_G gtnx_i2* trie, int x, int y) {
  while (x != y) {
    if (x <= 0 || y <= 0) return false;
    const gtnx_i2 ex = trie[x], ey = trie[y];
    if (ex.y != ey.y) return false;
    x = ex.x;
    y = ey.x;
  }
  return true;
}

// finite: neither an infinity nor NaN
__device__ __forceinline__ bool finite_bits(float f) { return (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u; }

// the launches of a rows kernel: grid.y holds at most 65535 utterances per launch
template <class Args, class Launch>
void for_row_slices(const Args& a, int lpr, int stride, Launch&& launch) {
  const int per_block = (kRowBlock / lpr) * kRowTrips;
  const unsigned gx = static_cast<unsigned>((a.M + per_block - 1) / per_block);
  for (int b0 = 0; b0 < a.n; b0 += 65535) {
    Args s = a;
    const int nb = a.n - b0 < 65535 ? a.n - b0 : 65535;
    s.em += int64_t(b0) * a.M * a.C;
    s.frames += b0;
    s.ent_val += int64_t(b0) * a.M * stride * 2;
    s.ent_cnt += int64_t(b0) * a.M;
    launch(s, dim3(gx, static_cast<unsigned>(nb)));
  }
}

}  // namespace gtnx
