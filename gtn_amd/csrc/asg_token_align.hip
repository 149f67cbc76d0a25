// asg_token_align.hip -- the best ASG alignment of device-resident hypotheses under shared emission slabs: per token its
// first frame, one past its last frame and its summed emissions, per hypothesis the Viterbi score, per frame (optional)
// the token index (DESIGN section 28 holds the contract; tests/asg_token_align_fp.py is the same arithmetic in numpy).
//
// Pair p = b * N + k is the hypothesis y = tokens[p * row_stride .. + len), len = clamp(lengths[p], 0, L), of utterance
// b with T_b frames; its states are those of asg_score.hip: position i = 0 .. len - 1 ("the first i + 1 labels are
// consumed") carries y[i], a frame enters it from itself with w_self[i] = table[C + y[i] * C + y[i]] or from i - 1 with
// w_step[i] = table[C + y[i] * C + y[i - 1]] (position 0: from the start with table[y[0]], at frame 0 only).  Equal
// neighbours are legal; there is no blank.  Paths start in position 0 at frame 0 and end in position len - 1 behind
// frame T_b - 1.
//
//   arithmetic: float32, that of asg_align.hip: c0 = alpha[i] + (w_self[i] + e), c1 = alpha[i - 1] + (w_step[i] + e), the
//             new value is the exact maximum, frame 0 is 0.0f + (w_step[0] + e).  Of two equal candidates the step wins
//             (c1 >= c0): no ranks, no second launch.  Every output is reproducible bit for bit.
//   sweep:    one workgroup per pair, width and positions per lane from asg_score_config(max_length).  A lane owns the
//             positions tid, tid + WG, ... (labels and the two gathered weights in registers); the alpha row ping-pongs
//             in LDS behind one -inf cell, one barrier per frame (a wave fence when the workgroup is one wave), the next
//             frame's emissions loaded before it.  A lane ors the one back-pointer bit of each of its positions over 32
//             frames into a word and stores bp[(t / 32) * U + i] every 32nd frame and at T_b - 1: coalesced stores.  A
//             dead position needs no code: -inf >= -inf stores a step the best path never reads.
//   walk:     wave 0, behind a workgroup barrier (the words are the other waves' stores).  In 32 frames the path descends
//             at most 32 positions and a row's step u is read before its descent, so anchored at the position the path
//             had a row earlier the offsets of a row are 0 .. 63: a word row is ONE window load of ONE register, lane i
//             holding the word of position top - i.  The 32 steps run in registers by readlane while the next row's
//             window, anchored at the position the path has now, is in flight: T / 32 dependent loads per pair.  Lane
//             t % 64 keeps the position of frame t; every 64 frames the wave stores frame_tokens and notes, where the
//             position changes between neighbouring frames, starts[i] / ends[i] in LDS (the alpha rows are free by then).
//   tokens:   behind a second barrier lane i (striding over the tokens) sums e(t, y[i]) over t = starts[i] .. ends[i] - 1
//             in ascending order, starting from the first frame's value, and stores starts, ends and token_scores.
// Entries no path covers (i >= len, t >= T_b, every entry of a pair without a path) are written -1 / -inf by the same
// workgroup: every element of every row is written over the widths L and M, nothing beyond them.  No path: len == 0,
// len > U, T_b < len, a token inside the length outside 0 .. C - 1 (checked before one becomes an address, by the lane
// that owns it and by the lane that gathers through it), or an end position at -inf.  Nothing at or past a length or a
// frame count is read.  NaN or +inf inputs give unspecified values, never an access outside the pair's rows: the walk's
// position is clamped at 0, offsets into a window are clamped, and a token whose span was not noted gets -inf without a
// read.  Every store is a plain C++ store; there is no inline assembly and there are no atomics.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "pair_kernels.h"

namespace gtnx {
namespace {

// every entry of the pair's rows from `i0` (tokens) and `t0` (frames) on: what no path covers
template <int WG>
__device__ __forceinline__ void fill_rows(const AsgTokenAlignArgs& a, int64_t p, int i0, int t0) {
  const int tid = static_cast<int>(threadIdx.x);
  for (int i = i0 + tid; i < a.L; i += WG) {
    a.starts[p * a.out_stride + i] = -1;
    a.ends[p * a.out_stride + i] = -1;
    if (a.token_scores) a.token_scores[p * a.out_stride + i] = NEG_INF;
  }
  if (a.frame_tokens)
    for (int t = t0 + tid; t < a.M; t += WG) a.frame_tokens[p * a.frame_stride + t] = -1;
}

template <int WG, int PER>
__global__ __launch_bounds__(WG) void asg_token_align_kernel(AsgTokenAlignArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_f[];
  const int U = a.U;
  const int W = U + 1;  // one -inf cell in front of each row
  const int tid = static_cast<int>(threadIdx.x);
  const int64_t p = a.pair0 + static_cast<int64_t>(blockIdx.x);
  const int b = static_cast<int>(p / a.N);
  const int T = min(max(a.frames[b], 0), a.M);
  const int len = min(max(a.lengths[p], 0), a.L);
  GTNX_G float* out = a.scores + p;
  if (len == 0 || len > U || T < len) {  // (uniform)
    if (tid == 0) *out = NEG_INF;
    fill_rows<WG>(a, p, 0, 0);
    return;
  }
  const GTNX_G int* tok = a.tokens + p * a.row_stride;
  // the labels and the gathered weights of the lane's positions; nothing is gathered through a token that is no label
  int lab[PER];
  float wself[PER], wstep[PER];
  int bad = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = tid + j * WG;
    lab[j] = 0;
    wself[j] = wstep[j] = NEG_INF;
    if (i < len) {
      const int v = tok[i];
      const int u = i > 0 ? tok[i - 1] : 0;
      if (v < 0 || v >= a.C || u < 0 || u >= a.C) {
        bad = 1;
      } else {
        lab[j] = v;
        const int64_t row = static_cast<int64_t>(a.C) + static_cast<int64_t>(v) * a.C;
        wself[j] = a.table[row + v];
        wstep[j] = i > 0 ? a.table[row + u] : a.table[v];
      }
    }
  }
  if (wg_any<WG>(bad)) {  // (uniform)
    if (tid == 0) *out = NEG_INF;
    fill_rows<WG>(a, p, 0, 0);
    return;
  }
  GTNX_G unsigned* bp = a.bp + static_cast<int64_t>(blockIdx.x) * a.pair_stride;
  const GTNX_G float* em = a.em + static_cast<int64_t>(b) * a.M * a.C;
  if (tid == 0) {
    s_f[0] = NEG_INF;
    s_f[W] = NEG_INF;
  }
  float e[PER];
  unsigned word[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    e[j] = tid + j * WG < len ? em[lab[j]] : NEG_INF;
    word[j] = 0;
  }
  int cur = 0;
  for (int t = 0; t < T; ++t) {
    float en[PER];
    if (t + 1 < T) {
      const GTNX_G float* row = em + static_cast<int64_t>(t + 1) * a.C;
#pragma unroll
      for (int j = 0; j < PER; ++j) en[j] = tid + j * WG < len ? row[lab[j]] : NEG_INF;
    } else {
#pragma unroll
      for (int j = 0; j < PER; ++j) en[j] = NEG_INF;
    }
    const float* prev = s_f + cur * W;
    float* next = s_f + (cur ^ 1) * W;
    const int sh = t & 31;
    const bool flush = sh == 31 || t == T - 1;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int i = tid + j * WG;
      if (i < len) {
        float v;
        unsigned k = 1u;
        if (t == 0) {  // (uniform) the start arc into position 0
          v = i == 0 ? 0.0f + (wstep[j] + e[j]) : NEG_INF;
        } else {
          const float c0 = prev[1 + i] + (wself[j] + e[j]), c1 = prev[i] + (wstep[j] + e[j]);
          // of two equal candidates the step: its source left the reference's queue first
          k = c1 >= c0 ? 1u : 0u;
          v = fmaxf(c0, c1);
        }
        next[1 + i] = v;
        word[j] |= k << sh;
        if (flush) {
          bp[static_cast<int64_t>(t >> 5) * U + i] = word[j];
          word[j] = 0;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) e[j] = en[j];
    wg_sync<WG>();
    cur ^= 1;
  }
  const float sc = s_f[cur * W + len];
  if (!(sc > NEG_INF)) {  // (uniform: every lane read the same cell)
    if (tid == 0) *out = NEG_INF;
    fill_rows<WG>(a, p, 0, 0);
    return;
  }
  if (tid == 0) *out = sc;
  fill_rows<WG>(a, p, len, T);
  wg_sync<WG>();  // (every lane has read the last row: the spans take its place)
  int* s_start = reinterpret_cast<int*>(s_f);  // [len]
  int* s_end = s_start + U;                    // [len]
  for (int i = tid; i < len; i += WG) {
    s_start[i] = -1;
    s_end[i] = -1;
  }
  wg_sync<WG>();  // (... and the back-pointer words of every wave are stored)
  if (tid < 64) {
    const int lane = tid;
    GTNX_G int* ft = a.frame_tokens ? a.frame_tokens + p * a.frame_stride : nullptr;
    const int NR = (T + 31) >> 5;
    int node = __builtin_amdgcn_readfirstlane(len - 1);
    // the window of word row r anchored at `top`: lane i holds the word of position top - i
    auto fetch = [&](int r, int top) { return bp[static_cast<int64_t>(r) * U + max(top - lane, 0)]; };
    int top = node;
    unsigned w = fetch(NR - 1, top), n = 0;
    int pn = 0;      // lane t % 64: the position of frame t
    int carry = -2;  // the position of the first frame of the 64 frames stored last (none yet)
    for (int r = NR - 1; r >= 0; --r) {
      const int ntop = node;
      if (r > 0) n = fetch(r - 1, ntop);
#pragma unroll
      for (int u = 31; u >= 0; --u) {
        const int t = r * 32 + u;
        if (t < T) {
          if (lane == (t & 63)) pn = node;
          const int off = min(max(top - node, 0), 63);  // (0 .. 63 on a path)
          const unsigned wv = unsigned(__builtin_amdgcn_readlane(int(w), off));
          const unsigned k = (wv >> u) & 1u;
          node -= int(min(k, unsigned(node)));
          if ((t & 63) == 0) {  // frames t .. t + 63, one per lane
            const int f = t + lane;
            int nb = __shfl_down(pn, 1);
            if (lane == 63) nb = carry;
            if (f + 1 >= T) nb = -2;
            if (f < T) {
              if (ft) ft[f] = pn;
              if (pn != nb) {
                s_end[pn] = f + 1;
                if (nb >= 0) s_start[nb] = f + 1;
              }
              if (f == 0) s_start[pn] = 0;
            }
            carry = __shfl(pn, 0);
          }
        }
      }
      w = n;
      top = ntop;
    }
  }
  wg_sync<WG>();
  for (int i = tid; i < len; i += WG) {
    const int st = s_start[i], en = s_end[i];
    a.starts[p * a.out_stride + i] = st;
    a.ends[p * a.out_stride + i] = en;
    if (a.token_scores) {
      float sum = NEG_INF;
      if (st >= 0 && en > st && en <= T) {
        const GTNX_G float* col = em + tok[i];
        sum = col[static_cast<int64_t>(st) * a.C];
        for (int t = st + 1; t < en; ++t) sum += col[static_cast<int64_t>(t) * a.C];
      }
      a.token_scores[p * a.out_stride + i] = sum;
    }
  }
}

// the alpha rows; the spans take their place behind the sweep (2 U ints)
size_t token_align_lds(int U) { return sizeof(float) * 2 * size_t(U + 1); }

template <int WG, int PER>
void launch(const AsgTokenAlignArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((asg_token_align_kernel<WG, PER>), dim3(static_cast<unsigned>(a.count)), dim3(WG),
                     token_align_lds(a.U), st, a);
}

}  // namespace

// fn<WG, PER>(a, st) with the width and the positions per lane asg_score_config gives for max_length a.U
#define GTNX_ASG_TOKEN_ALIGN_DISPATCH(fn)              \
  do {                                                 \
    int wg, per;                                       \
    asg_score_config(a.U, &wg, &per);                  \
    if (wg == 64) fn<64, 1>(a, st);                    \
    else if (wg == 256 && per == 1) fn<256, 1>(a, st); \
    else if (wg == 256) fn<256, 3>(a, st);             \
    else if (per == 1) fn<1024, 1>(a, st);             \
    else if (per == 2) fn<1024, 2>(a, st);             \
    else fn<1024, 4>(a, st);                           \
  } while (0)

void launch_asg_token_align(const AsgTokenAlignArgs& a, hipStream_t st) {
  if (a.count <= 0) return;
  GTNX_ASG_TOKEN_ALIGN_DISPATCH(launch);
}

}  // namespace gtnx
