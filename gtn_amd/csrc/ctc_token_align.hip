// ctc_token_align.hip -- the best alignment of device-resident hypotheses under shared emission slabs: per token its
// first frame, one past its last frame and its summed emissions, per hypothesis the Viterbi score, per frame (optional)
// the token index (DESIGN section 24 holds the contract; tests/ctc_token_align_fp.py is the same arithmetic in numpy).
//
// Pair p = b * N + k is the hypothesis y = tokens[p * row_stride .. + len), len = clamp(lengths[p], 0, L), of utterance
// b with T_b frames; its states are those of ctc_score.hip: s = 0 .. 2 len, even states carry `blank`, state 2 i + 1
// carries y[i], a frame enters s from s and s - 1, and from s - 2 for an odd s > 1 whose token differs from the one
// before (a token equal to `blank` is a label like any other).  Paths start in state 0 before frame 0 and end in state
// 2 len or 2 len - 1 behind frame T_b - 1.
//
//   arithmetic: float32, that of align.hip: a candidate is alpha[src] + e(t, label(s)), one addition; the new value is
//             the exact maximum; a state whose maximum is -inf is dead.  Of the candidates that reach the maximum the
//             one whose SOURCE has the smallest rank wins, the ranks being align.hip's queue_rank: with U = len, S =
//             2 U + 1 and p leading strict ascents y[0] < .. < y[p]
//               0 | (2i, 2i-1) for i = 1..p | S-1 | for i = U-1 down to p+1: (2i, 2i+1) if y[i] != y[i-1] else
//               (2i+1, 2i) | 2p+1
//             p comes from the tokens here (a workgroup minimum over the first i with y[i] <= y[i-1]); of two equal end
//             states the smaller wins.  Every output is reproducible bit for bit.
//   sweep:    one workgroup per pair, width and states per lane from ctc_score_config(max_length).  A lane owns the
//             states tid, tid + WG, ...; the alpha row ping-pongs in LDS behind two -inf cells, one barrier per frame,
//             the next frame's emissions loaded before it.  A lane packs the 2-bit code (0, 1, 2: the source s - code;
//             3: dead) of each of its states over 16 frames into one word and stores bp[(t / 16) * (2 U + 1) + s]
//             every 16th frame and at T_b - 1: coalesced stores, 2 bits per state and frame.
//   walk:     wave 0, behind a workgroup barrier (the words are the other waves' stores).  In 16 frames the path
//             descends at most 32 states, so a word row is ONE window load: lane i holds the word of state top - i (and
//             a second register that of state top - 64 - i), anchored at the state the path had a row earlier; the 16
//             steps run in registers by readlane while the next row's window, anchored at the state the path has now,
//             is in flight.  T / 16 dependent loads per pair instead of T.  Lane t % 64 keeps the state of step t;
//             every 64 steps the wave stores frame_tokens and notes, where the token index changes between
//             neighbouring frames, starts[i] / ends[i] in LDS (the alpha rows are free by then).
//   tokens:   behind a second barrier lane i (striding over the tokens) sums e(t, y[i]) over t = starts[i] .. ends[i] - 1
//             in ascending order, starting from the first frame's value, and stores starts, ends and token_scores.
// Entries no path covers (i >= len, t >= T_b, every entry of a pair without a path) are written -1 / -inf by the same
// workgroup: every element of every row is written over the widths L and M, nothing beyond them.  No path: len > U, a
// token inside the length outside 0 .. C - 1 (checked before one becomes an address), T_b == 0, or a best end state at
// -inf.  Nothing at or past a length or a frame count is read.  NaN emissions give unspecified values, never an access
// outside the pair's rows: a code never leads below state 0, offsets into a window are clamped, and a token whose span
// was not noted gets -inf without a read.  Every store is a plain C++ store; there is no inline assembly.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

#include "kernels.h"
#include "pair_kernels.h"

namespace gtnx {
namespace {

// position of state m in the reference's queue (align.hip queue_rank, with the skip flag read from the tokens)
__device__ __forceinline__ int queue_rank(int m, int S, int p, const GTNX_G int* tok) {
  if (m < 0 || m >= S) return 0x7ffffffe;
  const int U = (S - 1) >> 1;
  if (m == 0) return 0;
  if (m == 2 * U) return 2 * p + 1;
  if (m == 2 * p + 1) return 2 * U;
  if (m <= 2 * p) return (m & 1) ? m + 1 : m - 1;
  const int i = m >> 1;  // states 2i and 2i+1, p < i < U
  const bool skip = tok[i] != tok[i - 1];
  const bool even = (m & 1) == 0;
  return 2 * p + 2 + 2 * (U - 1 - i) + (even == skip ? 0 : 1);
}

// every entry of the pair's rows from `i0` (tokens) and `t0` (frames) on: what no path covers
template <int WG>
__device__ __forceinline__ void fill_rows(const CtcTokenAlignArgs& a, int64_t p, int i0, int t0) {
  const int tid = static_cast<int>(threadIdx.x);
  for (int i = i0 + tid; i < a.L; i += WG) {
    a.starts[p * a.out_stride + i] = -1;
    a.ends[p * a.out_stride + i] = -1;
    if (a.token_scores) a.token_scores[p * a.out_stride + i] = NEG_INF;
  }
  if (a.frame_tokens)
    for (int t = t0 + tid; t < a.M; t += WG) a.frame_tokens[p * a.frame_stride + t] = -1;
}

constexpr int F_SKIP = 1, F_01 = 2, F_02 = 4, F_12 = 8;  // the arc s - 2 -> s exists; rank(s - x) < rank(s - y)

template <int WG, int PER>
__global__ __launch_bounds__(WG) void ctc_token_align_kernel(CtcTokenAlignArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_f[];
  __shared__ int s_first;  // the first i with y[i] <= y[i - 1], len if there is none
  __shared__ int s_bad;
  const int SM = 2 * a.U + 1;
  const int W = SM + 3;  // two -inf cells in front of each row
  const int tid = static_cast<int>(threadIdx.x);
  const int64_t p = a.pair0 + static_cast<int64_t>(blockIdx.x);
  const int b = static_cast<int>(p / a.N);
  const int T = min(max(a.frames[b], 0), a.M);
  const int len = min(max(a.lengths[p], 0), a.L);
  GTNX_G float* out = a.scores + p;
  if (len > a.U || T == 0) {  // (uniform)
    if (tid == 0) *out = NEG_INF;
    fill_rows<WG>(a, p, 0, 0);
    return;
  }
  const int S = 2 * len + 1;
  const GTNX_G int* tok = a.tokens + p * a.row_stride;
  if (tid == 0) {
    s_first = len;
    s_bad = 0;
  }
  wg_sync<WG>();
  int lab[PER];
  {
    int bad = 0, first = len;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int s = tid + j * WG;
      lab[j] = a.blank;
      if (s < S && (s & 1)) {
        const int i = s >> 1;
        const int v = tok[i];
        if (v < 0 || v >= a.C) {
          bad = 1;
          lab[j] = 0;
        } else {
          lab[j] = v;
        }
        if (i > 0 && v <= tok[i - 1]) first = min(first, i);
      }
    }
    if (bad) s_bad = 1;
    if (first < len) atomicMin(&s_first, first);
  }
  wg_sync<WG>();
  if (s_bad) {  // (uniform)
    if (tid == 0) *out = NEG_INF;
    fill_rows<WG>(a, p, 0, 0);
    return;
  }
  const int asc = max(s_first, 1) - 1;  // the leading strict ascents y[0] < .. < y[asc]
  int flags[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int s = tid + j * WG;
    flags[j] = 0;
    if (s < S) {
      const int r0 = queue_rank(s, S, asc, tok), r1 = queue_rank(s - 1, S, asc, tok), r2 = queue_rank(s - 2, S, asc, tok);
      const bool skip = (s & 1) && s > 1 && tok[s >> 1] != tok[(s >> 1) - 1];
      flags[j] = (skip ? F_SKIP : 0) | (r0 < r1 ? F_01 : 0) | (r0 < r2 ? F_02 : 0) | (r1 < r2 ? F_12 : 0);
    }
  }
  GTNX_G unsigned* bp = a.bp + static_cast<int64_t>(blockIdx.x) * a.pair_stride;
  const GTNX_G float* em = a.em + static_cast<int64_t>(b) * a.M * a.C;
  if (tid < 2) {
    s_f[tid] = NEG_INF;
    s_f[W + tid] = NEG_INF;
  }
  float e[PER];
  unsigned word[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int s = tid + j * WG;
    e[j] = s < S ? em[lab[j]] : NEG_INF;
    word[j] = 0;
    if (s < S) s_f[2 + s] = s == 0 ? 0.0f : NEG_INF;  // before frame 0
  }
  wg_sync<WG>();
  int cur = 0;
  for (int t = 0; t < T; ++t) {
    float en[PER];
    if (t + 1 < T) {
      const GTNX_G float* row = em + static_cast<int64_t>(t + 1) * a.C;
#pragma unroll
      for (int j = 0; j < PER; ++j) en[j] = tid + j * WG < S ? row[lab[j]] : NEG_INF;
    } else {
#pragma unroll
      for (int j = 0; j < PER; ++j) en[j] = NEG_INF;
    }
    const float* prev = s_f + cur * W;
    float* next = s_f + (cur ^ 1) * W;
    const int sh = (t & 15) * 2;
    const bool flush = (t & 15) == 15 || t == T - 1;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int s = tid + j * WG;
      if (s < S) {
        const int f = flags[j];
        const float c0 = prev[2 + s] + e[j], c1 = prev[1 + s] + e[j], c2 = (f & F_SKIP) ? prev[s] + e[j] : NEG_INF;
        const float best = fmaxf(fmaxf(c0, c1), c2);
        // of the candidates that reach the maximum, the one from the source with the smallest rank
        const bool t0 = c0 == best, t1 = c1 == best, t2 = c2 == best;
        unsigned k = (t0 && (!t1 || (f & F_01)) && (!t2 || (f & F_02))) ? 0u : ((t1 && (!t2 || (f & F_12))) ? 1u : (t2 ? 2u : 0u));
        k = best == NEG_INF ? 3u : k;
        next[2 + s] = best;
        word[j] |= k << sh;
        if (flush) {
          bp[static_cast<int64_t>(t >> 4) * SM + s] = word[j];
          word[j] = 0;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) e[j] = en[j];
    wg_sync<WG>();
    cur ^= 1;
  }
  // the best end state: the maximum, the smaller state among equals
  const float* last = s_f + cur * W + 2;
  float sc = last[S - 1];
  int best = S - 1;
  if (S > 1) {
    const float a2 = last[S - 2];
    sc = fmaxf(sc, a2);
    if (a2 == sc) best = S - 2;
  }
  if (!(sc > NEG_INF)) {  // (uniform: every lane read the same two cells)
    if (tid == 0) *out = NEG_INF;
    fill_rows<WG>(a, p, 0, 0);
    return;
  }
  if (tid == 0) *out = sc;
  fill_rows<WG>(a, p, len, T);
  wg_sync<WG>();  // (every lane has read the last row: the spans take its place)
  int* s_start = reinterpret_cast<int*>(s_f);  // [len]
  int* s_end = s_start + a.U;                  // [len]
  for (int i = tid; i < len; i += WG) {
    s_start[i] = -1;
    s_end[i] = -1;
  }
  wg_sync<WG>();  // (... and the back-pointer words of every wave are stored)
  if (tid < 64) {
    const int lane = tid;
    GTNX_G int* ft = a.frame_tokens ? a.frame_tokens + p * a.frame_stride : nullptr;
    const int NR = (T + 15) >> 4;
    int node = __builtin_amdgcn_readfirstlane(best);
    // the window of word row r anchored at `top`: lane i holds state top - i in w0 and state top - 64 - i in w1
    auto fetch = [&](int r, int top, unsigned& w0, unsigned& w1) {
      const GTNX_G unsigned* row = bp + static_cast<int64_t>(r) * SM;
      w0 = row[max(top - lane, 0)];
      w1 = row[max(top - 64 - lane, 0)];
    };
    unsigned w0, w1, n0 = 0, n1 = 0;
    int top = node;
    fetch(NR - 1, top, w0, w1);
    int pn = 0;       // lane t % 64: the state step t enters
    int carry = -2;   // the token index of the first frame of the 64 frames stored last (none yet)
    for (int r = NR - 1; r >= 0; --r) {
      const int ntop = node;
      if (r > 0) fetch(r - 1, ntop, n0, n1);
#pragma unroll
      for (int u = 15; u >= 0; --u) {
        const int t = r * 16 + u;
        if (t < T) {
          if (lane == (t & 63)) pn = node;
          const int off = min(max(top - node, 0), 127);  // (0 .. 64 on a path)
          const unsigned wv = off < 64 ? unsigned(__builtin_amdgcn_readlane(int(w0), off))
                                       : unsigned(__builtin_amdgcn_readlane(int(w1), off - 64));
          unsigned k = (wv >> (2 * u)) & 3u;
          k = k == 3u ? 0u : k;  // (a dead state: the best path never runs through one)
          node -= int(min(k, unsigned(node)));
          if ((t & 63) == 0) {  // frames t .. t + 63, one per lane
            const int f = t + lane;
            const int tk = (pn & 1) ? (pn >> 1) : -1;
            int nb = __shfl_down(tk, 1);
            if (lane == 63) nb = carry;
            if (f + 1 >= T) nb = -2;
            if (f < T) {
              if (ft) ft[f] = tk;
              if (tk != nb) {
                if (tk >= 0) s_end[tk] = f + 1;
                if (nb >= 0) s_start[nb] = f + 1;
              }
              if (f == 0 && tk >= 0) s_start[tk] = 0;
            }
            carry = __shfl(tk, 0);
          }
        }
      }
      w0 = n0;
      w1 = n1;
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
size_t token_align_lds(int U) { return sizeof(float) * 2 * size_t(2 * U + 4); }

template <int WG, int PER>
void launch(const CtcTokenAlignArgs& a, hipStream_t st) {
  static std::atomic<uint64_t> done{0};
  if (gtnx_first_on_device first{done})
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(ctc_token_align_kernel<WG, PER>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, int(token_align_lds(kCtcScoreMaxU)));
  hipLaunchKernelGGL((ctc_token_align_kernel<WG, PER>), dim3(static_cast<unsigned>(a.count)), dim3(WG),
                     token_align_lds(a.U), st, a);
}

}  // namespace

void launch_ctc_token_align(const CtcTokenAlignArgs& a, hipStream_t st) {
  if (a.count <= 0) return;
  GTNX_CTC_SCORE_DISPATCH(a.U, launch, a, st);
}

}  // namespace gtnx
