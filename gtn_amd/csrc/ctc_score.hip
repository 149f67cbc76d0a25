// ctc_score.hip -- the exact log score of device-resident hypotheses under shared emission slabs, and its gradient
// (DESIGN section 22 holds the contract; tests/ctc_score_fp.py has the same recurrences in the same order in numpy).
//
// Pair p = b * N + k is the hypothesis y = tokens[p * row_stride .. + len), len = clamp(lengths[p], 0, L), of utterance
// b; its states are those of ctc_target_graph: s = 0 .. 2 len, even states carry `blank`, state 2 i + 1 carries y[i],
// and the arc s - 2 -> s exists for an odd s > 1 whose token differs from the one before (tokens are compared with each
// other only: a token equal to `blank` is a label like any other).  score = log sum over alignments, nothing subtracted.
//
//   forward:  one workgroup per pair.  A lane owns the states tid, tid + WG, ... (PER of them; labels and skip flags in
//             registers), the alpha row ping-pongs in LDS behind two -inf cells so that s - 1 and s - 2 need no branch:
//             one barrier per frame, none but a wave-level fence when the workgroup is one wave.  The emissions of the
//             next frame are loaded before the barrier.  alpha_t[s] = logadd(logadd(alpha[s], alpha[s - 1]), alpha[s - 2]
//             if skip) + e(t, label(s)); score = logadd(alpha[S - 1], alpha[S - 2]).  With a.alpha non-null every row
//             is also stored (the backward's recomputation), else nothing but the score is.
//   backward: one workgroup per utterance walks its pairs in k order.  Per pair it chains the odd states of equal token
//             (nxt[i] = the next index with the same token; the first one is the chain's head), then runs beta from the
//             last frame down: m[s] = beta[s] + e(t, label(s)) ping-pongs in LDS, beta_{t-1}[s] = logadd(logadd(m[s],
//             m[s + 1]), m[s + 2] if skip).  The occupancies g = exp(alpha + beta - score) of a frame are summed per
//             label in ONE order: the even (blank) states by lane (ascending state), then the xor tree of the wave,
//             then the waves ascending; a token's chain by its head, ascending index, the blank's sum in front when the
//             token is `blank`.  grad[b][t][label] = grad[b][t][label] + w * sum is a plain load (issued before the
//             frame's barrier, so that it is not waited for behind it) and store by the one lane that owns the label
//             in that frame, pairs in k order with a barrier between them: no atomics, and
//             the same bits whichever way the pairs are cut into launches.  The workgroup that holds k == 0 zeroes the
//             utterance's slab first, pad rows included.
// The width WG and PER come from 2 U + 1 alone (ctc_score_config), so a cut into slices changes no order of sums.
// Tokens are checked against 0 .. C - 1 before one becomes an address; nothing at or past a length or a frame count is
// read.  Every store is a plain C++ store; there is no inline assembly.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

#include "kernels.h"
#include "pair_kernels.h"

namespace gtnx {
namespace {

// what a lane keeps of its states: s = tid + j * WG
template <int PER>
struct Own {
  int lab[PER];    // the state's label (a valid one, or 0 for a state past S)
  bool skip[PER];  // forward: the arc s - 2 -> s exists; backward: the arc s -> s + 2 exists
};

// Reads the labels of the lane's states into its registers; true (in every lane, behind a barrier) when a token inside
// the length is no label.  BACKWARD selects which skip flag is kept.
template <int WG, int PER, bool BACKWARD>
__device__ __forceinline__ bool load_states(const CtcScoreArgs& a, const GTNX_G int* tok, int len, Own<PER>& o) {
  const int S = 2 * len + 1;
  const int tid = static_cast<int>(threadIdx.x);
  int bad = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int s = tid + j * WG;
    o.lab[j] = a.blank;
    o.skip[j] = false;
    if (s < S && (s & 1)) {
      const int i = s >> 1;
      const int v = tok[i];
      if (v < 0 || v >= a.C) {
        bad = 1;
        o.lab[j] = 0;
      } else {
        o.lab[j] = v;
        if (!BACKWARD) o.skip[j] = i > 0 && tok[i - 1] != v;
        else o.skip[j] = i + 1 < len && tok[i + 1] != v;
      }
    }
  }
  return wg_any<WG>(bad);
}

template <int WG, int PER>
__global__ __launch_bounds__(WG) void ctc_score_forward_kernel(CtcScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_f[];
  const int SM = 2 * a.U + 1;
  const int W = SM + 3;  // two -inf cells in front of each row
  const int tid = static_cast<int>(threadIdx.x);
  const int64_t p = a.pair0 + static_cast<int64_t>(blockIdx.x);
  const int b = static_cast<int>(p / a.N);
  const int T = min(max(a.frames[b], 0), a.M);
  const int len = min(max(a.lengths[p], 0), a.L);
  GTNX_G float* out = a.scores + (p - a.score0);
  if (len > a.U || T == 0) {  // (uniform)
    if (tid == 0) *out = NEG_INF;
    return;
  }
  const int S = 2 * len + 1;
  Own<PER> o;
  if (load_states<WG, PER, false>(a, a.tokens + p * a.row_stride, len, o)) {
    if (tid == 0) *out = NEG_INF;
    return;
  }
  GTNX_G float* keep = a.alpha ? a.alpha + static_cast<int64_t>(blockIdx.x) * a.pair_stride : nullptr;
  const GTNX_G float* em = a.em + static_cast<int64_t>(b) * a.M * a.C;
  if (tid < 2) {
    s_f[tid] = NEG_INF;
    s_f[W + tid] = NEG_INF;
  }
  float e[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) e[j] = tid + j * WG < S ? em[o.lab[j]] : NEG_INF;
  int cur = 0;
  // frame 0: the start state and the first label
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int s = tid + j * WG;
    if (s < S) {
      const float v = s < 2 ? e[j] : NEG_INF;
      s_f[2 + s] = v;
      if (keep) keep[s] = v;
    }
  }
  for (int t = 1; t < T; ++t) {
    const GTNX_G float* row = em + static_cast<int64_t>(t) * a.C;
#pragma unroll
    for (int j = 0; j < PER; ++j)
      if (tid + j * WG < S) e[j] = row[o.lab[j]];
    wg_sync<WG>();
    const float* prev = s_f + cur * W;
    float* next = s_f + (cur ^ 1) * W;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int s = tid + j * WG;
      if (s < S) {
        float x = logadd(prev[2 + s], prev[1 + s]);
        if (o.skip[j]) x = logadd(x, prev[s]);
        const float v = x == NEG_INF ? NEG_INF : x + e[j];
        next[2 + s] = v;
        if (keep) keep[static_cast<int64_t>(t) * SM + s] = v;
      }
    }
    cur ^= 1;
  }
  wg_sync<WG>();
  if (tid == 0) {
    const float* last = s_f + cur * W + 2;
    *out = S == 1 ? last[0] : logadd(last[S - 1], last[S - 2]);
  }
}

template <int WG, int PER>
__global__ __launch_bounds__(WG) void ctc_score_backward_kernel(CtcScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_f[];
  constexpr int NW = WG / 64;
  const int SM = 2 * a.U + 1;
  const int W = SM + 3;                                     // two -inf cells behind each row's last state
  float* s_m = s_f;                                          // [2][W]
  float* s_g = s_m + 2 * W;                                  // [2][U]: the occupancies of the odd states
  float* s_part = s_g + 2 * a.U;                             // [2][16]: the waves' sums over the even states
  int* s_nxt = reinterpret_cast<int*>(s_part + 32);          // [U]
  int* s_tok = s_nxt + a.U;                                  // [U]
  int* s_flag = s_tok + a.U;                                 // [1]: a chain's head carries `blank`
  const int tid = static_cast<int>(threadIdx.x);
  const int lane = tid & 63, wave = tid >> 6;
  const int b = static_cast<int>(a.pair0 / a.N) + static_cast<int>(blockIdx.x);
  const int64_t first = max(a.pair0, static_cast<int64_t>(b) * a.N);
  const int64_t end = min(a.pair0 + a.count, static_cast<int64_t>(b + 1) * a.N);
  const int T = min(max(a.frames[b], 0), a.M);
  const int64_t slab = static_cast<int64_t>(a.M) * a.C;
  GTNX_G float* grad = a.grad + static_cast<int64_t>(b) * slab;
  const GTNX_G float* em = a.em + static_cast<int64_t>(b) * slab;
  if (first == static_cast<int64_t>(b) * a.N)
    for (int64_t i = tid; i < slab; i += WG) grad[i] = 0.0f;
  wg_sync<WG>();

  for (int64_t p = first; p < end; ++p) {
    const float w = a.weights[p];
    const float sc = a.scores[p - a.score0];
    const int len = min(max(a.lengths[p], 0), a.L);
    // (uniform; a score above -inf says there is a path: T > 0, len <= U, every token a label -- and NaN is no score)
    if (w == 0.0f || !(sc > NEG_INF) || len > a.U || T == 0) continue;
    const int S = 2 * len + 1;
    const GTNX_G int* tok = a.tokens + p * a.row_stride;
    Own<PER> o;
    for (int i = tid; i < len; i += WG) s_tok[i] = tok[i];
    if (tid == 0) *s_flag = 0;
    if (tid < 2) {
      s_m[S + tid] = NEG_INF;
      s_m[W + S + tid] = NEG_INF;
    }
    if (load_states<WG, PER, true>(a, tok, len, o)) continue;  // (uniform; it is also the barrier behind s_tok)
    // the chains of equal tokens: ascending index, the first one is the head
    bool head[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int s = tid + j * WG;
      head[j] = false;
      if (s < S && (s & 1)) {
        const int i = s >> 1, v = o.lab[j];
        bool seen = false;
        for (int q = 0; q < i && !seen; ++q) seen = s_tok[q] == v;
        int nx = -1;
        for (int q = i + 1; q < len && nx < 0; ++q)
          if (s_tok[q] == v) nx = q;
        s_nxt[i] = nx;
        head[j] = !seen;
        if (!seen && v == a.blank) *s_flag = 1;
      }
    }
    const GTNX_G float* al = a.alpha + (p - a.pair0) * a.pair_stride;
    float beta[PER], av[PER], e[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int s = tid + j * WG;
      beta[j] = s < S && s >= S - 2 ? 0.0f : NEG_INF;
      av[j] = e[j] = NEG_INF;
      if (s < S) {
        av[j] = al[static_cast<int64_t>(T - 1) * SM + s];
        e[j] = em[static_cast<int64_t>(T - 1) * a.C + o.lab[j]];
      }
    }
    wg_sync<WG>();  // (the chains and the flag)
    const bool blank_in_chain = *s_flag != 0;
    int pp = 0;
    for (int t = T - 1; t >= 0; --t) {
      float* m = s_m + pp * W;
      float* g = s_g + pp * a.U;
      float* part = s_part + pp * 16;
      float ev = 0.0f;
      GTNX_G float* row = grad + static_cast<int64_t>(t) * a.C;
      // (what this frame adds to is loaded now, so that the load is not waited for behind the barrier)
      float old[PER], old_blank = 0.0f;
#pragma unroll
      for (int j = 0; j < PER; ++j) old[j] = head[j] ? row[o.lab[j]] : 0.0f;
      if (tid == 0 && !blank_in_chain) old_blank = row[a.blank];
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        const int s = tid + j * WG;
        if (s < S) {
          const float x = av[j] > NEG_INF && beta[j] > NEG_INF ? expf(av[j] + beta[j] - sc) : 0.0f;
          m[s] = beta[j] == NEG_INF ? NEG_INF : beta[j] + e[j];
          if (s & 1) g[s >> 1] = x;
          else ev += x;
        }
      }
      for (int off = 32; off > 0; off >>= 1) ev += __shfl_xor(ev, off);
      if (lane == 0) part[wave] = ev;
      if (t > 0) {
#pragma unroll
        for (int j = 0; j < PER; ++j) {
          const int s = tid + j * WG;
          if (s < S) {
            av[j] = al[static_cast<int64_t>(t - 1) * SM + s];
            e[j] = em[static_cast<int64_t>(t - 1) * a.C + o.lab[j]];
          }
        }
      }
      wg_sync<WG>();
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        const int s = tid + j * WG;
        if (s < S) {
          float x = logadd(m[s], m[s + 1]);
          if (o.skip[j]) x = logadd(x, m[s + 2]);
          beta[j] = x;
          if (head[j]) {
            const int i = s >> 1;
            float sum = g[i];
            if (o.lab[j] == a.blank) {
              float evs = part[0];
              for (int q = 1; q < NW; ++q) evs += part[q];
              sum = evs + sum;
            }
            for (int q = s_nxt[i]; q >= 0; q = s_nxt[q]) sum += g[q];
            row[o.lab[j]] = old[j] + w * sum;
          }
        }
      }
      if (tid == 0 && !blank_in_chain) {
        float evs = part[0];
        for (int q = 1; q < NW; ++q) evs += part[q];
        row[a.blank] = old_blank + w * evs;
      }
      pp ^= 1;
    }
    wg_sync<WG>();  // (the next pair reuses the rows, and reads what this one added)
  }
}

size_t forward_lds(int U) { return sizeof(float) * 2 * size_t(2 * U + 4); }
size_t backward_lds(int U) { return sizeof(float) * (2 * size_t(2 * U + 4) + 4 * size_t(U) + 32 + 4); }

template <int WG, int PER>
void launch_forward(const CtcScoreArgs& a, hipStream_t st) {
  static std::atomic<uint64_t> done{0};
  if (gtnx_first_on_device first{done})
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(ctc_score_forward_kernel<WG, PER>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, int(forward_lds(kCtcScoreMaxU)));
  hipLaunchKernelGGL((ctc_score_forward_kernel<WG, PER>), dim3(static_cast<unsigned>(a.count)), dim3(WG),
                     forward_lds(a.U), st, a);
}

template <int WG, int PER>
void launch_backward(const CtcScoreArgs& a, hipStream_t st) {
  static std::atomic<uint64_t> done{0};
  if (gtnx_first_on_device first{done})
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(ctc_score_backward_kernel<WG, PER>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, int(backward_lds(kCtcScoreMaxU)));
  const int64_t b0 = a.pair0 / a.N, b1 = (a.pair0 + a.count - 1) / a.N;
  hipLaunchKernelGGL((ctc_score_backward_kernel<WG, PER>), dim3(static_cast<unsigned>(b1 - b0 + 1)), dim3(WG),
                     backward_lds(a.U), st, a);
}

}  // namespace

// one wave without barriers while every state has a lane; beyond the widest workgroup a lane owns several states
void ctc_score_config(int U, int* width, int* per_lane) {
  const int SM = 2 * U + 1;
  int wg, per;
  if (SM <= 64) wg = 64, per = 1;
  else if (SM <= 256) wg = 256, per = 1;
  else if (SM <= 768) wg = 256, per = 3;
  else if (SM <= 1024) wg = 1024, per = 1;
  else if (SM <= 2048) wg = 1024, per = 2;
  else if (SM <= 4096) wg = 1024, per = 4;
  else wg = 1024, per = 9;
  if (width) *width = wg;
  if (per_lane) *per_lane = per;
}

void launch_ctc_score_forward(const CtcScoreArgs& a, hipStream_t st) {
  if (a.count <= 0) return;
  GTNX_CTC_SCORE_DISPATCH(a.U, launch_forward, a, st);
}

void launch_ctc_score_backward(const CtcScoreArgs& a, hipStream_t st) {
  if (a.count <= 0) return;
  GTNX_CTC_SCORE_DISPATCH(a.U, launch_backward, a, st);
}

}  // namespace gtnx
