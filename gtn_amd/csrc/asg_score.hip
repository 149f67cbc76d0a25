// asg_score.hip -- the ASG force-align score of device-resident hypotheses under shared emission slabs, and its gradients
// with respect to the emissions and the [C + C * C] table of start and transition scores (DESIGN section 25 holds the
// contract; tests/asg_score_fp.py has the same recurrences in the same order in numpy).
//
// Pair p = b * N + k is the hypothesis y = tokens[p * row_stride .. + len), len = clamp(lengths[p], 0, L), of utterance
// b.  Position i = 0 .. len - 1 ("the first i + 1 labels are consumed") carries y[i]; a frame enters it from itself with
// w_self[i] = table[C + y[i] * C + y[i]] or from i - 1 with w_step[i] = table[C + y[i] * C + y[i - 1]] (position 0: from
// the start with table[y[0]], at frame 0 only) and emits e(t, y[i]).  Equal neighbours are legal; there is no blank.
//
//   forward:  one workgroup per pair.  A lane owns the positions tid, tid + WG, ... (PER of them; labels and the two
//             gathered weights in registers), the alpha row ping-pongs in LDS behind one -inf cell so that i - 1 needs
//             no branch: one barrier per frame, none but a wave-level fence when the workgroup is one wave.  The
//             emissions of the next frame are loaded before the barrier.  alpha_t[i] = logadd(alpha[i] + w_self[i],
//             alpha[i - 1] + w_step[i]) + e(t, y[i]); score = alpha_{T - 1}[len - 1].  With a.alpha non-null every row
//             is also stored (the backward's recomputation), else nothing but the score is.
//   backward: one workgroup per pair.  beta runs from the last frame down: q[i] = beta_t[i] + e(t, y[i]), m[i] = q[i] +
//             w_step[i] ping-pongs in LDS, beta_{t-1}[i] = logadd(q[i] + w_self[i], m[i + 1]).  The occupancies of frame
//             t are p_self[i] = exp(alpha_{t-1}[i] + w_self[i] + q[i] - score) and p_step[i] = exp(alpha_{t-1}[i - 1] +
//             w_step[i] + q[i] - score) (frame 0: p_step[0] = exp(w_step[0] + q[0] - score) alone).  Their sum takes
//             the place of alpha_t[i] in scratch (every lane has used row t, for frame t + 1, before the barrier that
//             precedes this store).  A lane also sums p_self[i] and p_step[i] over the frames (last frame first) in
//             registers and stores them, times w, into the pair's row of a.occ.
//   scatter:  one workgroup per (utterance, tile of 8 rows of its slab) walks the utterance's pairs in k order.  Per
//             pair it chains the positions of equal token (nxt[i] = the next index with the same token; the first one
//             is the chain's head); a head sums the occupancies of a frame along its chain, ascending index, and
//             grad[b][t][label] = grad[b][t][label] + w * sum is a plain load and store by the one lane that owns the
//             label in that frame, pairs in k order with a barrier between them: no atomics, and the same bits
//             whichever way the pairs are cut into launches.  The launch that holds k == 0 zeroes the rows first, pad
//             rows included.
//   table:    workgroup r < C owns the entries C + r * C .. of the transitions (label r entered), workgroup C the start
//             entries.  One wave walks the pairs in p order and the positions ascending; per 64 positions a ballot finds
//             those that carry label r, and they are added one at a time, lowest lane first, into an LDS row indexed
//             by the label before (position i: its self sum into [r] first, then its step sum into [y[i - 1]]).  The
//             start workgroup does the same over 64 pairs at a time with the step sum of position 0.  The row is then
//             stored, zeros included.  Pairs the backward skipped (weight 0, no score) are skipped by the same test.
// The width WG and PER come from U alone (asg_score_config), so a cut into slices changes no order of sums.  Tokens are
// checked against 0 .. C - 1 before one becomes an address; nothing at or past a length or a frame count is read.
// Every store is a plain C++ store; there is no inline assembly.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "pair_kernels.h"

namespace gtnx {
namespace {

// what a lane keeps of its positions: i = tid + j * WG
template <int PER>
struct Own {
  int lab[PER];       // the position's label (a valid one, or 0 for a position past len)
  float wself[PER];   // table[C + lab * C + lab]
  float wstep[PER];   // table[C + lab * C + label before], position 0: table[lab]
};

// Reads the labels and the gathered weights of the lane's positions into its registers; true (in every lane, behind a
// barrier) when a token inside the length is no label.  Nothing is gathered through a token that is none.
template <int WG, int PER>
__device__ __forceinline__ bool load_positions(const AsgScoreArgs& a, const GTNX_G int* tok, int len, Own<PER>& o) {
  const int tid = static_cast<int>(threadIdx.x);
  int bad = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = tid + j * WG;
    o.lab[j] = 0;
    o.wself[j] = o.wstep[j] = NEG_INF;
    if (i < len) {
      const int v = tok[i];
      const int u = i > 0 ? tok[i - 1] : 0;
      if (v < 0 || v >= a.C) {
        bad = 1;
      } else if (u >= 0 && u < a.C) {  // (a bad `u` is reported by the lane that owns it)
        o.lab[j] = v;
        const int64_t row = static_cast<int64_t>(a.C) + static_cast<int64_t>(v) * a.C;
        o.wself[j] = a.table[row + v];
        o.wstep[j] = i > 0 ? a.table[row + u] : a.table[v];
      }
    }
  }
  return wg_any<WG>(bad);
}

template <int WG, int PER>
__global__ __launch_bounds__(WG) void asg_score_forward_kernel(AsgScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_f[];
  const int W = a.U + 1;  // one -inf cell in front of each row
  const int tid = static_cast<int>(threadIdx.x);
  const int64_t p = a.pair0 + static_cast<int64_t>(blockIdx.x);
  const int b = static_cast<int>(p / a.N);
  const int T = min(max(a.frames[b], 0), a.M);
  const int len = min(max(a.lengths[p], 0), a.L);
  GTNX_G float* out = a.scores + (p - a.score0);
  if (len == 0 || len > a.U || T < len) {  // (uniform)
    if (tid == 0) *out = NEG_INF;
    return;
  }
  Own<PER> o;
  if (load_positions<WG, PER>(a, a.tokens + p * a.row_stride, len, o)) {
    if (tid == 0) *out = NEG_INF;
    return;
  }
  GTNX_G float* keep = a.alpha ? a.alpha + static_cast<int64_t>(blockIdx.x) * a.pair_stride : nullptr;
  const GTNX_G float* em = a.em + static_cast<int64_t>(b) * a.M * a.C;
  if (tid == 0) {
    s_f[0] = NEG_INF;
    s_f[W] = NEG_INF;
  }
  float e[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) e[j] = tid + j * WG < len ? em[o.lab[j]] : NEG_INF;
  int cur = 0;
  // frame 0: the start arc into position 0
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = tid + j * WG;
    if (i < len) {
      const float v = i == 0 ? o.wstep[j] + e[j] : NEG_INF;
      s_f[1 + i] = v;
      if (keep) keep[i] = v;
    }
  }
  for (int t = 1; t < T; ++t) {
    const GTNX_G float* row = em + static_cast<int64_t>(t) * a.C;
#pragma unroll
    for (int j = 0; j < PER; ++j)
      if (tid + j * WG < len) e[j] = row[o.lab[j]];
    wg_sync<WG>();
    const float* prev = s_f + cur * W;
    float* next = s_f + (cur ^ 1) * W;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int i = tid + j * WG;
      if (i < len) {
        const float x = logadd(prev[1 + i] + o.wself[j], prev[i] + o.wstep[j]);
        const float v = x + e[j];
        next[1 + i] = v;
        if (keep) keep[static_cast<int64_t>(t) * a.U + i] = v;
      }
    }
    cur ^= 1;
  }
  wg_sync<WG>();
  if (tid == 0) *out = s_f[cur * W + len];
}

template <int WG, int PER>
__global__ __launch_bounds__(WG) void asg_score_backward_kernel(AsgScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_f[];
  const int U = a.U;
  const int W = U + 1;  // one -inf cell behind each row's last position
  float* s_m = s_f;     // [2][W]
  const int tid = static_cast<int>(threadIdx.x);
  const int64_t p = a.pair0 + static_cast<int64_t>(blockIdx.x);
  const int b = static_cast<int>(p / a.N);
  const int T = min(max(a.frames[b], 0), a.M);
  const float w = a.weights[p];
  const float sc = a.scores[p - a.score0];
  const int len = min(max(a.lengths[p], 0), a.L);
  // (uniform; a score above -inf says there is a path: 0 < len <= U, len <= T, every token a label -- NaN is no score)
  if (w == 0.0f || !(sc > NEG_INF) || len == 0 || len > U || T < len) return;
  Own<PER> o;
  if (tid == 0) {
    s_m[len] = NEG_INF;
    s_m[W + len] = NEG_INF;
  }
  if (load_positions<WG, PER>(a, a.tokens + p * a.row_stride, len, o)) return;  // (uniform)
  const GTNX_G float* em = a.em + static_cast<int64_t>(b) * a.M * a.C;
  GTNX_G float* al = a.alpha + static_cast<int64_t>(blockIdx.x) * a.pair_stride;
  float beta[PER], as[PER], ap[PER], e[PER], sum_self[PER], sum_step[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = tid + j * WG;
    beta[j] = i == len - 1 ? 0.0f : NEG_INF;
    as[j] = ap[j] = e[j] = NEG_INF;
    sum_self[j] = sum_step[j] = 0.0f;
    if (i < len) {
      e[j] = em[static_cast<int64_t>(T - 1) * a.C + o.lab[j]];
      if (T > 1) {
        as[j] = al[static_cast<int64_t>(T - 2) * U + i];
        if (i > 0) ap[j] = al[static_cast<int64_t>(T - 2) * U + i - 1];
      } else if (i == 0) {
        ap[j] = 0.0f;  // (the start, before frame 0)
      }
    }
  }
  int pp = 0;
  for (int t = T - 1; t >= 0; --t) {
    float* m = s_m + pp * W;
    float qs[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int i = tid + j * WG;
      qs[j] = NEG_INF;
      if (i < len) {
        const float q = beta[j] + e[j];
        const float xs = as[j] + o.wself[j] + q;
        const float xp = ap[j] + o.wstep[j] + q;
        const float ps = xs > NEG_INF ? expf(xs - sc) : 0.0f;
        const float pt = xp > NEG_INF ? expf(xp - sc) : 0.0f;
        sum_self[j] += ps;
        sum_step[j] += pt;
        m[i] = q + o.wstep[j];
        qs[j] = q + o.wself[j];
        // (row t of the alphas was read for frame t + 1: the occupancy of frame t takes its place)
        if (a.grad) al[static_cast<int64_t>(t) * U + i] = ps + pt;
      }
    }
    if (t > 0) {
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        const int i = tid + j * WG;
        if (i < len) {
          e[j] = em[static_cast<int64_t>(t - 1) * a.C + o.lab[j]];
          as[j] = ap[j] = NEG_INF;
          if (t > 1) {
            as[j] = al[static_cast<int64_t>(t - 2) * U + i];
            if (i > 0) ap[j] = al[static_cast<int64_t>(t - 2) * U + i - 1];
          } else if (i == 0) {
            ap[j] = 0.0f;  // (the start, before frame 0)
          }
        }
      }
    }
    wg_sync<WG>();
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int i = tid + j * WG;
      if (i < len) beta[j] = logadd(qs[j], m[i + 1]);
    }
    pp ^= 1;
  }
  if (a.occ) {
    GTNX_G float* oc = a.occ + p * 2 * a.occ_half;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int i = tid + j * WG;
      if (i < len) {
        oc[i] = w * sum_self[j];
        oc[a.occ_half + i] = w * sum_step[j];
      }
    }
  }
}

// the frames a scatter workgroup adds: the grid is (utterances of the range, tiles of this many rows of the slab)
constexpr int kScatterFrames = 8;
constexpr int kScatterWG = 256;

__global__ __launch_bounds__(kScatterWG) void asg_score_scatter_kernel(AsgScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_f[];
  const int U = a.U;
  int* s_tok = reinterpret_cast<int*>(s_f);  // [U]
  int* s_nxt = s_tok + U;                    // [U]: the next index with the same token, -1 at a chain's end
  int* s_head = s_nxt + U;                   // [U]: the first index of its token
  const int tid = static_cast<int>(threadIdx.x);
  const int b = static_cast<int>(a.pair0 / a.N) + static_cast<int>(blockIdx.x);
  const int t0 = static_cast<int>(blockIdx.y) * kScatterFrames;
  const int t1 = min(t0 + kScatterFrames, a.M);
  const int64_t first = max(a.pair0, static_cast<int64_t>(b) * a.N);
  const int64_t end = min(a.pair0 + a.count, static_cast<int64_t>(b + 1) * a.N);
  const int T = min(max(a.frames[b], 0), a.M);
  GTNX_G float* grad = a.grad + static_cast<int64_t>(b) * a.M * a.C;
  if (first == static_cast<int64_t>(b) * a.N) {
    GTNX_G float* z = grad + static_cast<int64_t>(t0) * a.C;
    const int64_t cells = static_cast<int64_t>(t1 - t0) * a.C;
    for (int64_t i = tid; i < cells; i += kScatterWG) z[i] = 0.0f;
  }
  const int frames = min(t1, T) - t0;
  if (frames <= 0) return;  // (uniform: pad rows hold nothing but the zeros)
  __syncthreads();
  for (int64_t p = first; p < end; ++p) {
    const float w = a.weights[p];
    const float sc = a.scores[p - a.score0];
    const int len = min(max(a.lengths[p], 0), a.L);
    if (w == 0.0f || !(sc > NEG_INF) || len == 0 || len > U || T < len) continue;  // (uniform: the backward's test)
    const GTNX_G int* tok = a.tokens + p * a.row_stride;
    for (int i = tid; i < len; i += kScatterWG) s_tok[i] = tok[i];
    __syncthreads();
    // the chains of equal tokens: ascending index, the first one is the head
    for (int i = tid; i < len; i += kScatterWG) {
      const int v = s_tok[i];
      bool seen = v < 0 || v >= a.C;  // (no score above -inf has such a token; it would be an address below)
      for (int q = 0; q < i && !seen; ++q) seen = s_tok[q] == v;
      int nx = -1;
      for (int q = i + 1; q < len && nx < 0; ++q)
        if (s_tok[q] == v) nx = q;
      s_nxt[i] = nx;
      s_head[i] = !seen;
    }
    __syncthreads();
    const GTNX_G float* g = a.alpha + (p - a.pair0) * a.pair_stride;
    for (int item = tid; item < frames * len; item += kScatterWG) {
      const int f = item / len, i = item - f * len;
      if (!s_head[i]) continue;
      const int64_t t = t0 + f;
      const GTNX_G float* gt = g + t * U;
      float sum = gt[i];
      for (int q = s_nxt[i]; q >= 0; q = s_nxt[q]) sum += gt[q];
      GTNX_G float* cell = grad + t * a.C + s_tok[i];
      *cell = *cell + w * sum;
    }
    __syncthreads();  // (the next pair reuses the chains, and reads what this one added)
  }
}

// one wave per table row; `acc` is volatile: the lanes of the wave add into it one after the other
__global__ __launch_bounds__(64) void asg_score_table_kernel(AsgScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_f[];
  volatile float* acc = s_f;  // [C]
  const int lane = static_cast<int>(threadIdx.x);
  const int r = static_cast<int>(blockIdx.x);
  const int C = a.C;
  for (int j = lane; j < C; j += 64) acc[j] = 0.0f;
  wg_sync<64>();
  if (r < C) {
    for (int64_t p = 0; p < a.pairs; ++p) {
      const float w = a.weights[p];
      const float sc = a.scores[p - a.score0];
      const int len = min(max(a.lengths[p], 0), a.L);
      if (w == 0.0f || !(sc > NEG_INF) || len == 0 || len > a.U) continue;  // (uniform: the backward's test)
      const GTNX_G int* tok = a.tokens + p * a.row_stride;
      const GTNX_G float* oc = a.occ + p * 2 * a.occ_half;
      for (int base = 0; base < len; base += 256) {
        int v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = base + u * 64 + lane;
          v[u] = i < len ? tok[i] : -1;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = base + u * 64 + lane;
          const bool mine = v[u] == r;
          unsigned long long mask = __ballot(mine);
          if (mask == 0) continue;  // (uniform)
          float vs = 0.0f, vp = 0.0f;
          int before = -1;
          if (mine) {
            vs = oc[i];
            if (i > 0) {
              before = tok[i - 1];
              vp = oc[a.occ_half + i];
            }
          }
          while (mask) {
            const int l = __ffsll(mask) - 1;
            mask &= mask - 1;
            if (lane == l) {
              acc[r] = acc[r] + vs;
              if (before >= 0 && before < C) acc[before] = acc[before] + vp;
            }
            wg_sync<64>();
          }
        }
      }
    }
  } else {
    for (int64_t base = 0; base < a.pairs; base += 64) {
      const int64_t p = base + lane;
      int y0 = -1;
      float vp = 0.0f;
      if (p < a.pairs) {
        const float w = a.weights[p];
        const float sc = a.scores[p - a.score0];
        const int len = min(max(a.lengths[p], 0), a.L);
        if (!(w == 0.0f || !(sc > NEG_INF) || len == 0 || len > a.U)) {
          y0 = a.tokens[p * a.row_stride];
          vp = a.occ[p * 2 * a.occ_half + a.occ_half];
        }
      }
      const bool mine = y0 >= 0 && y0 < C;
      unsigned long long mask = __ballot(mine);
      while (mask) {
        const int l = __ffsll(mask) - 1;
        mask &= mask - 1;
        if (lane == l) acc[y0] = acc[y0] + vp;
        wg_sync<64>();
      }
    }
  }
  wg_sync<64>();
  GTNX_G float* out = r < C ? a.grad_table + static_cast<int64_t>(C) + static_cast<int64_t>(r) * C : a.grad_table;
  for (int j = lane; j < C; j += 64) out[j] = acc[j];
}

size_t forward_lds(int U) { return sizeof(float) * 2 * size_t(U + 1); }
size_t scatter_lds(int U) { return sizeof(int) * 3 * size_t(U); }

template <int WG, int PER>
void launch_forward(const AsgScoreArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((asg_score_forward_kernel<WG, PER>), dim3(static_cast<unsigned>(a.count)), dim3(WG),
                     forward_lds(a.U), st, a);
}

template <int WG, int PER>
void launch_backward(const AsgScoreArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((asg_score_backward_kernel<WG, PER>), dim3(static_cast<unsigned>(a.count)), dim3(WG),
                     forward_lds(a.U), st, a);
}

}  // namespace

// one wave without barriers while every position has a lane; beyond the widest workgroup a lane owns several positions
void asg_score_config(int U, int* width, int* per_lane) {
  int wg, per;
  if (U <= 64) wg = 64, per = 1;
  else if (U <= 256) wg = 256, per = 1;
  else if (U <= 768) wg = 256, per = 3;
  else if (U <= 1024) wg = 1024, per = 1;
  else if (U <= 2048) wg = 1024, per = 2;
  else wg = 1024, per = 4;
  if (width) *width = wg;
  if (per_lane) *per_lane = per;
}

#define GTNX_ASG_SCORE_DISPATCH(fn)                  \
  int wg, per;                                       \
  asg_score_config(a.U, &wg, &per);                  \
  if (wg == 64) fn<64, 1>(a, st);                    \
  else if (wg == 256 && per == 1) fn<256, 1>(a, st); \
  else if (wg == 256) fn<256, 3>(a, st);             \
  else if (per == 1) fn<1024, 1>(a, st);             \
  else if (per == 2) fn<1024, 2>(a, st);             \
  else fn<1024, 4>(a, st);

void launch_asg_score_forward(const AsgScoreArgs& a, hipStream_t st) {
  if (a.count <= 0) return;
  GTNX_ASG_SCORE_DISPATCH(launch_forward)
}

void launch_asg_score_backward(const AsgScoreArgs& a, hipStream_t st) {
  if (a.count <= 0) return;
  GTNX_ASG_SCORE_DISPATCH(launch_backward)
}

void launch_asg_score_scatter(const AsgScoreArgs& a, hipStream_t st) {
  if (a.count <= 0 || !a.grad || a.M <= 0) return;
  const int64_t b0 = a.pair0 / a.N, b1 = (a.pair0 + a.count - 1) / a.N;
  const unsigned tiles = static_cast<unsigned>((a.M + kScatterFrames - 1) / kScatterFrames);
  hipLaunchKernelGGL(asg_score_scatter_kernel, dim3(static_cast<unsigned>(b1 - b0 + 1), tiles), dim3(kScatterWG),
                     scatter_lds(a.U), st, a);
}

void launch_asg_score_table(const AsgScoreArgs& a, hipStream_t st) {
  if (a.pairs <= 0 || !a.grad_table || !a.occ) return;
  hipLaunchKernelGGL(asg_score_table_kernel, dim3(static_cast<unsigned>(a.C + 1)), dim3(64), sizeof(float) * size_t(a.C),
                     st, a);
}

}  // namespace gtnx
