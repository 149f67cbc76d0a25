// ctc_lattice.hip -- the exact CTC log score of one device-resident acyclic token lattice per utterance, and its
// gradients (DESIGN section 35 holds the contract; tests/ctc_lattice_fp.py has the same recurrences in the same order
// in numpy).  ctc_score.hip with the states of a chain turned into the states of a DAG.
//
// Utterance b has K = num_nodes[b] nodes (0 starts, K - 1 accepts) and A = clamp(num_arcs[b], 0, width) arcs (src, dst,
// label) with 0 <= src < dst < K, sorted by dst, and an optional weight w per arc.  Its states are s = 0 .. K + A - 1:
// state n < K is the blank of node n, state K + a the token of arc a.  Both kinds loop; blank(src a) -> token(a),
// token(a) -> blank(dst a), and token(a') -> token(a) when dst a' == src a and the labels differ; w_a is paid on every
// transition that enters token(a) from another state.  score = log sum over every path and alignment, nothing subtracted.
//
//   staging:  the arcs are read once: label, (src | dst << 16) and the first incoming arc of every node (the arcs are
//             dst-sorted, so incoming(n) is the run lo[n] .. lo[n + 1]) go to LDS.  Every field is checked before it
//             becomes an address or an index: src < 0, src >= dst, dst >= K, a dst below the one before, a label outside
//             0 .. C - 1, a weight that is +inf or NaN each make the utterance score -inf.  Nothing at or past num_arcs is
//             read.
//   forward:  one workgroup per utterance.  A lane owns the states tid, tid + WG, ... (PER of them), the alpha row
//             ping-pongs in LDS with one barrier per frame, the emissions of the next frame are loaded before it.
//               token a: x = logadd(alpha[a], alpha[blank src] + w_a); for a' in incoming(src) ascending, label(a') !=
//                        label(a): x = logadd(x, alpha[a'] + w_a); alpha'[a] = x == -inf ? -inf : x + e(t, label a)
//               blank n: x = alpha[n]; for a' in incoming(n) ascending: x = logadd(x, alpha[a']); then + e(t, blank)
//             score = logadd over blank(K - 1), then incoming(K - 1) ascending.  With a.alpha non-null every row is also
//             stored (the backward's recomputation).
//   backward: one workgroup per utterance.  The arcs leaving a node are chained once (ascending arc index, found by
//             scanning the arcs whose dst is above the node), and so are the arcs of equal label.  beta runs from the
//             last frame down in LDS: m[s] = beta[s] + e(t, label s) (a token's cell holds w_a + m, which is what every
//             other state wants of it; its own m stays in a register),
//               token a: x = logadd(m[a], m[blank dst]); for a'' leaving dst ascending, label differs: x = logadd(x, m[a''])
//               blank n: x = m[n]; for a'' leaving n ascending: x = logadd(x, m[a''])
//             The occupancies exp(alpha + beta - score) of a frame are summed per label in ONE order: the blank states
//             by lane (ascending state), the xor tree of the wave, the waves ascending; a label's tokens along its
//             chain, ascending arc index, the blanks' sum in front when the label is `blank`; the lane that owns the
//             chain's head stores g * sum.  The arc-weight gradient is the sum over frames, descending, of exp(enter_t(a)
//             + m_t[a] - score) with enter_t(a) = logadd(alpha_{t-1}[blank src] + w_a, alpha_{t-1}[a'] + w_a ...) in the
//             forward's order (w_a alone at frame 0 for src == 0), kept in a register and stored once.  The workgroup
//             zeroes the utterance's slab and its arc-gradient row first.
// The width WG and PER come from max_states alone (ctc_lattice_config), so a cut into slices changes no order of sums.
// Every store is a plain C++ store; there are no floating-point atomics and no inline assembly.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

#include "kernels.h"
#include "pair_kernels.h"

namespace gtnx {
namespace {

constexpr unsigned kNone = 0xFFFFu;  // the end of a chain (an arc index is below 4096)

struct Lattice {
  int K, A, S;
};

// Stages utterance b's lattice: s_lab[K + a] the label, s_meta[K + a] = src | dst << 16, s_meta[n] = the first arc
// whose dst is >= n.  True (in every lane, behind a barrier) when the lattice is no valid one.  K + A <= SM is the
// caller's.
template <int WG>
__device__ __forceinline__ bool stage(const CtcLatticeArgs& a, int b, const Lattice& l, int* s_lab, int* s_meta) {
  const int tid = static_cast<int>(threadIdx.x);
  const GTNX_G int* arcs = a.arcs + static_cast<int64_t>(b) * a.row_stride;
  const GTNX_G float* wts = a.arc_weights ? a.arc_weights + static_cast<int64_t>(b) * a.A : nullptr;
  const int K = l.K, A = l.A;
  int bad = 0;
  // (i == A: the nodes above the last arc's dst have no incoming arc)
  for (int i = tid; i <= A; i += WG) {
    const int before = i > 0 ? arcs[3 * static_cast<int64_t>(i - 1) + 1] : -1;
    int dst = K - 1;
    if (i < A) {
      const int src = arcs[3 * static_cast<int64_t>(i)];
      dst = arcs[3 * static_cast<int64_t>(i) + 1];
      const int lab = arcs[3 * static_cast<int64_t>(i) + 2];
      const float w = wts ? wts[i] : 0.0f;
      const bool ok = src >= 0 && src < dst && dst < K && before <= dst && lab >= 0 && lab < a.C && w < __builtin_inff();
      if (!ok) {
        bad = 1;
        continue;
      }
      s_lab[K + i] = lab;
      s_meta[K + i] = src | (dst << 16);
    }
    // (dst < K here; a `before` that is no node is refused by its own lane)
    for (int n = max(before, -1) + 1; n <= dst; ++n) s_meta[n] = i;
  }
  return wg_any<WG>(bad);
}

// the run of arcs that enter node n
__device__ __forceinline__ void incoming(const int* s_meta, const Lattice& l, int n, int& lo, int& hi) {
  lo = s_meta[n];
  hi = n + 1 < l.K ? s_meta[n + 1] : l.A;
}

__device__ __forceinline__ float plus(float x, float w) { return x == NEG_INF || w == NEG_INF ? NEG_INF : x + w; }

template <int WG, int PER>
__global__ __launch_bounds__(WG) void ctc_lattice_forward_kernel(CtcLatticeArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_f[];
  const int SM = a.SM;
  float* s_alpha = s_f;                                   // [2][SM]
  int* s_lab = reinterpret_cast<int*>(s_alpha + 2 * SM);  // [SM]
  int* s_meta = s_lab + SM;                               // [SM]
  const int tid = static_cast<int>(threadIdx.x);
  const int b = a.utt0 + static_cast<int>(blockIdx.x);
  const int T = min(max(a.frames[b], 0), a.M);
  Lattice l;
  l.K = a.num_nodes[b];
  l.A = min(max(a.num_arcs[b], 0), a.A);
  l.S = l.K <= SM ? l.K + l.A : SM + 1;  // (a node count that is no count must not overflow the sum)
  GTNX_G float* out = a.scores + (b - a.score0);
  if (T == 0 || l.K < 1 || l.S > SM) {  // (uniform)
    if (tid == 0) *out = NEG_INF;
    return;
  }
  if (stage<WG>(a, b, l, s_lab, s_meta)) {
    if (tid == 0) *out = NEG_INF;
    return;
  }
  const int K = l.K, S = l.S;
  const GTNX_G float* wts = a.arc_weights ? a.arc_weights + static_cast<int64_t>(b) * a.A : nullptr;
  GTNX_G float* keep = a.alpha ? a.alpha + static_cast<int64_t>(blockIdx.x) * a.utt_stride : nullptr;
  const GTNX_G float* em = a.em + static_cast<int64_t>(b) * a.M * a.C;
  // what a lane keeps of its states: the label, the node whose incoming arcs enter it, their run, the arc's weight
  int lab[PER], node[PER], lo[PER], hi[PER];
  float w[PER], e[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int s = tid + j * WG;
    lab[j] = a.blank;
    node[j] = 0;
    lo[j] = hi[j] = 0;
    w[j] = 0.0f;
    e[j] = NEG_INF;
    if (s < S) {
      if (s >= K) {
        lab[j] = s_lab[s];
        node[j] = s_meta[s] & 0xFFFF;
        w[j] = wts ? wts[s - K] : 0.0f;
      } else {
        node[j] = s;
      }
      incoming(s_meta, l, node[j], lo[j], hi[j]);
      e[j] = em[lab[j]];
    }
  }
  int cur = 0;
  // frame 0: the start node's blank and the arcs that leave it
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int s = tid + j * WG;
    if (s < S) {
      float v = NEG_INF;
      if (s == 0) v = e[j];
      else if (s >= K && node[j] == 0) v = plus(e[j], w[j]);
      s_alpha[s] = v;
      if (keep) keep[s] = v;
    }
  }
  for (int t = 1; t < T; ++t) {
    const GTNX_G float* row = em + static_cast<int64_t>(t) * a.C;
#pragma unroll
    for (int j = 0; j < PER; ++j)
      if (tid + j * WG < S) e[j] = row[lab[j]];
    wg_sync<WG>();
    const float* prev = s_alpha + cur * SM;
    float* next = s_alpha + (cur ^ 1) * SM;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int s = tid + j * WG;
      if (s < S) {
        float x = prev[s];
        if (s >= K) {
          x = logadd(x, plus(prev[node[j]], w[j]));
          for (int q = lo[j]; q < hi[j]; ++q)
            if (s_lab[K + q] != lab[j]) x = logadd(x, plus(prev[K + q], w[j]));
        } else {
          for (int q = lo[j]; q < hi[j]; ++q) x = logadd(x, prev[K + q]);
        }
        const float v = x == NEG_INF ? NEG_INF : x + e[j];
        next[s] = v;
        if (keep) keep[static_cast<int64_t>(t) * SM + s] = v;
      }
    }
    cur ^= 1;
  }
  wg_sync<WG>();
  if (tid == 0) {
    const float* last = s_alpha + cur * SM;
    int q0, q1;
    incoming(s_meta, l, K - 1, q0, q1);
    float x = last[K - 1];
    for (int q = q0; q < q1; ++q) x = logadd(x, last[K + q]);
    *out = x;
  }
}

template <int WG, int PER>
__global__ __launch_bounds__(WG) void ctc_lattice_backward_kernel(CtcLatticeArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_f[];
  constexpr int NW = WG / 64;
  const int SM = a.SM;
  float* s_m = s_f;                                        // [2][SM]: beta + e; a token's cell has its weight on top
  float* s_g = s_m + 2 * SM;                               // [2][SM]: the occupancies of the token states
  float* s_al = s_g + 2 * SM;                              // [2][SM]: the alpha row of the frame before
  float* s_part = s_al + 2 * SM;                           // [2][16]: the waves' sums over the blank states
  int* s_lab = reinterpret_cast<int*>(s_part + 32);        // [SM]
  int* s_meta = s_lab + SM;                                // [SM]
  unsigned* s_ch = reinterpret_cast<unsigned*>(s_meta + SM);  // [SM]: node n: its first leaving arc; arc a: the next
                                                              // arc of its label | the next arc of its src << 16
  int* s_flag = reinterpret_cast<int*>(s_ch + SM);         // [1]: a chain's head carries `blank`
  const int tid = static_cast<int>(threadIdx.x);
  const int lane = tid & 63, wave = tid >> 6;
  const int b = a.utt0 + static_cast<int>(blockIdx.x);
  const int T = min(max(a.frames[b], 0), a.M);
  const int64_t slab = static_cast<int64_t>(a.M) * a.C;
  GTNX_G float* grad = a.grad + static_cast<int64_t>(b) * slab;
  GTNX_G float* garc = a.arc_grad ? a.arc_grad + static_cast<int64_t>(b) * a.A : nullptr;
  const GTNX_G float* em = a.em + static_cast<int64_t>(b) * slab;
  for (int64_t i = tid; i < slab; i += WG) grad[i] = 0.0f;
  if (garc)
    for (int i = tid; i < a.A; i += WG) garc[i] = 0.0f;
  const float gw = a.weights[b];
  const float sc = a.scores[b - a.score0];
  Lattice l;
  l.K = a.num_nodes[b];
  l.A = min(max(a.num_arcs[b], 0), a.A);
  l.S = l.K <= SM ? l.K + l.A : SM + 1;
  // (uniform; a score above -inf says there is a path: T > 0 and a valid lattice within SM -- and NaN is no score)
  if (gw == 0.0f || !(sc > NEG_INF) || T == 0 || l.K < 1 || l.S > SM) return;
  const int K = l.K, A = l.A, S = l.S;
  for (int n = tid; n < K; n += WG) s_ch[n] = kNone;
  if (tid == 0) *s_flag = 0;
  if (stage<WG>(a, b, l, s_lab, s_meta)) return;  // (uniform; it is also the barrier behind the zeroes and s_ch)
  const GTNX_G float* wts = a.arc_weights ? a.arc_weights + static_cast<int64_t>(b) * a.A : nullptr;
  int lab[PER];
  float w[PER];
  bool head[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int s = tid + j * WG;
    lab[j] = a.blank;
    w[j] = 0.0f;
    head[j] = false;
    if (s < S && s >= K) {
      const int i = s - K, v = s_lab[s], src = s_meta[s] & 0xFFFF;
      lab[j] = v;
      w[j] = wts ? wts[i] : 0.0f;
      // the chain of its label: ascending arc index, the first one is the head
      bool seen = false;
      for (int q = 0; q < i && !seen; ++q) seen = s_lab[K + q] == v;
      unsigned nl = kNone;
      for (int q = i + 1; q < A && nl == kNone; ++q)
        if (s_lab[K + q] == v) nl = static_cast<unsigned>(q);
      // the chain of its src: an arc that leaves src enters a node above it, so it lies at or behind lo[src + 1]
      bool first = true;
      for (int q = src + 1 < K ? s_meta[src + 1] : A; q < i && first; ++q) first = (s_meta[K + q] & 0xFFFF) != src;
      unsigned no = kNone;
      for (int q = i + 1; q < A && no == kNone; ++q)
        if ((s_meta[K + q] & 0xFFFF) == src) no = static_cast<unsigned>(q);
      s_ch[s] = nl | (no << 16);
      if (first) s_ch[src] = static_cast<unsigned>(i);
      head[j] = !seen;
      if (!seen && v == a.blank) *s_flag = 1;
    }
  }
  const GTNX_G float* al = a.alpha + static_cast<int64_t>(blockIdx.x) * a.utt_stride;
  float beta[PER], av[PER], e[PER], wacc[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int s = tid + j * WG;
    beta[j] = av[j] = e[j] = NEG_INF;
    wacc[j] = 0.0f;
    if (s < S) {
      const int end = s >= K ? s_meta[s] >> 16 : s;  // the node behind the state
      if (end == K - 1) beta[j] = 0.0f;
      av[j] = al[static_cast<int64_t>(T - 1) * SM + s];
      e[j] = em[static_cast<int64_t>(T - 1) * a.C + lab[j]];
    }
  }
  wg_sync<WG>();  // (the chains and the flag)
  const bool blank_in_chain = *s_flag != 0;
  int pp = 0;
  for (int t = T - 1; t >= 0; --t) {
    float* m = s_m + pp * SM;
    float* g = s_g + pp * SM;
    float* ap = s_al + pp * SM;
    float* part = s_part + pp * 16;
    GTNX_G float* row = grad + static_cast<int64_t>(t) * a.C;
    float ev = 0.0f, mo[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int s = tid + j * WG;
      mo[j] = NEG_INF;
      if (s < S) {
        const float x = av[j] > NEG_INF && beta[j] > NEG_INF ? expf(av[j] + beta[j] - sc) : 0.0f;
        mo[j] = beta[j] == NEG_INF ? NEG_INF : beta[j] + e[j];
        if (s >= K) {
          m[s] = plus(mo[j], w[j]);
          g[s] = x;
        } else {
          m[s] = mo[j];
          ev += x;
        }
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
          e[j] = em[static_cast<int64_t>(t - 1) * a.C + lab[j]];
          if (garc) ap[s] = av[j];
        }
      }
    }
    wg_sync<WG>();
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int s = tid + j * WG;
      if (s < S) {
        float x = mo[j];
        if (s >= K) {
          const int src = s_meta[s] & 0xFFFF, dst = s_meta[s] >> 16;
          x = logadd(x, m[dst]);
          for (unsigned q = s_ch[dst]; q != kNone; q = s_ch[K + q] >> 16)
            if (s_lab[K + q] != lab[j]) x = logadd(x, m[K + q]);
          if (garc) {
            // how the frame enters the arc: the forward's order over the frame before
            float ent = NEG_INF;
            if (t == 0) {
              if (src == 0) ent = w[j];
            } else {
              int q0, q1;
              incoming(s_meta, l, src, q0, q1);
              ent = plus(ap[src], w[j]);
              for (int q = q0; q < q1; ++q)
                if (s_lab[K + q] != lab[j]) ent = logadd(ent, plus(ap[K + q], w[j]));
            }
            if (ent > NEG_INF && mo[j] > NEG_INF) wacc[j] += expf(ent + mo[j] - sc);
          }
          if (head[j]) {
            float sum = g[s];
            if (lab[j] == a.blank) {
              float evs = part[0];
              for (int q = 1; q < NW; ++q) evs += part[q];
              sum = evs + sum;
            }
            for (unsigned q = s_ch[s] & 0xFFFF; q != kNone; q = s_ch[K + q] & 0xFFFF) sum += g[K + q];
            row[lab[j]] = gw * sum;
          }
        } else {
          for (unsigned q = s_ch[s]; q != kNone; q = s_ch[K + q] >> 16) x = logadd(x, m[K + q]);
        }
        beta[j] = x;
      }
    }
    if (tid == 0 && !blank_in_chain) {
      float evs = part[0];
      for (int q = 1; q < NW; ++q) evs += part[q];
      row[a.blank] = gw * evs;
    }
    pp ^= 1;
  }
  if (garc) {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int s = tid + j * WG;
      if (s < S && s >= K) garc[s - K] = gw * wacc[j];
    }
  }
}

size_t forward_lds(int SM) { return sizeof(float) * 4 * size_t(SM); }
size_t backward_lds(int SM) { return sizeof(float) * (9 * size_t(SM) + 32 + 4); }

template <int WG, int PER>
void launch_forward(const CtcLatticeArgs& a, hipStream_t st) {
  static std::atomic<uint64_t> done{0};
  if (gtnx_first_on_device first{done})
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(ctc_lattice_forward_kernel<WG, PER>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, int(forward_lds(kCtcLatticeMaxStates)));
  hipLaunchKernelGGL((ctc_lattice_forward_kernel<WG, PER>), dim3(static_cast<unsigned>(a.count)), dim3(WG),
                     forward_lds(a.SM), st, a);
}

template <int WG, int PER>
void launch_backward(const CtcLatticeArgs& a, hipStream_t st) {
  static std::atomic<uint64_t> done{0};
  if (gtnx_first_on_device first{done})
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(ctc_lattice_backward_kernel<WG, PER>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, int(backward_lds(kCtcLatticeMaxStates)));
  hipLaunchKernelGGL((ctc_lattice_backward_kernel<WG, PER>), dim3(static_cast<unsigned>(a.count)), dim3(WG),
                     backward_lds(a.SM), st, a);
}

// fn<WG, PER>(...) with the width and the states per lane of ctc_lattice_config: six instantiations and no other
#define GTNX_CTC_LATTICE_DISPATCH(SM, fn, ...)               \
  do {                                                       \
    int wg, per;                                             \
    ctc_lattice_config(SM, &wg, &per);                       \
    if (wg == 64) fn<64, 1>(__VA_ARGS__);                    \
    else if (wg == 256 && per == 1) fn<256, 1>(__VA_ARGS__); \
    else if (wg == 256) fn<256, 3>(__VA_ARGS__);             \
    else if (per == 1) fn<1024, 1>(__VA_ARGS__);             \
    else if (per == 2) fn<1024, 2>(__VA_ARGS__);             \
    else fn<1024, 4>(__VA_ARGS__);                           \
  } while (0)

}  // namespace

// one wave without barriers while every state has a lane; beyond the widest workgroup a lane owns several states
void ctc_lattice_config(int max_states, int* width, int* per_lane) {
  int wg, per;
  if (max_states <= 64) wg = 64, per = 1;
  else if (max_states <= 256) wg = 256, per = 1;
  else if (max_states <= 768) wg = 256, per = 3;
  else if (max_states <= 1024) wg = 1024, per = 1;
  else if (max_states <= 2048) wg = 1024, per = 2;
  else wg = 1024, per = 4;
  if (width) *width = wg;
  if (per_lane) *per_lane = per;
}

void launch_ctc_lattice_forward(const CtcLatticeArgs& a, hipStream_t st) {
  if (a.count <= 0) return;
  GTNX_CTC_LATTICE_DISPATCH(a.SM, launch_forward, a, st);
}

void launch_ctc_lattice_backward(const CtcLatticeArgs& a, hipStream_t st) {
  if (a.count <= 0) return;
  GTNX_CTC_LATTICE_DISPATCH(a.SM, launch_backward, a, st);
}

}  // namespace gtnx
