// ctc_lattice_align.hip -- the best (lattice path, alignment) pair of one device-resident acyclic token lattice per
// utterance: ctc_lattice.hip's forward sweep in the tropical semiring, with back-pointers and a walk (DESIGN section 38
// holds the contract; tests/ctc_lattice_align_fp.py is the same arithmetic in numpy).
//
// The lattice, its states and what makes it invalid are ctc_lattice.hip's: K = num_nodes[b] nodes, A = clamp(num_arcs[b],
// 0, width) dst-sorted arcs (src, dst, label) with 0 <= src < dst < K, state n < K the blank of node n, state K + a the
// token of arc a.
//
//   arithmetic: float32.  A state's candidates come in the forward's order:
//               token a: alpha[a] | alpha[blank src] + w_a | alpha[a'] + w_a for a' in incoming(src) ascending, label(a')
//                        != label(a);   blank n: alpha[n] | alpha[a'] for a' in incoming(n) ascending
//             x is their exact maximum and alpha'[s] = x == -inf ? -inf : x + e(t, label s).  The FIRST candidate that
//             reaches the maximum wins (a later one replaces it only if strictly greater), a -inf candidate is never
//             chosen, a state whose maximum is -inf is dead.  The end: blank(K - 1) | incoming(K - 1) ascending, by the
//             same rule.  Every output is reproducible bit for bit.
//   staging:  ctc_lattice.hip's, copied (sharing it is a later change): every arc field is checked before it becomes an
//             address or an index, nothing at or past num_arcs is read.
//   sweep:    one workgroup per utterance, width and states per lane from ctc_lattice_config(max_states).  The alpha row
//             ping-pongs in LDS with one barrier per frame, the emissions of the next frame are loaded before it.  Per
//             state and frame t >= 1 the lane stores bp[t * SM + s], 16 bits: the SOURCE STATE, 0xFFFF for a dead one --
//             coalesced plain stores into pooled scratch.
//   walk:     wave 0, behind a workgroup barrier (the back-pointers are the other waves' stores), from the end state down
//             through the frames: T_b dependent loads.  Where the state changes it notes the run's first frame and one
//             past its last in LDS (the alpha rows are free by then) and collects the arc, in reverse; lane t % 64 keeps
//             the state of frame t and every 64 frames the wave stores frame_arcs.  A source is clamped to 0 .. K + A - 1
//             and at most K - 1 arcs are collected, so NaN emissions give unspecified values and no access outside the
//             utterance's rows.
//   tokens:   behind a second barrier the lanes stride over the P positions: position i < path_len gets the arc, its
//             label, its span and (if asked) the sum of e(t, label) over the span in ascending order, starting from the
//             first frame's value; the others -1 / -inf.
// Every element of every output row is written over the widths P and M, nothing beyond them.  No path (score -inf,
// path_len 0, fills everywhere): T_b == 0, an invalid or too large lattice, a +inf or NaN weight, an end at -inf.
// Every store is a plain C++ store; there are no atomics on global memory and no inline assembly.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

#include "kernels.h"
#include "pair_kernels.h"

namespace gtnx {
namespace {

constexpr unsigned kDead = 0xFFFFu;  // (a state index is below 4096)

struct Lattice {
  int K, A, S;
};

// Stages utterance b's lattice: s_lab[K + a] the label, s_meta[K + a] = src | dst << 16, s_meta[n] = the first arc
// whose dst is >= n.  True (in every lane, behind a barrier) when the lattice is no valid one.  K + A <= SM is the
// caller's.
template <int WG>
__device__ __forceinline__ bool stage(const CtcLatticeAlignArgs& a, int b, const Lattice& l, int* s_lab, int* s_meta) {
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

// every entry of the utterance's rows from position `i0` and frame `t0` on: what no path covers
template <int WG>
__device__ __forceinline__ void fill_rows(const CtcLatticeAlignArgs& a, int64_t b, int i0, int t0) {
  const int tid = static_cast<int>(threadIdx.x);
  for (int i = i0 + tid; i < a.P; i += WG) {
    const int64_t o = b * a.out_stride + i;
    a.path_arcs[o] = -1;
    a.path_tokens[o] = -1;
    a.starts[o] = -1;
    a.ends[o] = -1;
    if (a.token_scores) a.token_scores[o] = NEG_INF;
  }
  if (a.frame_arcs)
    for (int t = t0 + tid; t < a.M; t += WG) a.frame_arcs[b * a.frame_stride + t] = -1;
}

template <int WG>
__device__ __forceinline__ void no_path(const CtcLatticeAlignArgs& a, int64_t b) {
  if (threadIdx.x == 0) {
    a.scores[b] = NEG_INF;
    a.path_len[b] = 0;
  }
  fill_rows<WG>(a, b, 0, 0);
}

template <int WG, int PER>
__global__ __launch_bounds__(WG) void ctc_lattice_align_kernel(CtcLatticeAlignArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_f[];
  __shared__ float s_score;
  __shared__ int s_end, s_plen;
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
  if (T == 0 || l.K < 1 || l.S > SM) {   // (uniform)
    no_path<WG>(a, b);
    return;
  }
  if (stage<WG>(a, b, l, s_lab, s_meta)) {
    no_path<WG>(a, b);
    return;
  }
  const int K = l.K, S = l.S;
  const GTNX_G float* wts = a.arc_weights ? a.arc_weights + static_cast<int64_t>(b) * a.A : nullptr;
  GTNX_G unsigned short* bp = a.bp + static_cast<int64_t>(blockIdx.x) * a.utt_stride;
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
    GTNX_G unsigned short* bt = bp + static_cast<int64_t>(t) * SM;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int s = tid + j * WG;
      if (s < S) {
        // the first candidate that reaches the maximum: a later one replaces it only if strictly greater
        float x = prev[s];
        int from = s;
        if (s >= K) {
          const float c = plus(prev[node[j]], w[j]);
          if (c > x) x = c, from = node[j];
          for (int q = lo[j]; q < hi[j]; ++q)
            if (s_lab[K + q] != lab[j]) {
              const float d = plus(prev[K + q], w[j]);
              if (d > x) x = d, from = K + q;
            }
        } else {
          for (int q = lo[j]; q < hi[j]; ++q) {
            const float d = prev[K + q];
            if (d > x) x = d, from = K + q;
          }
        }
        const bool dead = x == NEG_INF;
        next[s] = dead ? NEG_INF : x + e[j];
        bt[s] = static_cast<unsigned short>(dead ? kDead : static_cast<unsigned>(from));
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
    int end = K - 1;
    for (int q = q0; q < q1; ++q)
      if (last[K + q] > x) x = last[K + q], end = K + q;
    s_score = x;
    s_end = end;
  }
  wg_sync<WG>();  // (the alpha rows are free from here on; the back-pointers of every wave are stored)
  const float sc = s_score;
  if (!(sc > NEG_INF)) {  // (uniform)
    no_path<WG>(a, b);
    return;
  }
  if (tid == 0) a.scores[b] = sc;
  if (a.frame_arcs)
    for (int t = T + tid; t < a.M; t += WG) a.frame_arcs[static_cast<int64_t>(b) * a.frame_stride + t] = -1;
  int* s_first = reinterpret_cast<int*>(s_f);  // [SM]: state K + a: the first frame of arc a
  int* s_last = s_first + SM;                  // [SM]: ... and one past its last
  int* s_path = s_first;                       // [K - 1]: the arcs from the end down (the blank states' cells)
  if (tid < 64) {
    const int lane = tid;
    GTNX_G int* fa = a.frame_arcs ? a.frame_arcs + static_cast<int64_t>(b) * a.frame_stride : nullptr;
    int s = s_end;
    int top = T;  // one past the last frame of the run of `s`
    int cnt = 0;
    int pn = 0;   // lane t % 64: the state of frame t
    for (int t = T - 1; t >= 0; --t) {
      if (lane == (t & 63)) pn = s;
      int from = s;
      if (t > 0) from = static_cast<int>(min(static_cast<unsigned>(bp[static_cast<int64_t>(t) * SM + s]), static_cast<unsigned>(S - 1)));
      if (from != s || t == 0) {
        if (s >= K) {
          if (lane == 0) {
            s_first[s] = t;
            s_last[s] = top;
            if (cnt < K - 1) s_path[cnt] = s - K;
          }
          if (cnt < K - 1) ++cnt;
        }
        top = t;
      }
      if ((t & 63) == 0 && fa) {  // frames t .. t + 63, one per lane
        const int f = t + lane;
        if (f < T) fa[f] = pn >= K ? pn - K : -1;
      }
      s = from;
    }
    if (lane == 0) s_plen = cnt;
  }
  wg_sync<WG>();
  const int plen = s_plen;
  if (tid == 0) a.path_len[b] = plen;
  for (int i = tid; i < a.P; i += WG) {
    const int64_t o = static_cast<int64_t>(b) * a.out_stride + i;
    int arc = -1, tok = -1, st = -1, en = -1;
    float sum = NEG_INF;
    if (i < plen) {
      arc = s_path[plen - 1 - i];
      tok = s_lab[K + arc];
      st = s_first[K + arc];
      en = s_last[K + arc];
      if (a.token_scores && st >= 0 && en > st && en <= T) {
        const GTNX_G float* col = em + tok;
        sum = col[static_cast<int64_t>(st) * a.C];
        for (int t = st + 1; t < en; ++t) sum += col[static_cast<int64_t>(t) * a.C];
      }
    }
    a.path_arcs[o] = arc;
    a.path_tokens[o] = tok;
    a.starts[o] = st;
    a.ends[o] = en;
    if (a.token_scores) a.token_scores[o] = sum;
  }
}

// the forward kernel's: two alpha rows (the spans and the path behind the sweep), the labels, the arcs' ends
size_t align_lds(int SM) { return sizeof(float) * 4 * size_t(SM); }

template <int WG, int PER>
void launch(const CtcLatticeAlignArgs& a, hipStream_t st) {
  static std::atomic<uint64_t> done{0};
  if (gtnx_first_on_device first{done})
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(ctc_lattice_align_kernel<WG, PER>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, int(align_lds(kCtcLatticeMaxStates)));
  hipLaunchKernelGGL((ctc_lattice_align_kernel<WG, PER>), dim3(static_cast<unsigned>(a.count)), dim3(WG),
                     align_lds(a.SM), st, a);
}

}  // namespace

void launch_ctc_lattice_align(const CtcLatticeAlignArgs& a, hipStream_t st) {
  if (a.count <= 0) return;
  // the width and the states per lane of ctc_lattice_config: six instantiations and no other
  int wg, per;
  ctc_lattice_config(a.SM, &wg, &per);
  if (wg == 64) launch<64, 1>(a, st);
  else if (wg == 256 && per == 1) launch<256, 1>(a, st);
  else if (wg == 256) launch<256, 3>(a, st);
  else if (per == 1) launch<1024, 1>(a, st);
  else if (per == 2) launch<1024, 2>(a, st);
  else launch<1024, 4>(a, st);
}

}  // namespace gtnx
