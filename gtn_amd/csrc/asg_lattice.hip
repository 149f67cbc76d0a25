// asg_lattice.hip -- the exact ASG log score of one device-resident acyclic token lattice per utterance, and its
// gradients with respect to the emissions, the [C + C * C] table of start and transition scores and the arc weights
// (DESIGN section 37 holds the contract; tests/asg_lattice_fp.py has the same recurrences in the same order in numpy).
// ctc_lattice.hip without the blank states, with asg_score.hip's table on every edge.
//
// Utterance b has K = num_nodes[b] nodes (0 starts, K - 1 accepts) and A = clamp(num_arcs[b], 0, width) arcs (src, dst,
// label) with 0 <= src < dst < K, sorted by dst, and an optional weight w per arc.  Its states are the arcs.  Arc a loops
// with table[C + lab a * C + lab a]; an EDGE (a' -> a), dst a' == src a, pays w_a + table[C + lab a * C + lab a'] (equal
// labels are legal); an arc that leaves node 0 is entered at frame 0 with w_a + table[lab a].  The edges are numbered
// CSR-wise: arc a's incoming edges are off[a] .. off[a] + indegree(src a), off the prefix sum over the arcs.
//
//   staging:  ctc_lattice.hip's: every arc field is checked before it becomes an address or an index, nothing at or
//             past num_arcs is read.  On top: E = sum over the arcs of indegree(src a) by a workgroup scan; E above
//             max_edges scores -inf (the backward's edge rows have max_edges cells per utterance).
//   forward:  one workgroup per utterance.  A lane owns the arcs tid, tid + WG, ... (PER of them; label, weight, self
//             weight and the base of its table row in registers), the alpha row ping-pongs in LDS with one barrier per
//             frame, the emissions of the next frame are loaded before it.
//               x = alpha[a] + w_self; for a' in incoming(src a) ascending: x = logadd(x, alpha[a'] + (w_a + table[row a
//               + lab a'])); alpha'[a] = x + e(t, lab a)
//             The edge weights are gathered from the table every frame (L2 hits; a cache of E floats fits neither
//             registers nor LDS at the caps).  score = logadd over incoming(K - 1) ascending.  With a.alpha non-null
//             every row is also stored (the backward's recomputation), else nothing but the score is.
//   backward: one workgroup per utterance.  beta runs from the last frame down in LDS: m[a] = beta[a] + e(t, lab a) (the
//             LDS cell holds w_a + m[a], which is what every arc in front of it wants),
//               beta'[a] = logadd(m[a] + w_self, for a'' leaving dst a ascending: cell[a''] + table[row a'' + lab a])
//             The emission gradient of a frame is summed per label along the chain of arcs of equal label, ascending arc
//             index; the lane that owns the chain's head stores g * sum.  An arc keeps the sum over the frames (last
//             frame first) of its self occupancy exp(alpha_{t-1}[a] + w_self + m_t[a] - score) and its start term in
//             registers; the occupancy of edge (a' -> a), exp(alpha_{t-1}[a'] + (w_a + table) + m_t[a] - score), is added
//             to the edge's own cell of the utterance's edge row by the lane that owns a (plain load and store).  The
//             arc-weight gradient is g * (start term + the arc's cells ascending).
//   table:    one launch per slice behind its backward.  Workgroup r < C (one wave) owns table[C + r * C ..], workgroup C
//             the start entries.  It walks the slice's utterances in b order and the arcs ascending; for an arc of label
//             r its self sum goes into [r], then its edges ascending into [lab a'], one value at a time (lane 0 adds; the
//             wave only loads).  The first slice starts the row from zeros, a later one from what the row holds, so the
//             chain of additions is the same however the utterances are cut.  The row is stored whole.
// The width WG and PER come from max_states alone (asg_lattice_config), so a cut into slices changes no order of sums.
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
__device__ __forceinline__ bool stage(const AsgLatticeArgs& a, int b, const Lattice& l, int* s_lab, int* s_meta) {
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

// E = the sum over the arcs of indegree(src a), in every lane, behind a barrier; with s_off non-null s_off[a] = the sum
// over the arcs below a.  For the scan alone a lane takes the PER arcs tid * PER .. (s_red: one int per wave)
template <int WG, int PER>
__device__ __forceinline__ int edge_scan(const int* s_meta, const Lattice& l, int* s_off, int* s_red) {
  constexpr int NW = WG / 64;
  const int tid = static_cast<int>(threadIdx.x);
  const int lane = tid & 63, wave = tid >> 6;
  int deg[PER], sum = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = tid * PER + j;
    deg[j] = 0;
    if (i < l.A) {
      int lo, hi;
      incoming(s_meta, l, s_meta[l.K + i] & 0xFFFF, lo, hi);
      deg[j] = hi - lo;
    }
    sum += deg[j];
  }
  int inc = sum;
  for (int d = 1; d < 64; d <<= 1) {
    const int v = __shfl_up(inc, d);
    if (lane >= d) inc += v;
  }
  if (lane == 63) s_red[wave] = inc;
  wg_sync<WG>();
  int below = 0, total = 0;
  for (int q = 0; q < NW; ++q) {
    const int v = s_red[q];
    if (q < wave) below += v;
    total += v;
  }
  if (s_off) {
    int run = below + inc - sum;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int i = tid * PER + j;
      if (i < l.A) s_off[i] = run;
      run += deg[j];
    }
  }
  wg_sync<WG>();
  return total;
}

template <int WG, int PER>
__global__ __launch_bounds__(WG) void asg_lattice_forward_kernel(AsgLatticeArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_f[];
  const int SM = a.SM;
  float* s_alpha = s_f;                                   // [2][SM], by arc
  int* s_lab = reinterpret_cast<int*>(s_alpha + 2 * SM);  // [SM]
  int* s_meta = s_lab + SM;                               // [SM]
  int* s_red = s_meta + SM;                               // [16]
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
  if (edge_scan<WG, PER>(s_meta, l, nullptr, s_red) > a.max_edges) {  // (uniform)
    if (tid == 0) *out = NEG_INF;
    return;
  }
  const int K = l.K, A = l.A;
  const GTNX_G float* wts = a.arc_weights ? a.arc_weights + static_cast<int64_t>(b) * a.A : nullptr;
  GTNX_G float* keep = a.alpha ? a.alpha + static_cast<int64_t>(blockIdx.x) * a.utt_stride : nullptr;
  const GTNX_G float* em = a.em + static_cast<int64_t>(b) * a.M * a.C;
  // what a lane keeps of its arcs: the label, the run of arcs entering its src, the weight, the self weight and its row
  int lab[PER], lo[PER], hi[PER];
  bool first[PER];
  float w[PER], wself[PER], e[PER];
  const GTNX_G float* trow[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = tid + j * WG;
    lab[j] = 0;
    lo[j] = hi[j] = 0;
    first[j] = false;
    w[j] = 0.0f;
    wself[j] = e[j] = NEG_INF;
    trow[j] = a.table;
    if (i < A) {
      const int src = s_meta[K + i] & 0xFFFF;
      lab[j] = s_lab[K + i];
      first[j] = src == 0;
      incoming(s_meta, l, src, lo[j], hi[j]);
      w[j] = wts ? wts[i] : 0.0f;
      trow[j] = a.table + (static_cast<int64_t>(a.C) + static_cast<int64_t>(lab[j]) * a.C);
      wself[j] = trow[j][lab[j]];
      e[j] = em[lab[j]];
    }
  }
  int cur = 0;
  // frame 0: the arcs that leave the start node
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = tid + j * WG;
    if (i < A) {
      const float v = first[j] ? (w[j] + a.table[lab[j]]) + e[j] : NEG_INF;
      s_alpha[i] = v;
      if (keep) keep[i] = v;
    }
  }
  for (int t = 1; t < T; ++t) {
    const GTNX_G float* row = em + static_cast<int64_t>(t) * a.C;
#pragma unroll
    for (int j = 0; j < PER; ++j)
      if (tid + j * WG < A) e[j] = row[lab[j]];
    wg_sync<WG>();
    const float* prev = s_alpha + cur * SM;
    float* next = s_alpha + (cur ^ 1) * SM;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int i = tid + j * WG;
      if (i < A) {
        float x = prev[i] + wself[j];
        for (int q = lo[j]; q < hi[j]; ++q) x = logadd(x, prev[q] + (w[j] + trow[j][s_lab[K + q]]));
        const float v = x + e[j];
        next[i] = v;
        if (keep) keep[static_cast<int64_t>(t) * SM + i] = v;
      }
    }
    cur ^= 1;
  }
  wg_sync<WG>();
  if (tid == 0) {
    const float* last = s_alpha + cur * SM;
    int q0, q1;
    incoming(s_meta, l, K - 1, q0, q1);
    float x = NEG_INF;
    for (int q = q0; q < q1; ++q) x = logadd(x, last[q]);
    *out = x;
  }
}

template <int WG, int PER>
__global__ __launch_bounds__(WG) void asg_lattice_backward_kernel(AsgLatticeArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_f[];
  const int SM = a.SM;
  float* s_m = s_f;                                        // [2][SM]: w_a + beta + e, by arc
  float* s_g = s_m + 2 * SM;                               // [2][SM]: the occupancies of the arcs
  float* s_al = s_g + 2 * SM;                              // [2][SM]: the alpha row of the frame before
  int* s_lab = reinterpret_cast<int*>(s_al + 2 * SM);      // [SM]
  int* s_meta = s_lab + SM;                                // [SM]
  unsigned* s_ch = reinterpret_cast<unsigned*>(s_meta + SM);  // [SM]: node n: its first leaving arc; arc a: the next
                                                              // arc of its label | the next arc of its src << 16
  int* s_red = reinterpret_cast<int*>(s_ch + SM);          // [16]
  int* s_off = reinterpret_cast<int*>(s_g);                // [SM]: the arcs' edge offsets, until the frames begin
  const int tid = static_cast<int>(threadIdx.x);
  const int b = a.utt0 + static_cast<int>(blockIdx.x);
  const int T = min(max(a.frames[b], 0), a.M);
  const int64_t slab = static_cast<int64_t>(a.M) * a.C;
  GTNX_G float* grad = a.grad ? a.grad + static_cast<int64_t>(b) * slab : nullptr;
  GTNX_G float* garc = a.arc_grad ? a.arc_grad + static_cast<int64_t>(b) * a.A : nullptr;
  const GTNX_G float* em = a.em + static_cast<int64_t>(b) * slab;
  if (grad)
    for (int64_t i = tid; i < slab; i += WG) grad[i] = 0.0f;
  if (garc)
    for (int i = tid; i < a.A; i += WG) garc[i] = 0.0f;
  const float gw = a.weights[b];
  const float sc = a.scores[b - a.score0];
  Lattice l;
  l.K = a.num_nodes[b];
  l.A = min(max(a.num_arcs[b], 0), a.A);
  l.S = l.K <= SM ? l.K + l.A : SM + 1;
  // (uniform; a score above -inf says there is a path: T > 0, a valid lattice within SM and max_edges -- NaN is no score)
  if (gw == 0.0f || !(sc > NEG_INF) || T == 0 || l.K < 1 || l.S > SM) return;
  const int K = l.K, A = l.A;
  for (int n = tid; n < K; n += WG) s_ch[n] = kNone;
  if (stage<WG>(a, b, l, s_lab, s_meta)) return;  // (uniform; it is also the barrier behind the zeroes and s_ch)
  if (edge_scan<WG, PER>(s_meta, l, s_off, s_red) > a.max_edges) return;  // (uniform)
  const GTNX_G float* wts = a.arc_weights ? a.arc_weights + static_cast<int64_t>(b) * a.A : nullptr;
  GTNX_G float* edge = a.edge ? a.edge + static_cast<int64_t>(blockIdx.x) * a.max_edges : nullptr;
  int lab[PER], lo[PER], hi[PER], off[PER], dst[PER];
  float w[PER], wself[PER], wstart[PER];
  bool head[PER];
  const GTNX_G float* trow[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = tid + j * WG;
    lab[j] = 0;
    lo[j] = hi[j] = off[j] = dst[j] = 0;
    w[j] = 0.0f;
    wself[j] = wstart[j] = NEG_INF;
    head[j] = false;
    trow[j] = a.table;
    if (i < A) {
      const int v = s_lab[K + i], src = s_meta[K + i] & 0xFFFF;
      lab[j] = v;
      dst[j] = s_meta[K + i] >> 16;
      off[j] = s_off[i];
      incoming(s_meta, l, src, lo[j], hi[j]);
      w[j] = wts ? wts[i] : 0.0f;
      trow[j] = a.table + (static_cast<int64_t>(a.C) + static_cast<int64_t>(v) * a.C);
      wself[j] = trow[j][v];
      if (src == 0) wstart[j] = w[j] + a.table[v];
      // the chain of its label: ascending arc index, the first one is the head
      bool seen = false;
      for (int q = 0; q < i && !seen; ++q) seen = s_lab[K + q] == v;
      unsigned nl = kNone;
      for (int q = i + 1; q < A && nl == kNone; ++q)
        if (s_lab[K + q] == v) nl = static_cast<unsigned>(q);
      // the chain of its src: an arc that leaves src enters a node above it, so it lies at or behind lo[src + 1]
      bool firstout = true;
      for (int q = src + 1 < K ? s_meta[src + 1] : A; q < i && firstout; ++q) firstout = (s_meta[K + q] & 0xFFFF) != src;
      unsigned no = kNone;
      for (int q = i + 1; q < A && no == kNone; ++q)
        if ((s_meta[K + q] & 0xFFFF) == src) no = static_cast<unsigned>(q);
      s_ch[K + i] = nl | (no << 16);
      if (firstout) s_ch[src] = static_cast<unsigned>(i);
      head[j] = !seen;
      if (edge)
        for (int k = 0; k < hi[j] - lo[j]; ++k) edge[off[j] + k] = 0.0f;
    }
  }
  const GTNX_G float* al = a.alpha + static_cast<int64_t>(blockIdx.x) * a.utt_stride;
  float beta[PER], av[PER], e[PER], sum_self[PER], sum_start[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = tid + j * WG;
    beta[j] = av[j] = e[j] = NEG_INF;
    sum_self[j] = sum_start[j] = 0.0f;
    if (i < A) {
      if (dst[j] == K - 1) beta[j] = 0.0f;
      av[j] = al[static_cast<int64_t>(T - 1) * SM + i];
      e[j] = em[static_cast<int64_t>(T - 1) * a.C + lab[j]];
    }
  }
  wg_sync<WG>();  // (the chains; s_off is read, its cells become s_g)
  int pp = 0;
  for (int t = T - 1; t >= 0; --t) {
    float* m = s_m + pp * SM;
    float* g = s_g + pp * SM;
    float* ap = s_al + pp * SM;
    float mo[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int i = tid + j * WG;
      mo[j] = NEG_INF;
      if (i < A) {
        g[i] = av[j] > NEG_INF && beta[j] > NEG_INF ? expf(av[j] + beta[j] - sc) : 0.0f;
        mo[j] = beta[j] + e[j];
        m[i] = mo[j] + w[j];
      }
    }
    if (t > 0) {
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        const int i = tid + j * WG;
        if (i < A) {
          av[j] = al[static_cast<int64_t>(t - 1) * SM + i];
          e[j] = em[static_cast<int64_t>(t - 1) * a.C + lab[j]];
          ap[i] = av[j];
        }
      }
    }
    wg_sync<WG>();
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int i = tid + j * WG;
      if (i < A) {
        // the frame's occupancies of the ways into the arc
        if (mo[j] > NEG_INF) {
          if (t == 0) {
            const float xs = wstart[j] + mo[j];
            if (xs > NEG_INF) sum_start[j] += expf(xs - sc);
          } else {
            const float xs = (av[j] + wself[j]) + mo[j];
            if (xs > NEG_INF) sum_self[j] += expf(xs - sc);
            if (edge) {
              for (int q = lo[j]; q < hi[j]; ++q) {
                const float xe = (ap[q] + (w[j] + trow[j][s_lab[K + q]])) + mo[j];
                if (xe > NEG_INF) {
                  GTNX_G float* cell = edge + off[j] + (q - lo[j]);
                  *cell = *cell + expf(xe - sc);
                }
              }
            }
          }
        }
        if (grad && head[j]) {
          float sum = g[i];
          for (unsigned q = s_ch[K + i] & 0xFFFF; q != kNone; q = s_ch[K + q] & 0xFFFF) sum += g[q];
          grad[static_cast<int64_t>(t) * a.C + lab[j]] = gw * sum;
        }
        float x = mo[j] + wself[j];
        for (unsigned q = s_ch[dst[j]]; q != kNone; q = s_ch[K + q] >> 16)
          x = logadd(x, m[q] + a.table[static_cast<int64_t>(a.C) + static_cast<int64_t>(s_lab[K + q]) * a.C + lab[j]]);
        beta[j] = x;
      }
    }
    pp ^= 1;
  }
  GTNX_G float* occ = a.occ ? a.occ + static_cast<int64_t>(blockIdx.x) * 2 * SM : nullptr;
  GTNX_G int* csr = a.csr ? a.csr + static_cast<int64_t>(blockIdx.x) * 3 * SM : nullptr;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = tid + j * WG;
    if (i < A) {
      if (garc) {
        float s = sum_start[j];
        for (int k = 0; k < hi[j] - lo[j]; ++k) s += edge[off[j] + k];
        garc[i] = gw * s;
      }
      if (occ) {
        occ[i] = gw * sum_self[j];
        occ[SM + i] = gw * sum_start[j];
        csr[i] = off[j];
        csr[SM + i] = lo[j];
        csr[2 * SM + i] = hi[j] - lo[j];
      }
    }
  }
}

// one wave per table row: the wave loads, lane 0 adds one value after the other
__global__ __launch_bounds__(64) void asg_lattice_table_kernel(AsgLatticeArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_f[];
  float* acc = s_f;  // [C]
  const int lane = static_cast<int>(threadIdx.x);
  const int r = static_cast<int>(blockIdx.x);
  const int C = a.C, SM = a.SM;
  GTNX_G float* out = r < C ? a.grad_table + static_cast<int64_t>(C) + static_cast<int64_t>(r) * C : a.grad_table;
  for (int j = lane; j < C; j += 64) acc[j] = a.table_first ? 0.0f : out[j];
  wg_sync<64>();
  for (int u = 0; u < a.count; ++u) {
    const int b = a.utt0 + u;
    const float gw = a.weights[b];
    const float sc = a.scores[b - a.score0];
    if (gw == 0.0f || !(sc > NEG_INF)) continue;  // (uniform: the backward's test; a score says the lattice is valid)
    const int A = min(max(a.num_arcs[b], 0), a.A);
    const GTNX_G int* arcs = a.arcs + static_cast<int64_t>(b) * a.row_stride;
    const GTNX_G float* occ = a.occ + static_cast<int64_t>(u) * 2 * SM;
    const GTNX_G int* csr = a.csr + static_cast<int64_t>(u) * 3 * SM;
    const GTNX_G float* edge = a.edge + static_cast<int64_t>(u) * a.max_edges;
    for (int base = 0; base < A; base += 64) {
      const int i = base + lane;
      int lb = -1;
      float v = 0.0f;
      bool mine = false;
      if (i < A) {
        lb = arcs[3 * static_cast<int64_t>(i) + 2];
        if (r < C) {
          mine = lb == r;
        } else {
          mine = arcs[3 * static_cast<int64_t>(i)] == 0;
          if (mine) v = occ[SM + i];
        }
      }
      unsigned long long mask = __ballot(mine);
      while (mask) {  // (uniform)
        const int ln = __ffsll(mask) - 1;
        mask &= mask - 1;
        if (r == C) {
          const int lu = __shfl(lb, ln);
          const float vu = __shfl(v, ln);
          if (lane == 0) acc[lu] = acc[lu] + vu;
          continue;
        }
        const int ai = base + ln;
        const int off = csr[ai], lo = csr[SM + ai], deg = csr[2 * SM + ai];
        if (lane == 0) acc[r] = acc[r] + occ[ai];
        for (int k0 = 0; k0 < deg; k0 += 64) {
          const int k = k0 + lane;
          int lq = 0;
          float vq = 0.0f;
          if (k < deg) {
            lq = arcs[3 * static_cast<int64_t>(lo + k) + 2];
            vq = gw * edge[off + k];
          }
          const int n = min(64, deg - k0);
          for (int s = 0; s < n; ++s) {
            const int lu = __shfl(lq, s);
            const float vu = __shfl(vq, s);
            if (lane == 0) acc[lu] = acc[lu] + vu;
          }
        }
      }
    }
  }
  wg_sync<64>();
  for (int j = lane; j < C; j += 64) out[j] = acc[j];
}

size_t forward_lds(int SM) { return sizeof(float) * (4 * size_t(SM) + 16); }
size_t backward_lds(int SM) { return sizeof(float) * (9 * size_t(SM) + 16); }

template <int WG, int PER>
void launch_forward(const AsgLatticeArgs& a, hipStream_t st) {
  static std::atomic<uint64_t> done{0};
  if (gtnx_first_on_device first{done})
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(asg_lattice_forward_kernel<WG, PER>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, int(forward_lds(kAsgLatticeMaxStates)));
  hipLaunchKernelGGL((asg_lattice_forward_kernel<WG, PER>), dim3(static_cast<unsigned>(a.count)), dim3(WG),
                     forward_lds(a.SM), st, a);
}

template <int WG, int PER>
void launch_backward(const AsgLatticeArgs& a, hipStream_t st) {
  static std::atomic<uint64_t> done{0};
  if (gtnx_first_on_device first{done})
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(asg_lattice_backward_kernel<WG, PER>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, int(backward_lds(kAsgLatticeMaxStates)));
  hipLaunchKernelGGL((asg_lattice_backward_kernel<WG, PER>), dim3(static_cast<unsigned>(a.count)), dim3(WG),
                     backward_lds(a.SM), st, a);
}

// fn<WG, PER>(...) with the width and the arcs per lane of asg_lattice_config: six instantiations and no other
#define GTNX_ASG_LATTICE_DISPATCH(SM, fn, ...)               \
  do {                                                       \
    int wg, per;                                             \
    asg_lattice_config(SM, &wg, &per);                       \
    if (wg == 64) fn<64, 1>(__VA_ARGS__);                    \
    else if (wg == 256 && per == 1) fn<256, 1>(__VA_ARGS__); \
    else if (wg == 256) fn<256, 3>(__VA_ARGS__);             \
    else if (per == 1) fn<1024, 1>(__VA_ARGS__);             \
    else if (per == 2) fn<1024, 2>(__VA_ARGS__);             \
    else fn<1024, 4>(__VA_ARGS__);                           \
  } while (0)

}  // namespace

// ctc_lattice_config's cells: max_states bounds nodes + arcs for both criteria, so the same argument picks the same cell
void asg_lattice_config(int max_states, int* width, int* per_lane) {
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

void launch_asg_lattice_forward(const AsgLatticeArgs& a, hipStream_t st) {
  if (a.count <= 0) return;
  GTNX_ASG_LATTICE_DISPATCH(a.SM, launch_forward, a, st);
}

void launch_asg_lattice_backward(const AsgLatticeArgs& a, hipStream_t st) {
  if (a.count <= 0) return;
  GTNX_ASG_LATTICE_DISPATCH(a.SM, launch_backward, a, st);
}

void launch_asg_lattice_table(const AsgLatticeArgs& a, hipStream_t st) {
  if (a.count <= 0 || !a.grad_table || !a.occ || !a.csr || !a.edge) return;
  hipLaunchKernelGGL(asg_lattice_table_kernel, dim3(static_cast<unsigned>(a.C + 1)), dim3(64),
                     sizeof(float) * size_t(a.C), st, a);
}

}  // namespace gtnx
