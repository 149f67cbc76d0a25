// transducer_tdt.hip -- the token-and-duration transducer (TDT) log score of a padded batch over device-resident joint
// logits x [B][T][U+1][C + D] and its gradient under caller-supplied weights (DESIGN section 47 holds the contract;
// tests/transducer_tdt_fp.py has the recurrences in float64).  Entries 0 .. C-1 of a row are token logits, C .. C+D-1 the
// logits of durations 0 .. D-1; a blank arc of duration d >= 1 goes from (t, u) to (t + d, u), a label arc of duration
// d >= 0 to (t + d, u + 1), each weighing lp_tok + lp_dur[d].  Node (b, t, u) is live when t < T_b and u <= U_b.
//
//   rows:   transducer.hip's ladder over a row of C + D entries held in registers, with two masked reductions in the
//           same pass (maximum and sum of exp for c < C and for c >= C; the boundary may fall inside a lane's vector).
//           One lane stores the D + 4 values (lp_blank - sigma, lp_label - sigma, lse_tok, lse_dur, lp_dur[0 .. D-1]).
//           A row either of whose segments holds NaN or +inf, or nothing finite, stores -inf in every log-probability: a
//           node no path leaves.  Rows above 4096 entries run an online maximum / sum per segment, one wave per row.
//           The ladder has more rungs than transducer.hip's: a row is C + D entries, so the common C = 2^n lands just
//           ABOVE a power of two, where the next doubling would leave three quarters of the registers as padding.
//   sweep:  one wave per utterance and direction, no LDS, no barrier, templated on (K, D).  Lane l owns K columns and
//           does row t = s - l at step s, as transducer.hip's.  alpha[t, u] has up to 2 D - 1 terms; the kernel keeps ONE
//           three-way logadd per node on the chain: the d = 0 label arc from (t, u - 1) (just computed, or lane l - 1's
//           DPP move), the d = 1 blank arc from (t - 1, u) (the lane's own previous step, as transducer.hip's `keep`),
//           and R[u][0], a finished partial log-sum of everything older.  R is a register ring of depth D - 1 per
//           column: once alpha[t, u] is known its arcs of duration d are scattered, with the node's own weights, into
//           the ring slots of rows t + d -- off the chain, after the step's K chain links.  The left neighbour's D label
//           contributions travel as D DPP moves of already weighted values (section 47 says why).  beta gathers instead:
//           the weights are the receiving node's, so a ring of the D - 1 last beta rows per column, plus one ring for
//           the right neighbour's column fed by ONE DPP move, is reduced with the next row's weights into G[u] one step
//           ahead; the chain link is logadd3(label d = 0 from (t, u + 1), blank d = 1 from (t + 1, u), G[u]).
//   grad:   per row of the slice alpha, the score, up to 2 D - 1 betas and the plane give the arc occupancies ob_d, ol_d;
//           one pass over the C + D logits at the rows kernel's widths stores both parts.  Rows nothing passes through
//           are stored as zeros without a load.  Every row of the output is stored exactly once.
// Every store is a plain C++ store; there are no atomics and no inline assembly, and no workgroup waits on another.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "kernels.h"

namespace gtnx {
namespace {

constexpr float NEG_INF = -__builtin_inff();
constexpr float POS_INF = __builtin_inff();
constexpr int kWG = 256;       // the streaming kernels' workgroup
constexpr int kRegRow = 4096;  // the widest row the rows kernel holds in registers
typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// row r of the slice -> (b, t, u), T_b, U_b; true for a live node
struct Node {
  int b, t, u, Tb, Ub, global;  // global: the node's index in the whole batch
};
__device__ __forceinline__ bool decode(const TransducerTdtArgs& a, int r, Node& n) {
  const int per = a.T * a.U1;
  const int lb = r / per, rem = r - lb * per;
  n.b = a.utt0 + lb;
  n.t = rem / a.U1;
  n.u = rem - n.t * a.U1;
  n.global = n.b * per + rem;
  n.Tb = a.frames[n.b];
  n.Ub = a.tlen[n.b];
  return n.Tb >= 1 && n.Tb <= a.T && n.Ub >= 0 && n.Ub < a.U1 && n.t < n.Tb && n.u <= n.Ub;
}

// y[u] of a live node with u < U_b, or -1 where there is no label to leave the node by
__device__ __forceinline__ int label_of(const TransducerTdtArgs& a, const Node& n) {
  if (n.u >= n.Ub) return -1;
  const int tok = a.targets[static_cast<int64_t>(n.b) * (a.U1 - 1) + n.u];
  return (tok >= 0 && tok < a.C && tok != a.blank) ? tok : -1;
}

template <int G>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}
template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// the D + 4 values of one row from its two lse: by one lane of the group
__device__ __forceinline__ void store_plane(const TransducerTdtArgs& a, int r, const Node& n, const GTNX_G float* row,
                                            float lse_t, float lse_d) {
  GTNX_G float* out = a.rows + static_cast<int64_t>(r) * (a.D + 4);
  if (!(fabsf(lse_t) < POS_INF) || !(fabsf(lse_d) < POS_INF)) {  // NaN or +inf in a segment, or nothing finite in it
    out[0] = NEG_INF;
    out[1] = NEG_INF;
    out[2] = 0.0f;
    out[3] = 0.0f;
    for (int d = 0; d < a.D; ++d) out[4 + d] = NEG_INF;
    return;
  }
  const int tok = label_of(a, n);
  out[0] = row[a.blank] - lse_t - a.sigma;
  out[1] = tok >= 0 ? row[tok] - lse_t - a.sigma : NEG_INF;
  out[2] = lse_t;
  out[3] = lse_d;
  for (int d = 0; d < a.D; ++d) out[4 + d] = row[a.C + d] - lse_d;
}

// ---- rows, C + D <= 4096: a group of G lanes holds a row in NV registers of W floats per lane ----
template <int G, int NV, int W>
__global__ __launch_bounds__(kWG) void transducer_tdt_rows_kernel(TransducerTdtArgs a) {
  const int tid = static_cast<int>(threadIdx.x), g = tid & (G - 1);
  const int64_t r64 = static_cast<int64_t>(blockIdx.x) * (kWG / G) + tid / G;
  if (r64 >= static_cast<int64_t>(a.count) * a.T * a.U1) return;
  const int r = static_cast<int>(r64);
  Node n;
  if (!decode(a, r, n)) return;  // (a whole group leaves together)
  const int CD = a.C + a.D, C = a.C;
  const GTNX_G float* row = a.x + static_cast<int64_t>(n.global) * CD;
  float v[NV * W];
  if (W == 4) {
    const GTNX_G f4* row4 = reinterpret_cast<const GTNX_G f4*>(row);
    const int nvec = CD >> 2;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int i = j * G + g;
      f4 q = {NEG_INF, NEG_INF, NEG_INF, NEG_INF};
      if (i < nvec) q = row4[i];
      v[j * W + 0] = q.x;
      v[j * W + 1 % W] = q.y;
      v[j * W + 2 % W] = q.z;
      v[j * W + 3 % W] = q.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int i = j * G + g;
      v[j * W] = i < CD ? row[i] : NEG_INF;
    }
  }
  // the entry in register j is a token logit below C, a duration logit (or padding, -inf) from C on
  float mt = NEG_INF, md = NEG_INF;
#pragma unroll
  for (int j = 0; j < NV * W; ++j) {
    const bool tk = ((j / W) * G + g) * W + j % W < C;
    mt = fmaxf(mt, tk ? v[j] : NEG_INF);
    md = fmaxf(md, tk ? NEG_INF : v[j]);
  }
  mt = group_max<G>(mt);
  md = group_max<G>(md);
  // (a NaN entry passes fmaxf and makes its segment's sum NaN; +inf and an all -inf segment give inf - inf: the lse tells)
  float st = 0.0f, sd = 0.0f;
#pragma unroll
  for (int j = 0; j < NV * W; ++j) {
    const bool tk = ((j / W) * G + g) * W + j % W < C;
    const float e = expf(v[j] - (tk ? mt : md));
    st += tk ? e : 0.0f;
    sd += tk ? 0.0f : e;
  }
  st = group_sum<G>(st);
  sd = group_sum<G>(sd);
  if (g == 0) store_plane(a, r, n, row, mt + logf(st), md + logf(sd));
}

// ---- rows, C + D > 4096: one wave per row, an online maximum / sum per lane and segment, then one combine ----
template <int W>
__global__ __launch_bounds__(kWG) void transducer_tdt_rows_wide_kernel(TransducerTdtArgs a) {
  const int tid = static_cast<int>(threadIdx.x), g = tid & 63;
  const int64_t r64 = static_cast<int64_t>(blockIdx.x) * (kWG / 64) + tid / 64;
  if (r64 >= static_cast<int64_t>(a.count) * a.T * a.U1) return;
  const int r = static_cast<int>(r64);
  Node n;
  if (!decode(a, r, n)) return;
  const int CD = a.C + a.D, C = a.C;
  const GTNX_G float* row = a.x + static_cast<int64_t>(n.global) * CD;
  float m[2] = {NEG_INF, NEG_INF}, s[2] = {0.0f, 0.0f};  // [0] tokens, [1] durations
  bool bad[2] = {false, false};                          // NaN or +inf seen
  const int cnt = W == 4 ? CD >> 2 : CD;
  for (int i = g; i < cnt; i += 64) {
    float q[W];
    if (W == 4) {
      const f4 t4 = reinterpret_cast<const GTNX_G f4*>(row)[i];
      q[0] = t4.x;
      q[1 % W] = t4.y;
      q[2 % W] = t4.z;
      q[3 % W] = t4.w;
    } else {
      q[0] = row[i];
    }
    const int c0 = i * W;
#pragma unroll
    for (int seg = 0; seg < 2; ++seg) {
      if (seg == 0 ? c0 >= C : c0 + W <= C) continue;  // (nothing of this segment in the vector)
      float cm = m[seg];
#pragma unroll
      for (int k = 0; k < W; ++k) {
        if ((c0 + k < C) != (seg == 0)) continue;
        bad[seg] |= !(q[k] < POS_INF);
        cm = fmaxf(cm, q[k]);
      }
      if (cm > NEG_INF && !bad[seg]) {
        float add = 0.0f;
#pragma unroll
        for (int k = 0; k < W; ++k) add += (c0 + k < C) == (seg == 0) ? expf(q[k] - cm) : 0.0f;
        s[seg] = s[seg] * expf(m[seg] - cm) + add;  // (m == -inf: s is 0 and stays 0)
        m[seg] = cm;
      }
    }
  }
  float lse[2];
#pragma unroll
  for (int seg = 0; seg < 2; ++seg) {
    const float M = group_max<64>(m[seg]);
    const float S = group_sum<64>(m[seg] > NEG_INF ? s[seg] * expf(m[seg] - M) : 0.0f);
    lse[seg] = __any(bad[seg]) ? POS_INF : M + logf(S);
  }
  if (g == 0) store_plane(a, r, n, row, lse[0], lse[1]);
}

// ---- sweep ----
// (max + __logf of a sum of __expf, as transducer.hip's logadd: the chain is what the kernel costs)
__device__ __forceinline__ float logadd3(float x, float y, float z) {
  const float m = fmaxf(fmaxf(x, y), z);
  const float r = m + __logf(__expf(x - m) + __expf(y - m) + __expf(z - m));
  return m > NEG_INF ? r : NEG_INF;  // (all -inf: the differences are NaN)
}
// lane l's value of lane l - 1 (lane 0: `edge`) / of lane l + 1 (lane 63: `edge`); every lane of the wave takes part
__device__ __forceinline__ float from_lower_lane(float v, float edge) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float from_upper_lane(float v, float edge) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x130, 0xf, 0xf, false));
}

template <int K, int D>
__global__ __launch_bounds__(64) void transducer_tdt_sweep_kernel(TransducerTdtArgs a) {
  constexpr int P = D + 4;               // the plane's floats per node
  constexpr int E = D > 2 ? D - 2 : 1;   // durations 2 .. D-1 (one unused register at D == 2)
  const int lane = static_cast<int>(threadIdx.x);
  const int lb = static_cast<int>(blockIdx.x), b = a.utt0 + lb;
  const bool backward = blockIdx.y == 1;
  const int Tb = uni(a.frames[b]), Ub = uni(a.tlen[b]);
  const int U1 = a.U1;
  if (!(Tb >= 1 && Tb <= a.T && Ub >= 0 && Ub < U1)) {
    if (!backward && lane == 0) a.scores[b] = NEG_INF;
    return;
  }
  const int64_t base = static_cast<int64_t>(lb) * a.T * U1;
  const GTNX_G float* rows = a.rows + base * P;
  const int u0 = lane * K;
  const int lmax = Ub / K, kend = Ub - lmax * K;  // the lane and the register that own column U_b
  const int steps = Tb + lmax;
  const bool mine = lane <= lmax;
  // (t outside 0 .. T_b - 1 and u > U_b load nothing: every weight -inf)
  auto live = [&](int t, int k) { return t >= 0 && t < Tb && u0 + k <= Ub; };
  auto at = [&](int t, int k) { return rows + (static_cast<int64_t>(t) * U1 + u0 + k) * P; };

  if (!backward) {
    float R[K][D - 1];  // R[k][j]: the finished log-sum of the arcs into (t + j, u0 + k) from rows before t, less `keep`
    float keep[K];      // alpha[t-1, u] + w_blank[t-1, u][1]
    float carry[D];     // alpha[t, u0 + K - 1] + w_label[..][d] of the row done last, for lane l + 1
    float nb[K], nl[K], n0[K], n1[K];  // (lp_blank, lp_label, lp_dur[0], lp_dur[1]) of the row to do next
#pragma unroll
    for (int k = 0; k < K; ++k) {
      keep[k] = NEG_INF;
#pragma unroll
      for (int j = 0; j < D - 1; ++j) R[k][j] = NEG_INF;
    }
#pragma unroll
    for (int d = 0; d < D; ++d) carry[d] = NEG_INF;
    if (lane == 0) keep[0] = 0.0f;  // (the start enters node (0, 0))
    auto load4 = [&](int t) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        nb[k] = nl[k] = n0[k] = n1[k] = NEG_INF;
        if (live(t, k)) {
          const GTNX_G float* p = at(t, k);
          nb[k] = p[0];
          nl[k] = p[1];
          n0[k] = p[4];
          n1[k] = p[5];
        }
      }
    };
    GTNX_G float* plane = a.alpha ? a.alpha + base : nullptr;
    load4(-lane);
    for (int s = 0; s < steps; ++s) {
      const int t = s - lane;
      float cb[K], cl[K], wl0[K], wb1[K], c1[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {  // the chain's two weights are formed here, a step before alpha arrives
        cb[k] = nb[k];
        cl[k] = nl[k];
        c1[k] = n1[k];
        wl0[k] = nl[k] + n0[k];
        wb1[k] = nb[k] + n1[k];
      }
      load4(t + 1);
      float e[K][E];  // lp_dur[2 .. D-1] of this row: used after the chain
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int d = 2; d < D; ++d) e[k][d - 2] = live(t, k) ? at(t, k)[4 + d] : NEG_INF;
      float in[D];
#pragma unroll
      for (int d = 0; d < D; ++d) in[d] = from_lower_lane(carry[d], NEG_INF);
      if (mine && t >= 0 && t < Tb) {
        float al[K];
        float left = in[0];
#pragma unroll
        for (int k = 0; k < K; ++k) {
          al[k] = logadd3(left, R[k][0], keep[k]);
          if (plane && u0 + k <= Ub) plane[static_cast<int64_t>(t) * U1 + u0 + k] = al[k];
          left = al[k] + wl0[k];
          keep[k] = al[k] + wb1[k];
        }
        // off the chain: the ring moves on one row and takes this row's arcs of duration d into the slot of row t + d
        // (a label arc that lands on row T_b carries no path; a blank arc does, at u == U_b, and is the score's term)
#pragma unroll
        for (int k = K - 1; k >= 0; --k) {
#pragma unroll
          for (int j = 0; j < D - 1; ++j) {
            const int d = j + 1;
            const float old = j + 1 < D - 1 ? R[k][j + 1] : NEG_INF;
            const float blank = d >= 2 ? al[k] + (cb[k] + e[k][d >= 2 ? d - 2 : 0]) : NEG_INF;
            float label = in[d];
            if (k > 0) label = al[k - 1] + (cl[k - 1] + (d == 1 ? c1[k - 1] : e[k - 1][d >= 2 ? d - 2 : 0]));
            R[k][j] = logadd3(old, blank, t + d < Tb ? label : NEG_INF);
          }
        }
        carry[0] = left;
#pragma unroll
        for (int d = 1; d < D; ++d)
          carry[d] = t + d < Tb ? al[K - 1] + (cl[K - 1] + (d == 1 ? c1[K - 1] : e[K - 1][d >= 2 ? d - 2 : 0])) : NEG_INF;
      }
    }
    if (lane == lmax) {  // the ring's head now belongs to row T_b: the end arcs of durations >= 2, `keep` the one of 1
      float sc = NEG_INF;
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (k == kend) sc = logadd3(R[k][0], keep[k], NEG_INF);
      a.scores[b] = sc;
    }
  } else {
    float Bq[K][D - 1];  // Bq[k][j] = beta[t + 1 + j, u0 + k] for the row t to do next
    float NB[D - 1];     // the same ring for column u0 + K, lane l + 1's first
    float G[K], wl0[K], wb1[K];  // of the row to do next: everything off the chain reduced, and the chain's two weights
    float w[K][D + 2];   // (lp_blank, lp_label, lp_dur[0 .. D-1]) of the row to prepare
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int j = 0; j < D - 1; ++j) Bq[k][j] = NEG_INF;
#pragma unroll
    for (int j = 0; j < D - 1; ++j) NB[j] = NEG_INF;
    if (lane == lmax) {
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (k == kend) Bq[k][0] = 0.0f;  // (beta of the virtual end, at (T_b, U_b); only blank arcs reach it)
    }
    auto load_row = [&](int t) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const bool ok = live(t, k);
        w[k][0] = ok ? at(t, k)[0] : NEG_INF;
        w[k][1] = ok ? at(t, k)[1] : NEG_INF;
#pragma unroll
        for (int d = 0; d < D; ++d) w[k][2 + d] = ok ? at(t, k)[4 + d] : NEG_INF;
      }
    };
    // row tp's weights against the rings (which hold beta[tp + 1 ..]): one log-sum of 2 D - 3 terms per column
    auto prepare = [&](int tp) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        wl0[k] = w[k][1] + w[k][2];
        wb1[k] = w[k][0] + w[k][3];
        float term[2 * D - 3];
#pragma unroll
        for (int d = 2; d < D; ++d) term[d - 2] = (w[k][0] + w[k][2 + d]) + Bq[k][d - 1];
#pragma unroll
        for (int d = 1; d < D; ++d) {
          const float br = k + 1 < K ? Bq[k + 1 < K ? k + 1 : k][d - 1] : NB[d - 1];
          term[D - 2 + d - 1] = tp + d < Tb ? (w[k][1] + w[k][2 + d]) + br : NEG_INF;
        }
        float m = NEG_INF;
#pragma unroll
        for (int i = 0; i < 2 * D - 3; ++i) m = fmaxf(m, term[i]);
        float sum = 0.0f;
#pragma unroll
        for (int i = 0; i < 2 * D - 3; ++i) sum += __expf(term[i] - m);
        G[k] = m > NEG_INF ? m + __logf(sum) : NEG_INF;
      }
    };
    GTNX_G float* plane = a.beta + base;
    load_row(Tb - 1);
    prepare(Tb - 1);
    float carry = NEG_INF;
    for (int s = 0; s < steps; ++s) {
      const int t = Tb - 1 - (s - (lmax - lane));
      load_row(t - 1);
      const float right = from_upper_lane(carry, NEG_INF);
      if (mine && t >= 0 && t < Tb) {
        float be[K];
        float r = right;
#pragma unroll
        for (int k = K - 1; k >= 0; --k) {
          be[k] = logadd3(wl0[k] + r, wb1[k] + Bq[k][0], G[k]);
          if (u0 + k <= Ub) plane[static_cast<int64_t>(t) * U1 + u0 + k] = be[k];
          r = be[k];
        }
        carry = r;
        // off the chain: the rings take this row, then the next row's weights
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
          for (int j = D - 2; j > 0; --j) Bq[k][j] = Bq[k][j - 1];
          Bq[k][0] = be[k];
        }
#pragma unroll
        for (int j = D - 2; j > 0; --j) NB[j] = NB[j - 1];
        NB[0] = right;
        prepare(t - 1);
      }
    }
  }
}

// ---- gradient: a group of G lanes per row of the slice, W floats per load and store ----
template <int G, int W>
__global__ __launch_bounds__(kWG) void transducer_tdt_grad_kernel(TransducerTdtArgs a) {
  const int tid = static_cast<int>(threadIdx.x), g = tid & (G - 1);
  const int64_t r64 = static_cast<int64_t>(blockIdx.x) * (kWG / G) + tid / G;
  if (r64 >= static_cast<int64_t>(a.count) * a.T * a.U1) return;
  const int r = static_cast<int>(r64);
  Node n;
  const bool live = decode(a, r, n);
  const int C = a.C, D = a.D, CD = C + D;
  float od[kTransducerTdtMaxD];  // ob_d + ol_d
#pragma unroll
  for (int d = 0; d < kTransducerTdtMaxD; ++d) od[d] = 0.0f;
  float ob = 0.0f, ol = 0.0f, lse_t = 0.0f, lse_d = 0.0f, w = 0.0f;
  int tok = -1;
  if (live) {
    const float sc = a.scores[n.b];
    if (sc > NEG_INF) {
      const GTNX_G float* p = a.rows + static_cast<int64_t>(r) * (D + 4);
      const float al = a.alpha[r];
      const float lb = p[0], ll = p[1];
      // (every term is finite or -inf, so is the sum; the score is finite)
#pragma unroll
      for (int d = 0; d < kTransducerTdtMaxD; ++d) {
        if (d >= D) continue;
        const float ld = p[4 + d];
        const int64_t to = static_cast<int64_t>(r) + static_cast<int64_t>(d) * a.U1;
        if (d >= 1) {
          const float bb = n.t + d < n.Tb ? a.beta[to] : (n.t + d == n.Tb && n.u == n.Ub ? 0.0f : NEG_INF);
          const float o = expf(al + (lb + ld) + bb - sc);
          ob += o;
          od[d] += o;
        }
        if (n.u < n.Ub && n.t + d < n.Tb) {
          const float o = expf(al + (ll + ld) + a.beta[to + 1] - sc);
          ol += o;
          od[d] += o;
        }
      }
      lse_t = p[2];
      lse_d = p[3];
      w = a.weights[n.b];
      tok = label_of(a, n);
    }
  }
  const float occ = ob + ol;
  const int64_t off = static_cast<int64_t>(n.global) * CD;
  const GTNX_G float* row = a.x + off;
  GTNX_G float* out = a.grad + off;
  const int cnt = W == 4 ? CD >> 2 : CD;
  const int blank = a.blank;
  if (!(occ > 0.0f)) {  // never read, a -inf score, a dead row, or a node nothing passes through
    if (W == 4) {
      const f4 z = {0.0f, 0.0f, 0.0f, 0.0f};
      for (int i = g; i < cnt; i += G) reinterpret_cast<GTNX_G f4*>(out)[i] = z;
    } else {
      for (int i = g; i < cnt; i += G) out[i] = 0.0f;
    }
    return;
  }
#pragma unroll 4
  for (int i = g; i < cnt; i += G) {
    float q[W];
    if (W == 4) {
      const f4 t4 = reinterpret_cast<const GTNX_G f4*>(row)[i];
      q[0] = t4.x;
      q[1 % W] = t4.y;
      q[2 % W] = t4.z;
      q[3 % W] = t4.w;
    } else {
      q[0] = row[i];
    }
    if (i * W + W <= C) {  // token logits only: all but the last one to three vectors of a row
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const int c = i * W + k;
        const float hit = (c == blank ? ob : 0.0f) + (c == tok ? ol : 0.0f);
        q[k] = w * (hit - expf(q[k] - lse_t) * occ);
      }
    } else {  // the vector the boundary falls in, and the durations
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const int c = i * W + k;
        float hit = (c == blank ? ob : 0.0f) + (c == tok ? ol : 0.0f);
#pragma unroll
        for (int d = 0; d < kTransducerTdtMaxD; ++d) hit = c - C == d ? od[d] : hit;
        q[k] = w * (hit - expf(q[k] - (c < C ? lse_t : lse_d)) * occ);
      }
    }
    if (W == 4) {
      const f4 t4 = {q[0], q[1 % W], q[2 % W], q[3 % W]};
      reinterpret_cast<GTNX_G f4*>(out)[i] = t4;
    } else {
      out[i] = q[0];
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline unsigned blocks_for(const TransducerTdtArgs& a, int rows_per_block) {
  const int64_t total = static_cast<int64_t>(a.count) * a.T * a.U1;
  return static_cast<unsigned>((total + rows_per_block - 1) / rows_per_block);
}

template <int G, int NV, int W>
void rows_launch(const TransducerTdtArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((transducer_tdt_rows_kernel<G, NV, W>), dim3(blocks_for(a, kWG / G)), dim3(kWG), 0, st, a);
}
template <int G, int W>
void grad_launch(const TransducerTdtArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((transducer_tdt_grad_kernel<G, W>), dim3(blocks_for(a, kWG / G)), dim3(kWG), 0, st, a);
}
template <int K, int D>
void sweep_launch(const TransducerTdtArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((transducer_tdt_sweep_kernel<K, D>), dim3(unsigned(a.count), a.beta ? 2u : 1u), dim3(64), 0, st, a);
}
template <int D>
void sweep_by_k(const TransducerTdtArgs& a, hipStream_t st) {
  const int k = (a.U1 + 63) / 64;
  if (k <= 1) sweep_launch<1, D>(a, st);
  else if (k <= 2) sweep_launch<2, D>(a, st);
  else if (k <= 4) sweep_launch<4, D>(a, st);
  else if (k <= 8) sweep_launch<8, D>(a, st);
  else sweep_launch<16, D>(a, st);
}

}  // namespace

void launch_transducer_tdt_rows(const TransducerTdtArgs& a, hipStream_t st) {
  if (a.count <= 0) return;
  const int CD = a.C + a.D;
  if ((CD & 3) == 0 && aligned16(a.x)) {
    const int nvec = CD >> 2;
    if (CD > kRegRow)
      hipLaunchKernelGGL(transducer_tdt_rows_wide_kernel<4>, dim3(blocks_for(a, kWG / 64)), dim3(kWG), 0, st, a);
    else if (nvec <= 8) rows_launch<8, 1, 4>(a, st);
    else if (nvec <= 32) rows_launch<32, 1, 4>(a, st);
    else if (nvec <= 128) rows_launch<64, 2, 4>(a, st);
    else if (nvec <= 192) rows_launch<64, 3, 4>(a, st);
    else if (nvec <= 256) rows_launch<64, 4, 4>(a, st);
    else if (nvec <= 320) rows_launch<64, 5, 4>(a, st);
    else if (nvec <= 384) rows_launch<64, 6, 4>(a, st);
    else if (nvec <= 512) rows_launch<64, 8, 4>(a, st);
    else if (nvec <= 640) rows_launch<64, 10, 4>(a, st);
    else if (nvec <= 768) rows_launch<64, 12, 4>(a, st);
    else rows_launch<64, 16, 4>(a, st);
  } else {
    if (CD > kRegRow)
      hipLaunchKernelGGL(transducer_tdt_rows_wide_kernel<1>, dim3(blocks_for(a, kWG / 64)), dim3(kWG), 0, st, a);
    else if (CD <= 8) rows_launch<8, 1, 1>(a, st);
    else if (CD <= 32) rows_launch<32, 1, 1>(a, st);
    else if (CD <= 256) rows_launch<64, 4, 1>(a, st);
    else if (CD <= 512) rows_launch<64, 8, 1>(a, st);
    else if (CD <= 768) rows_launch<64, 12, 1>(a, st);
    else if (CD <= 1024) rows_launch<64, 16, 1>(a, st);
    else if (CD <= 1280) rows_launch<64, 20, 1>(a, st);
    else if (CD <= 1536) rows_launch<64, 24, 1>(a, st);
    else if (CD <= 2048) rows_launch<64, 32, 1>(a, st);
    else if (CD <= 3072) rows_launch<64, 48, 1>(a, st);
    else rows_launch<64, 64, 1>(a, st);
  }
  HIP_CHECK(hipGetLastError());
}

void launch_transducer_tdt_sweep(const TransducerTdtArgs& a, hipStream_t st) {
  if (a.count <= 0) return;
  switch (a.D) {
    case 2: sweep_by_k<2>(a, st); break;
    case 3: sweep_by_k<3>(a, st); break;
    case 4: sweep_by_k<4>(a, st); break;
    case 5: sweep_by_k<5>(a, st); break;
    case 6: sweep_by_k<6>(a, st); break;
    case 7: sweep_by_k<7>(a, st); break;
    default: sweep_by_k<8>(a, st); break;
  }
  HIP_CHECK(hipGetLastError());
}

void launch_transducer_tdt_grad(const TransducerTdtArgs& a, hipStream_t st) {
  if (a.count <= 0) return;
  const int CD = a.C + a.D;
  if ((CD & 3) == 0 && aligned16(a.x) && aligned16(a.grad)) {
    const int nvec = CD >> 2;
    if (nvec <= 8) grad_launch<8, 4>(a, st);
    else if (nvec <= 32) grad_launch<32, 4>(a, st);
    else grad_launch<64, 4>(a, st);
  } else {
    if (CD <= 8) grad_launch<8, 1>(a, st);
    else if (CD <= 32) grad_launch<32, 1>(a, st);
    else grad_launch<64, 1>(a, st);
  }
  HIP_CHECK(hipGetLastError());
}

}  // namespace gtnx
