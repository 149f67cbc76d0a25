// transducer_pruned.hip -- the pruned (banded) transducer log score of a padded batch over device-resident joint logits
// x [B][T][S][C] with a per-frame band start r_t = ranges[b][t], and its gradient under caller-supplied weights (DESIGN
// section 44 holds the contract; tests/transducer_pruned_fp.py has the recurrences in float64).  Band node (b, t, s)
// stands for lattice node (t, u = r_t + s) of section 42's lattice; it is live when t < T_b, 0 <= r_t <= U and
// u <= U_b.  A frame whose r_t is outside 0 .. U has no live node, so r_t never becomes an address.
//
//   rows:   transducer.hip's streaming rows kernel with the band decode: a group of G lanes holds one live row in
//           registers (16-byte loads when C % 4 == 0 and the tensor is aligned), stores the compact triple (lp_blank,
//           lp_label, lse); an online loop above 4096 labels; a two-entry gather without `normalize`.
//   sweep:  a group of G = 8, 16, 32 or 64 lanes (the smallest G >= S) per utterance and direction, 64 / G utterances per
//           wave, no LDS and no barrier.  Lane s owns band position s and keeps one node's value in registers.  The walk
//           is skewed by the ABSOLUTE column: lane s advances frame t at step k = t + r_t + s = t + u, so both
//           predecessors of (t, u) finished at step k - 1: the label predecessor (t, u - 1) in lane s - 1 (a DPP wave
//           shift, the group's edge feeds -inf) and the blank predecessor (t - 1, u) in lane s + (r_t - r_{t-1}), a
//           per-lane variable cross-lane read (ds_bpermute) of that lane's latest value.  Between two frames a lane
//           idles r_t - r_{t-1} steps; every lane keeps a frame counter of its own and the wave leaves when no lane has
//           a frame left.  A lane takes its frame when k has REACHED its step, so ranges that decrease (refused: the
//           score is -inf) only make a lane late, never stuck; every lane sees every r_t and raises the same flag.
//           Beta mirrors both axes: step (T_b - 1 - t) + (r_{T_b-1} - r_t) + (S - 1 - s), the label successor from lane
//           s + 1, the blank successor from lane s - (r_{t+1} - r_t).  Each lane has loaded r and the compact pair of its
//           next frame before it computes the current one.  About T_b + U_b + S steps of one logadd.
//   grad:   transducer.hip's streaming gradient kernel with the band decode and the band's neighbours beta[t, s + 1] and
//           beta[t + 1, s - (r_{t+1} - r_t)].  Every row of the output is stored exactly once.
//   occupancy: exp(alpha + beta - score) of a FULL lattice's planes (launch_transducer_sweep's), every element stored
//           once, for torch_loss.transducer_prune_ranges.
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
using Args = TransducerPrunedArgs;

// row r of the slice -> (b, t, s), u = r_t + s, T_b, U_b; true for a live node
struct Node {
  int b, t, s, u, rt, Tb, Ub;
  int64_t global;  // the band row's index in the whole batch
};
__device__ __forceinline__ bool decode(const Args& a, int r, Node& n) {
  const int per = a.T * a.S;
  const int lb = r / per, rem = r - lb * per;
  n.b = a.utt0 + lb;
  n.t = rem / a.S;
  n.s = rem - n.t * a.S;
  n.global = static_cast<int64_t>(n.b) * per + rem;
  n.Tb = a.frames[n.b];
  n.Ub = a.tlen[n.b];
  n.rt = n.u = -1;
  if (!(n.Tb >= 1 && n.Tb <= a.T && n.Ub >= 0 && n.Ub < a.U1 && n.t < n.Tb)) return false;
  n.rt = a.ranges[static_cast<int64_t>(n.b) * a.T + n.t];
  if (n.rt < 0 || n.rt >= a.U1) return false;  // (a frame without a node; r_t + s cannot overflow below)
  n.u = n.rt + n.s;
  return n.u <= n.Ub;
}

// y[u] of a live node with u < U_b, or -1 where there is no label to leave the node by
__device__ __forceinline__ int label_of(const Args& a, const Node& n) {
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

// the compact triple of one row from its lse: by one lane of the group
__device__ __forceinline__ void store_triple(const Args& a, int r, const Node& n, const GTNX_G float* row, float lse) {
  GTNX_G float* out = a.rows + static_cast<int64_t>(r) * 3;
  if (!(fabsf(lse) < POS_INF)) {  // NaN or +inf in the row, or nothing but -inf
    out[0] = NEG_INF;
    out[1] = NEG_INF;
    out[2] = 0.0f;
    return;
  }
  const int tok = label_of(a, n);
  out[0] = row[a.blank] - lse;
  out[1] = tok >= 0 ? row[tok] - lse : NEG_INF;
  out[2] = lse;
}

// ---- rows, C <= 4096: a group of G lanes holds a row in NV registers of W floats per lane ----
template <int G, int NV, int W>
__global__ __launch_bounds__(kWG) void transducer_pruned_rows_kernel(Args a) {
  const int tid = static_cast<int>(threadIdx.x), g = tid & (G - 1);
  const int64_t r64 = static_cast<int64_t>(blockIdx.x) * (kWG / G) + tid / G;
  if (r64 >= static_cast<int64_t>(a.count) * a.T * a.S) return;
  const int r = static_cast<int>(r64);
  Node n;
  if (!decode(a, r, n)) return;  // (a whole group leaves together)
  const GTNX_G float* row = a.x + n.global * a.C;
  float v[NV * W];
  if (W == 4) {
    const GTNX_G f4* row4 = reinterpret_cast<const GTNX_G f4*>(row);
    const int nvec = a.C >> 2;
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
      v[j * W] = i < a.C ? row[i] : NEG_INF;
    }
  }
  float m = NEG_INF;
#pragma unroll
  for (int j = 0; j < NV * W; ++j) m = fmaxf(m, v[j]);
  m = group_max<G>(m);
  // (a NaN entry passes fmaxf and makes the sum NaN; +inf and an all -inf row give inf - inf: the lse tells)
  float sum = 0.0f;
#pragma unroll
  for (int j = 0; j < NV * W; ++j) sum += expf(v[j] - m);
  sum = group_sum<G>(sum);
  if (g == 0) store_triple(a, r, n, row, m + logf(sum));
}

// ---- rows, C > 4096: one wave per row, an online maximum / sum per lane, then one combine ----
template <int W>
__global__ __launch_bounds__(kWG) void transducer_pruned_rows_wide_kernel(Args a) {
  const int tid = static_cast<int>(threadIdx.x), g = tid & 63;
  const int64_t r64 = static_cast<int64_t>(blockIdx.x) * (kWG / 64) + tid / 64;
  if (r64 >= static_cast<int64_t>(a.count) * a.T * a.S) return;
  const int r = static_cast<int>(r64);
  Node n;
  if (!decode(a, r, n)) return;
  const GTNX_G float* row = a.x + n.global * a.C;
  float m = NEG_INF, sum = 0.0f;
  bool bad = false;  // NaN or +inf seen
  const int cnt = W == 4 ? a.C >> 2 : a.C;
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
    float cm = m;
#pragma unroll
    for (int k = 0; k < W; ++k) {
      bad |= !(q[k] < POS_INF);
      cm = fmaxf(cm, q[k]);
    }
    if (cm > NEG_INF && !bad) {
      float add = 0.0f;
#pragma unroll
      for (int k = 0; k < W; ++k) add += expf(q[k] - cm);
      sum = sum * expf(m - cm) + add;  // (m == -inf: the sum is 0 and stays 0)
      m = cm;
    }
  }
  const float M = group_max<64>(m);
  const float S = group_sum<64>(m > NEG_INF ? sum * expf(m - M) : 0.0f);
  const bool any_bad = __any(bad);
  if (g == 0) store_triple(a, r, n, row, any_bad ? POS_INF : M + logf(S));
}

// ---- rows, unnormalised: the two entries of a node, nothing else is read ----
__global__ __launch_bounds__(kWG) void transducer_pruned_gather_kernel(Args a) {
  const int64_t r64 = static_cast<int64_t>(blockIdx.x) * kWG + threadIdx.x;
  if (r64 >= static_cast<int64_t>(a.count) * a.T * a.S) return;
  const int r = static_cast<int>(r64);
  Node n;
  if (!decode(a, r, n)) return;
  const GTNX_G float* row = a.x + n.global * a.C;
  const int tok = label_of(a, n);
  float lb = row[a.blank], ll = tok >= 0 ? row[tok] : NEG_INF;
  if (!(lb < POS_INF) || !(ll < POS_INF)) lb = ll = NEG_INF;  // (NaN or +inf: a node no path leaves)
  GTNX_G float* out = a.rows + static_cast<int64_t>(r) * 3;
  out[0] = lb;
  out[1] = ll;
  out[2] = 0.0f;
}

// ---- sweep ----
__device__ __forceinline__ float logadd(float x, float y) {
  const float m = fmaxf(x, y);
  const float r = m + __logf(1.0f + __expf(-fabsf(x - y)));
  return m > NEG_INF ? r : NEG_INF;  // (both -inf: the difference is NaN)
}
// lane l's value of lane l - 1 / of lane l + 1 (the wave's edge: -inf); every lane of the wave takes part
__device__ __forceinline__ float from_lower_lane(float v) {
  return __int_as_float(
      __builtin_amdgcn_update_dpp(__float_as_int(NEG_INF), __float_as_int(v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float from_upper_lane(float v) {
  return __int_as_float(
      __builtin_amdgcn_update_dpp(__float_as_int(NEG_INF), __float_as_int(v), 0x130, 0xf, 0xf, false));
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <int G>
__global__ __launch_bounds__(64) void transducer_pruned_sweep_kernel(Args a) {
  const int lane = static_cast<int>(threadIdx.x), s = lane & (G - 1);
  const int lb = static_cast<int>(blockIdx.x) * (64 / G) + lane / G;
  const bool backward = blockIdx.y == 1;
  const bool present = lb < a.count;  // (the last wave may carry fewer utterances)
  const int b = a.utt0 + (present ? lb : 0);
  const int S = a.S, U1 = a.U1;
  int Tb = present ? a.frames[b] : 0;
  const int Ub = a.tlen[b];
  const bool fits = Tb >= 1 && Tb <= a.T && Ub >= 0 && Ub < U1;
  if (!fits || s >= S) Tb = 0;  // (a lane without a frame to walk: it publishes -inf throughout)
  const int64_t base = static_cast<int64_t>(present ? lb : 0) * a.T;  // (frames before the utterance's, in the slice)
  const GTNX_G int* rng = a.ranges + static_cast<int64_t>(b) * a.T;
  const GTNX_G float* rows = a.rows + (base * S + s) * 3;

  int nr = 0;                        // the frame to do next: its r and, as loaded, its compact pair
  float nb = NEG_INF, nl = NEG_INF;  // (a node that is not live holds anything here: selected away before use)
  auto load = [&](int t) {
    if (t >= 0 && t < Tb) {
      nr = rng[t];
      const GTNX_G float* p = rows + static_cast<int64_t>(t) * S * 3;
      nb = p[0];
      nl = p[1];
    }
  };

  if (!backward) {
    GTNX_G float* plane = a.alpha ? a.alpha + base * S + s : nullptr;
    float keep = NEG_INF, carry = NEG_INF;  // alpha + lp_blank / alpha + lp_label of the node done last
    float fin = NEG_INF;
    bool bad = false;  // the ranges decrease
    int t = 0, pr = 0;
    load(0);
    for (int k = 0; __any(t < Tb); ++k) {
      float left = from_lower_lane(carry);
      if (s == 0) left = NEG_INF;
      const int rc = clampi(nr, 0, U1 - 1), d = rc - pr;
      const bool go = t < Tb && k >= t + rc + s;
      float up = __shfl(keep, lane + (go ? clampi(d, 0, G - 1 - s) : 0), 64);
      if (go) {
        const int u = nr >= 0 && nr < U1 ? nr + s : -1;  // (-1: a frame without a node)
        const bool live = u >= 0 && u <= Ub;
        if (t == 0) {
          up = u == 0 ? 0.0f : NEG_INF;  // (the start enters node (0, 0))
        } else {
          bad |= d < 0;
          if (d < 0 || s + d >= S) up = NEG_INF;  // (no node (t - 1, u) in the band)
        }
        const float cb = live ? nb : NEG_INF, cl = live && u < Ub ? nl : NEG_INF;
        const float al = live ? logadd(up, left) : NEG_INF;
        if (plane) plane[static_cast<int64_t>(t) * S] = al;
        keep = al + cb;
        carry = al + cl;
        if (t == Tb - 1 && u == Ub) fin = keep;
        pr = rc;
        ++t;
        load(t);
      }
    }
    // (one lane of the group at most holds the end; every walking lane saw every r_t, so `bad` is the group's)
    const bool any_bad = group_max<G>(bad ? 1.0f : 0.0f) > 0.0f;
    fin = group_max<G>(fin);
    if (present && s == 0) a.scores[b] = any_bad ? NEG_INF : fin;
  } else {
    GTNX_G float* plane = a.beta + base * S + s;
    float pub = NEG_INF;  // beta of the node done last
    int t = Tb - 1, pr = 0;
    const int R = Tb > 0 ? clampi(rng[Tb - 1], 0, U1 - 1) : 0;
    load(t);
    for (int k = 0; __any(t >= 0); ++k) {
      float right = from_upper_lane(pub);
      if (s == G - 1) right = NEG_INF;
      const int rc = clampi(nr, 0, U1 - 1), d = pr - rc;
      const bool go = t >= 0 && k >= (Tb - 1 - t) + (R - rc) + (S - 1 - s);
      float dn = __shfl(pub, lane - (go ? clampi(d, 0, s) : 0), 64);
      if (go) {
        const int u = nr >= 0 && nr < U1 ? nr + s : -1;  // (-1: a frame without a node)
        const bool live = u >= 0 && u <= Ub;
        if (t == Tb - 1) dn = u == Ub ? 0.0f : NEG_INF;  // (beta of the virtual end, below (T_b - 1, U_b))
        else if (d < 0 || s - d < 0) dn = NEG_INF;       // (no node (t + 1, u) in the band)
        const float cb = live ? nb : NEG_INF, cl = live && u < Ub ? nl : NEG_INF;
        const float be = live ? logadd(dn + cb, right + cl) : NEG_INF;
        plane[static_cast<int64_t>(t) * S] = be;
        pub = be;
        pr = rc;
        --t;
        load(t);
      }
    }
  }
}

// ---- gradient: a group of G lanes per band row of the slice, W floats per load and store ----
template <int G, int W>
__global__ __launch_bounds__(kWG) void transducer_pruned_grad_kernel(Args a) {
  const int tid = static_cast<int>(threadIdx.x), g = tid & (G - 1);
  const int64_t r64 = static_cast<int64_t>(blockIdx.x) * (kWG / G) + tid / G;
  if (r64 >= static_cast<int64_t>(a.count) * a.T * a.S) return;
  const int r = static_cast<int>(r64);
  Node n;
  const bool live = decode(a, r, n);
  float ob = 0.0f, ol = 0.0f, lse = 0.0f, w = 0.0f;
  int tok = -1;
  if (live) {
    const float sc = a.scores[n.b];
    if (sc > NEG_INF) {
      const GTNX_G float* p = a.rows + static_cast<int64_t>(r) * 3;
      const float al = a.alpha[r];
      float bb = n.u == n.Ub ? 0.0f : NEG_INF;
      if (n.t + 1 < n.Tb) {
        // (a finite score: the ranges are inside 0 .. U and do not decrease; the band position is checked all the same)
        const int sp = n.s - (a.ranges[static_cast<int64_t>(n.b) * a.T + n.t + 1] - n.rt);
        bb = sp >= 0 && sp <= n.s ? a.beta[static_cast<int64_t>(r) + (a.S - n.s) + sp] : NEG_INF;
      }
      const float bl = n.u < n.Ub && n.s + 1 < a.S ? a.beta[static_cast<int64_t>(r) + 1] : NEG_INF;
      // (every term is finite or -inf, so is the sum; the score is finite)
      ob = expf(al + p[0] + bb - sc);
      ol = expf(al + p[1] + bl - sc);
      lse = p[2];
      w = a.weights[n.b];
      tok = label_of(a, n);
    }
  }
  const float occ = ob + ol;
  const int64_t off = n.global * a.C;
  const GTNX_G float* row = a.x + off;
  GTNX_G float* out = a.grad + off;
  const int cnt = W == 4 ? a.C >> 2 : a.C;
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
  const bool norm = a.normalize != 0;
#pragma unroll 4
  for (int i = g; i < cnt; i += G) {
    float q[W];
    if (W == 4) {
      f4 t4 = {0.0f, 0.0f, 0.0f, 0.0f};
      if (norm) t4 = reinterpret_cast<const GTNX_G f4*>(row)[i];
      q[0] = t4.x;
      q[1 % W] = t4.y;
      q[2 % W] = t4.z;
      q[3 % W] = t4.w;
    } else {
      q[0] = norm ? row[i] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const int c = i * W + k;
      const float hit = (c == blank ? ob : 0.0f) + (c == tok ? ol : 0.0f);
      q[k] = w * (hit - (norm ? expf(q[k] - lse) * occ : 0.0f));
    }
    if (W == 4) {
      const f4 t4 = {q[0], q[1 % W], q[2 % W], q[3 % W]};
      reinterpret_cast<GTNX_G f4*>(out)[i] = t4;
    } else {
      out[i] = q[0];
    }
  }
}

// ---- occupancy of a full lattice: one lane per node of the slice, every element stored ----
__global__ __launch_bounds__(kWG) void transducer_occupancy_kernel(TransducerOccupancyArgs oa) {
  const TransducerArgs& a = oa.a;
  const int64_t r64 = static_cast<int64_t>(blockIdx.x) * kWG + threadIdx.x;
  const int per = a.T * a.U1;
  if (r64 >= static_cast<int64_t>(a.count) * per) return;
  const int r = static_cast<int>(r64);
  const int lb = r / per, rem = r - lb * per, b = a.utt0 + lb;
  const int t = rem / a.U1, u = rem - t * a.U1;
  const int Tb = a.frames[b], Ub = a.tlen[b];
  float v = 0.0f;
  if (Tb >= 1 && Tb <= a.T && Ub >= 0 && Ub < a.U1 && t < Tb && u <= Ub) {
    const float sc = a.scores[b];
    if (sc > NEG_INF) v = expf(a.alpha[r] + a.beta[r] - sc);  // (finite or -inf, never NaN)
  }
  oa.occ[static_cast<int64_t>(b) * per + rem] = v;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline unsigned blocks_for(const Args& a, int rows_per_block) {
  const int64_t total = static_cast<int64_t>(a.count) * a.T * a.S;
  return static_cast<unsigned>((total + rows_per_block - 1) / rows_per_block);
}

template <int G, int NV, int W>
void rows_launch(const Args& a, hipStream_t st) {
  hipLaunchKernelGGL((transducer_pruned_rows_kernel<G, NV, W>), dim3(blocks_for(a, kWG / G)), dim3(kWG), 0, st, a);
}
template <int G, int W>
void grad_launch(const Args& a, hipStream_t st) {
  hipLaunchKernelGGL((transducer_pruned_grad_kernel<G, W>), dim3(blocks_for(a, kWG / G)), dim3(kWG), 0, st, a);
}
template <int G>
void sweep_launch(const Args& a, hipStream_t st) {
  const unsigned waves = static_cast<unsigned>((a.count + 64 / G - 1) / (64 / G));
  hipLaunchKernelGGL(transducer_pruned_sweep_kernel<G>, dim3(waves, a.beta ? 2u : 1u), dim3(64), 0, st, a);
}

}  // namespace

void launch_transducer_pruned_rows(const TransducerPrunedArgs& a, hipStream_t st) {
  if (a.count <= 0) return;
  if (!a.normalize) {
    hipLaunchKernelGGL(transducer_pruned_gather_kernel, dim3(blocks_for(a, kWG)), dim3(kWG), 0, st, a);
  } else if ((a.C & 3) == 0 && aligned16(a.x)) {
    const int nvec = a.C >> 2;
    if (a.C > kRegRow)
      hipLaunchKernelGGL(transducer_pruned_rows_wide_kernel<4>, dim3(blocks_for(a, kWG / 64)), dim3(kWG), 0, st, a);
    else if (nvec <= 8) rows_launch<8, 1, 4>(a, st);
    else if (nvec <= 32) rows_launch<32, 1, 4>(a, st);
    else if (nvec <= 128) rows_launch<64, 2, 4>(a, st);
    else if (nvec <= 256) rows_launch<64, 4, 4>(a, st);
    else rows_launch<64, 16, 4>(a, st);
  } else {
    if (a.C > kRegRow)
      hipLaunchKernelGGL(transducer_pruned_rows_wide_kernel<1>, dim3(blocks_for(a, kWG / 64)), dim3(kWG), 0, st, a);
    else if (a.C <= 8) rows_launch<8, 1, 1>(a, st);
    else if (a.C <= 32) rows_launch<32, 1, 1>(a, st);
    else if (a.C <= 256) rows_launch<64, 4, 1>(a, st);
    else if (a.C <= 1024) rows_launch<64, 16, 1>(a, st);
    else rows_launch<64, 64, 1>(a, st);
  }
  HIP_CHECK(hipGetLastError());
}

void launch_transducer_pruned_sweep(const TransducerPrunedArgs& a, hipStream_t st) {
  if (a.count <= 0) return;
  if (a.S <= 8) sweep_launch<8>(a, st);
  else if (a.S <= 16) sweep_launch<16>(a, st);
  else if (a.S <= 32) sweep_launch<32>(a, st);
  else sweep_launch<64>(a, st);
  HIP_CHECK(hipGetLastError());
}

void launch_transducer_pruned_grad(const TransducerPrunedArgs& a, hipStream_t st) {
  if (a.count <= 0) return;
  if ((a.C & 3) == 0 && aligned16(a.x) && aligned16(a.grad)) {
    const int nvec = a.C >> 2;
    if (nvec <= 8) grad_launch<8, 4>(a, st);
    else if (nvec <= 32) grad_launch<32, 4>(a, st);
    else grad_launch<64, 4>(a, st);
  } else {
    if (a.C <= 8) grad_launch<8, 1>(a, st);
    else if (a.C <= 32) grad_launch<32, 1>(a, st);
    else grad_launch<64, 1>(a, st);
  }
  HIP_CHECK(hipGetLastError());
}

void launch_transducer_occupancy(const TransducerOccupancyArgs& oa, hipStream_t st) {
  const TransducerArgs& a = oa.a;
  if (a.count <= 0) return;
  const int64_t total = static_cast<int64_t>(a.count) * a.T * a.U1;
  hipLaunchKernelGGL(transducer_occupancy_kernel, dim3(static_cast<unsigned>((total + kWG - 1) / kWG)), dim3(kWG), 0, st,
                     oa);
  HIP_CHECK(hipGetLastError());
}

}  // namespace gtnx
