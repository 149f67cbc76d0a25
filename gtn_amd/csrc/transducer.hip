// transducer.hip -- the transducer (RNN-T) log score of a padded batch over device-resident joint logits x [B][T][U+1][C]
// and its gradient under caller-supplied weights (DESIGN section 42 holds the contract; tests/transducer_fp.py has the
// recurrences in float64).  Node (b, t, u) is live when t < T_b and u <= U_b; T_b and U_b are read on the device and an
// utterance whose counts do not fit the tensor has no live node and scores -inf.
//
//   rows:   the forward's only pass over the logits.  A group of G lanes (8, 32 or 64: narrow rows share a wave) takes
//           one live row, holds it in registers (NV loads of 16 bytes per lane when C % 4 == 0 and the tensor is 16-byte
//           aligned, else of 4 bytes), takes the maximum and the sum of exp over the registers and stores the compact
//           triple (lp_blank, lp_label, lse), 12 bytes per node.  Rows above 4096 labels run an online maximum / sum
//           loop, one wave per row.  A row with NaN or +inf, or nothing but -inf, stores (-inf, -inf, 0): a node no path
//           leaves.  A token outside 0 .. C-1 or equal to blank stores lp_label = -inf, which closes column u for every
//           frame, so the utterance scores -inf without a check of its own.  Unnormalised: one lane per node gathers the
//           two entries and reads nothing else.
//   sweep:  one wave per utterance and direction, no LDS and no barrier.  Lane l owns the K = ceil((U+1)/64) (rounded up
//           to 1, 2, 4, 8, 16) columns u0 = l K .. u0 + K - 1 in registers.  The walk is skewed: at step s lane l
//           advances row t = s - l (alpha; beta mirrors both axes), takes alpha[t, u0 - 1] + lp_label[t, u0 - 1] from lane
//           l - 1's previous step through a DPP wave shift, and has loaded the compact values of its next row before it
//           computes the current one.  T_b + U_b / K steps of K serial logadds each; alpha and beta go to planes, the score
//           is written by the alpha wave.
//   grad:   the rows kernel's twin without the reductions: per row of the slice it reads the node's alpha, beta[t+1, u],
//           beta[t, u+1], the compact triple and the score, then streams the logits row once and stores
//           w ([c == blank] occ_b + [c == y[u]] occ_l - exp(x - lse) (occ_b + occ_l)) with the same widths.  Rows that
//           are never read, rows of an utterance that scores -inf and rows nothing passes through are stored as zeros
//           without a load.  Every row of the output is stored exactly once.
// Every store is a plain C++ store; there are no atomics and no inline assembly, and no workgroup waits on another.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "kernels.h"

namespace gtnx {
namespace {

constexpr float NEG_INF = -__builtin_inff();
constexpr float POS_INF = __builtin_inff();
constexpr int kWG = 256;         // the streaming kernels' workgroup
constexpr int kRegRow = 4096;    // the widest row the rows kernel holds in registers
typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// row r of the slice -> (b, t, u), T_b, U_b; true for a live node
struct Node {
  int b, t, u, Tb, Ub, global;  // global: the node's index in the whole batch
};
__device__ __forceinline__ bool decode(const TransducerArgs& a, int r, Node& n) {
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
__device__ __forceinline__ int label_of(const TransducerArgs& a, const Node& n) {
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
__device__ __forceinline__ void store_triple(const TransducerArgs& a, int r, const Node& n, const GTNX_G float* row,
                                             float lse) {
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
__global__ __launch_bounds__(kWG) void transducer_rows_kernel(TransducerArgs a) {
  const int tid = static_cast<int>(threadIdx.x), g = tid & (G - 1);
  const int64_t r64 = static_cast<int64_t>(blockIdx.x) * (kWG / G) + tid / G;
  if (r64 >= static_cast<int64_t>(a.count) * a.T * a.U1) return;
  const int r = static_cast<int>(r64);
  Node n;
  if (!decode(a, r, n)) return;  // (a whole group leaves together)
  const GTNX_G float* row = a.x + static_cast<int64_t>(n.global) * a.C;
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
  float s = 0.0f;
#pragma unroll
  for (int j = 0; j < NV * W; ++j) s += expf(v[j] - m);
  s = group_sum<G>(s);
  if (g == 0) store_triple(a, r, n, row, m + logf(s));
}

// ---- rows, C > 4096: one wave per row, an online maximum / sum per lane, then one combine ----
template <int W>
__global__ __launch_bounds__(kWG) void transducer_rows_wide_kernel(TransducerArgs a) {
  const int tid = static_cast<int>(threadIdx.x), g = tid & 63;
  const int64_t r64 = static_cast<int64_t>(blockIdx.x) * (kWG / 64) + tid / 64;
  if (r64 >= static_cast<int64_t>(a.count) * a.T * a.U1) return;
  const int r = static_cast<int>(r64);
  Node n;
  if (!decode(a, r, n)) return;
  const GTNX_G float* row = a.x + static_cast<int64_t>(n.global) * a.C;
  float m = NEG_INF, s = 0.0f;
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
      s = s * expf(m - cm) + add;  // (m == -inf: s is 0 and stays 0)
      m = cm;
    }
  }
  const float M = group_max<64>(m);
  const float S = group_sum<64>(m > NEG_INF ? s * expf(m - M) : 0.0f);
  const bool any_bad = __any(bad);
  if (g == 0) store_triple(a, r, n, row, any_bad ? POS_INF : M + logf(S));
}

// ---- rows, unnormalised: the two entries of a node, nothing else is read ----
__global__ __launch_bounds__(kWG) void transducer_gather_kernel(TransducerArgs a) {
  const int64_t r64 = static_cast<int64_t>(blockIdx.x) * kWG + threadIdx.x;
  if (r64 >= static_cast<int64_t>(a.count) * a.T * a.U1) return;
  const int r = static_cast<int>(r64);
  Node n;
  if (!decode(a, r, n)) return;
  const GTNX_G float* row = a.x + static_cast<int64_t>(n.global) * a.C;
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
// lane l's value of lane l - 1 (lane 0: `edge`) / of lane l + 1 (lane 63: `edge`); every lane of the wave takes part
__device__ __forceinline__ float from_lower_lane(float v, float edge) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float from_upper_lane(float v, float edge) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x130, 0xf, 0xf, false));
}

template <int K>
__global__ __launch_bounds__(64) void transducer_sweep_kernel(TransducerArgs a) {
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
  const GTNX_G float* rows = a.rows + base * 3;
  const int u0 = lane * K;
  const int lmax = Ub / K, kend = Ub - lmax * K;  // the lane and the register that own column U_b
  const int steps = Tb + lmax;
  const bool mine = lane <= lmax;

  float keep[K];  // alpha[t-1, u] + lp_blank[t-1, u] (alpha) / beta[t+1, u] (beta) of the row done last
  float nb[K], nl[K];  // the compact values of the row to do next
#pragma unroll
  for (int k = 0; k < K; ++k) keep[k] = NEG_INF;

  // (t outside 0 .. T_b - 1 and u > U_b load nothing: -inf)
  auto load = [&](int t, float* pb, float* pl) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      pb[k] = NEG_INF;
      pl[k] = NEG_INF;
      if (t >= 0 && t < Tb && u0 + k <= Ub) {
        const GTNX_G float* p = rows + (static_cast<int64_t>(t) * U1 + u0 + k) * 3;
        pb[k] = p[0];
        pl[k] = p[1];
      }
    }
  };

  float carry = NEG_INF;
  if (!backward) {
    if (lane == 0) keep[0] = 0.0f;  // (the start enters node (0, 0))
    GTNX_G float* plane = a.alpha ? a.alpha + base : nullptr;
    load(-lane, nb, nl);
    for (int s = 0; s < steps; ++s) {
      const int t = s - lane;
      float cb[K], cl[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        cb[k] = nb[k];
        cl[k] = nl[k];
      }
      load(t + 1, nb, nl);
      float left = from_lower_lane(carry, NEG_INF);
      if (mine && t >= 0 && t < Tb) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float al = logadd(keep[k], left);
          if (plane && u0 + k <= Ub) plane[static_cast<int64_t>(t) * U1 + u0 + k] = al;
          keep[k] = al + cb[k];
          left = al + cl[k];
        }
        carry = left;
      }
    }
    if (lane == lmax) {
      float sc = NEG_INF;
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (k == kend) sc = keep[k];
      a.scores[b] = sc;
    }
  } else {
    if (lane == lmax) {
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (k == kend) keep[k] = 0.0f;  // (beta of the virtual end, below (T_b - 1, U_b))
    }
    GTNX_G float* plane = a.beta + base;
    load(Tb - 1 + (lmax - lane), nb, nl);
    for (int s = 0; s < steps; ++s) {
      const int t = Tb - 1 - (s - (lmax - lane));
      float cb[K], cl[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        cb[k] = nb[k];
        cl[k] = nl[k];
      }
      load(t - 1, nb, nl);
      float right = from_upper_lane(carry, NEG_INF);
      if (mine && t >= 0 && t < Tb) {
#pragma unroll
        for (int k = K - 1; k >= 0; --k) {
          const float be = logadd(keep[k] + cb[k], right + cl[k]);
          if (u0 + k <= Ub) plane[static_cast<int64_t>(t) * U1 + u0 + k] = be;
          keep[k] = be;
          right = be;
        }
        carry = right;
      }
    }
  }
}

// ---- gradient: a group of G lanes per row of the slice, W floats per load and store ----
template <int G, int W>
__global__ __launch_bounds__(kWG) void transducer_grad_kernel(TransducerArgs a) {
  const int tid = static_cast<int>(threadIdx.x), g = tid & (G - 1);
  const int64_t r64 = static_cast<int64_t>(blockIdx.x) * (kWG / G) + tid / G;
  if (r64 >= static_cast<int64_t>(a.count) * a.T * a.U1) return;
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
      const float bb = n.t + 1 < n.Tb ? a.beta[static_cast<int64_t>(r) + a.U1] : (n.u == n.Ub ? 0.0f : NEG_INF);
      const float bl = n.u < n.Ub ? a.beta[static_cast<int64_t>(r) + 1] : NEG_INF;
      // (every term is finite or -inf, so is the sum; the score is finite)
      ob = expf(al + p[0] + bb - sc);
      ol = expf(al + p[1] + bl - sc);
      lse = p[2];
      w = a.weights[n.b];
      tok = label_of(a, n);
    }
  }
  const float occ = ob + ol;
  const int64_t off = static_cast<int64_t>(n.global) * a.C;
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

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline unsigned blocks_for(const TransducerArgs& a, int rows_per_block) {
  const int64_t total = static_cast<int64_t>(a.count) * a.T * a.U1;
  return static_cast<unsigned>((total + rows_per_block - 1) / rows_per_block);
}

template <int G, int NV, int W>
void rows_launch(const TransducerArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((transducer_rows_kernel<G, NV, W>), dim3(blocks_for(a, kWG / G)), dim3(kWG), 0, st, a);
}
template <int G, int W>
void grad_launch(const TransducerArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((transducer_grad_kernel<G, W>), dim3(blocks_for(a, kWG / G)), dim3(kWG), 0, st, a);
}
template <int K>
void sweep_launch(const TransducerArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(transducer_sweep_kernel<K>, dim3(unsigned(a.count), a.beta ? 2u : 1u), dim3(64), 0, st, a);
}

}  // namespace

void launch_transducer_rows(const TransducerArgs& a, hipStream_t st) {
  if (a.count <= 0) return;
  if (!a.normalize) {
    hipLaunchKernelGGL(transducer_gather_kernel, dim3(blocks_for(a, kWG)), dim3(kWG), 0, st, a);
  } else if ((a.C & 3) == 0 && aligned16(a.x)) {
    const int nvec = a.C >> 2;
    if (a.C > kRegRow) hipLaunchKernelGGL(transducer_rows_wide_kernel<4>, dim3(blocks_for(a, kWG / 64)), dim3(kWG), 0, st, a);
    else if (nvec <= 8) rows_launch<8, 1, 4>(a, st);
    else if (nvec <= 32) rows_launch<32, 1, 4>(a, st);
    else if (nvec <= 128) rows_launch<64, 2, 4>(a, st);
    else if (nvec <= 256) rows_launch<64, 4, 4>(a, st);
    else rows_launch<64, 16, 4>(a, st);
  } else {
    if (a.C > kRegRow) hipLaunchKernelGGL(transducer_rows_wide_kernel<1>, dim3(blocks_for(a, kWG / 64)), dim3(kWG), 0, st, a);
    else if (a.C <= 8) rows_launch<8, 1, 1>(a, st);
    else if (a.C <= 32) rows_launch<32, 1, 1>(a, st);
    else if (a.C <= 256) rows_launch<64, 4, 1>(a, st);
    else if (a.C <= 1024) rows_launch<64, 16, 1>(a, st);
    else rows_launch<64, 64, 1>(a, st);
  }
  HIP_CHECK(hipGetLastError());
}

void launch_transducer_sweep(const TransducerArgs& a, hipStream_t st) {
  if (a.count <= 0) return;
  const int k = (a.U1 + 63) / 64;
  if (k <= 1) sweep_launch<1>(a, st);
  else if (k <= 2) sweep_launch<2>(a, st);
  else if (k <= 4) sweep_launch<4>(a, st);
  else if (k <= 8) sweep_launch<8>(a, st);
  else sweep_launch<16>(a, st);
  HIP_CHECK(hipGetLastError());
}

void launch_transducer_grad(const TransducerArgs& a, hipStream_t st) {
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

}  // namespace gtnx
