// transducer16.hip -- the rows and gradient passes of the transducer (RNN-T) score over bfloat16 / float16 joint logits,
// for the full lattice x [B][T][U+1][C] and for the band x [B][T][S][C] (DESIGN section 45 holds the contract, on top of
// sections 42 and 44).  Only the logits and the gradient are 16-bit: an element is converted exactly to float32, all
// arithmetic is float32, and the compact plane (lp_blank, lp_label, lse), alpha, beta, the scores and the weights are the
// float32 planes of transducer.hip / transducer_pruned.hip, whose sweeps run between the two passes unchanged.
//
//   rows16: the forward's only pass over the logits.  A row of C labels is C / 8 vectors of 16 bytes, half as many as in
//           float32, so a group of G lanes takes one live row with G = 4 up to 32 labels (16 rows per wave), 16 up to 128,
//           64 above; every lane holds NV vectors = 8 NV labels in float32 registers (NV = 1 up to 512 labels, 2 up to
//           1024, 4 up to 2048, 8 up to 4096), takes the maximum and the sum of exp over them and one lane of the group
//           stores the triple.  Rows above kRegRow = 4096 labels run an online maximum / sum loop, one wave per row.  The
//           pairs of a 32-bit word are unpacked together: bfloat16 by a shift and a mask, float16 by a packed convert, so
//           float16's own inf and NaN arrive as inf and NaN.  16-byte loads need C % 8 == 0 and a 16-byte aligned base;
//           anything else (a base that is only 2-byte aligned included) takes the same instantiations with 2-byte loads.
//           Unnormalised: one lane per node gathers the two entries and reads nothing else.
//   grad16: per row of the slice it reads the node's alpha, the two betas, the triple and the score exactly as the
//           float32 gradient kernels do, streams the 16-bit row once, forms w ([c == blank] occ_b + [c == y[u]] occ_l -
//           exp(x - lse) (occ_b + occ_l)) in float32, rounds it once to nearest even into the logits' type and stores
//           16-byte vectors of 8 (2-byte elements on the narrow path).  Rows that are never read, rows of an utterance
//           that scores -inf, dead rows and nodes nothing passes through are stored as +0 bits without a load.  Every
//           row of the output is stored exactly once.
//   decode: both kernels take the node decode as a policy: Full maps the row index to (b, t, u); Band maps it to
//           (b, t, s) with u = ranges[b][t] + s and transducer_pruned.hip's liveness rule.  One body serves both tensors.
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
constexpr int kRegRow = 4096;  // the widest row the rows kernel holds in registers: 8 vectors of 8 labels per lane
typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef float f2 __attribute__((ext_vector_type(2)));
using Args = Transducer16Args;
using Elem = uint16_t;

// ---- the two element types: exact widening, one rounding to nearest even ----
template <bool BF>
__device__ __forceinline__ float widen(Elem h) {
  if (BF) return __uint_as_float(static_cast<uint32_t>(h) << 16);
  return static_cast<float>(__builtin_bit_cast(_Float16, h));
}
// the two elements of a 32-bit word, the lower address first
template <bool BF>
__device__ __forceinline__ void widen2(uint32_t w, float& lo, float& hi) {
  if (BF) {
    lo = __uint_as_float(w << 16);
    hi = __uint_as_float(w & 0xffff0000u);
  } else {
    const f2 p = __builtin_convertvector(__builtin_bit_cast(h2, w), f2);
    lo = p.x;
    hi = p.y;
  }
}
template <bool BF>
__device__ __forceinline__ void widen8(const u4& q, float* v) {
  widen2<BF>(q.x, v[0], v[1]);
  widen2<BF>(q.y, v[2], v[3]);
  widen2<BF>(q.z, v[4], v[5]);
  widen2<BF>(q.w, v[6], v[7]);
}
template <bool BF>
__device__ __forceinline__ uint32_t narrow(float f) {
  if (BF) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;  // (NaN stays NaN; the gradient has none)
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
  }
  return __builtin_bit_cast(Elem, static_cast<_Float16>(f));
}
template <bool BF>
__device__ __forceinline__ uint32_t narrow2(float lo, float hi) {
  if (BF) return narrow<true>(lo) | (narrow<true>(hi) << 16);
  const f2 p = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(p, h2));
}

// ---- the node decode: row r of the slice -> the node, T_b, U_b; true for a live node ----
struct Node {
  int b, t, s, u, rt, Tb, Ub;  // s: the position inside the frame (Full: u); rt: the band start (Full: 0)
  int64_t global;              // the row's index in the whole batch
};
__device__ __forceinline__ void split(const Args& a, int r, Node& n) {
  const int per = a.T * a.W;
  const int lb = r / per, rem = r - lb * per;
  n.b = a.utt0 + lb;
  n.t = rem / a.W;
  n.s = rem - n.t * a.W;
  n.global = static_cast<int64_t>(n.b) * per + rem;
  n.Tb = a.frames[n.b];
  n.Ub = a.tlen[n.b];
}
struct Full {  // x [B][T][U1][C], W == U1
  static __device__ __forceinline__ bool node(const Args& a, int r, Node& n) {
    split(a, r, n);
    n.u = n.s;
    n.rt = 0;
    return n.Tb >= 1 && n.Tb <= a.T && n.Ub >= 0 && n.Ub < a.U1 && n.t < n.Tb && n.u <= n.Ub;
  }
  // beta[t + 1, u] and beta[t, u + 1] of a live node (beyond the lattice: the virtual end, or -inf)
  static __device__ __forceinline__ void betas(const Args& a, int r, const Node& n, float& bb, float& bl) {
    bb = n.t + 1 < n.Tb ? a.beta[static_cast<int64_t>(r) + a.U1] : (n.u == n.Ub ? 0.0f : NEG_INF);
    bl = n.u < n.Ub ? a.beta[static_cast<int64_t>(r) + 1] : NEG_INF;
  }
};
struct Band {  // x [B][T][S][C], W == S, u = ranges[b][t] + s
  static __device__ __forceinline__ bool node(const Args& a, int r, Node& n) {
    split(a, r, n);
    n.rt = n.u = -1;
    if (!(n.Tb >= 1 && n.Tb <= a.T && n.Ub >= 0 && n.Ub < a.U1 && n.t < n.Tb)) return false;
    n.rt = a.ranges[static_cast<int64_t>(n.b) * a.T + n.t];
    if (n.rt < 0 || n.rt >= a.U1) return false;  // (a frame without a node; r_t + s cannot overflow below)
    n.u = n.rt + n.s;
    return n.u <= n.Ub;
  }
  static __device__ __forceinline__ void betas(const Args& a, int r, const Node& n, float& bb, float& bl) {
    bb = n.u == n.Ub ? 0.0f : NEG_INF;
    if (n.t + 1 < n.Tb) {
      // (a finite score: the ranges are inside 0 .. U and do not decrease; the band position is checked all the same)
      const int sp = n.s - (a.ranges[static_cast<int64_t>(n.b) * a.T + n.t + 1] - n.rt);
      bb = sp >= 0 && sp <= n.s ? a.beta[static_cast<int64_t>(r) + (a.W - n.s) + sp] : NEG_INF;
    }
    bl = n.u < n.Ub && n.s + 1 < a.W ? a.beta[static_cast<int64_t>(r) + 1] : NEG_INF;
  }
};

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
template <bool BF>
__device__ __forceinline__ void store_triple(const Args& a, int r, const Node& n, const GTNX_G Elem* row, float lse) {
  GTNX_G float* out = a.rows + static_cast<int64_t>(r) * 3;
  if (!(fabsf(lse) < POS_INF)) {  // NaN or +inf in the row, or nothing but -inf
    out[0] = NEG_INF;
    out[1] = NEG_INF;
    out[2] = 0.0f;
    return;
  }
  const int tok = label_of(a, n);
  out[0] = widen<BF>(row[a.blank]) - lse;
  out[1] = tok >= 0 ? widen<BF>(row[tok]) - lse : NEG_INF;
  out[2] = lse;
}

// ---- rows16, C <= 4096: a group of G lanes holds a row as 8 NV floats per lane ----
// VEC: lane g loads the 16-byte vectors g, g + G, ...; else the 2-byte elements g, g + G, ... (8 NV of them)
template <class D, bool BF, int G, int NV, bool VEC>
__global__ __launch_bounds__(kWG) void transducer16_rows_kernel(Args a) {
  const int tid = static_cast<int>(threadIdx.x), g = tid & (G - 1);
  const int64_t r64 = static_cast<int64_t>(blockIdx.x) * (kWG / G) + tid / G;
  if (r64 >= static_cast<int64_t>(a.count) * a.T * a.W) return;
  const int r = static_cast<int>(r64);
  Node n;
  if (!D::node(a, r, n)) return;  // (a whole group leaves together)
  const GTNX_G Elem* row = static_cast<const GTNX_G Elem*>(a.x) + n.global * a.C;
  float v[NV * 8];
  if (VEC) {
    const GTNX_G u4* rowv = reinterpret_cast<const GTNX_G u4*>(row);
    const int nvec = a.C >> 3;
    constexpr uint32_t kPad = BF ? 0xff80ff80u : 0xfc00fc00u;  // two -inf
    u4 q[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {  // (every load is issued before the first conversion)
      const int i = j * G + g;
      q[j] = u4{kPad, kPad, kPad, kPad};
      if (i < nvec) q[j] = rowv[i];
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) widen8<BF>(q[j], v + 8 * j);
  } else {
#pragma unroll
    for (int j = 0; j < NV * 8; ++j) {
      const int i = j * G + g;
      v[j] = i < a.C ? widen<BF>(row[i]) : NEG_INF;
    }
  }
  float m = NEG_INF;
#pragma unroll
  for (int j = 0; j < NV * 8; ++j) m = fmaxf(m, v[j]);
  m = group_max<G>(m);
  // (a NaN entry passes fmaxf and makes the sum NaN; +inf and an all -inf row give inf - inf: the lse tells)
  float sum = 0.0f;
#pragma unroll
  for (int j = 0; j < NV * 8; ++j) sum += expf(v[j] - m);
  sum = group_sum<G>(sum);
  if (g == 0) store_triple<BF>(a, r, n, row, m + logf(sum));
}

// ---- rows16, C > 4096: one wave per row, an online maximum / sum per lane, then one combine ----
template <class D, bool BF, bool VEC>
__global__ __launch_bounds__(kWG) void transducer16_rows_wide_kernel(Args a) {
  constexpr int W = VEC ? 8 : 1;
  const int tid = static_cast<int>(threadIdx.x), g = tid & 63;
  const int64_t r64 = static_cast<int64_t>(blockIdx.x) * (kWG / 64) + tid / 64;
  if (r64 >= static_cast<int64_t>(a.count) * a.T * a.W) return;
  const int r = static_cast<int>(r64);
  Node n;
  if (!D::node(a, r, n)) return;
  const GTNX_G Elem* row = static_cast<const GTNX_G Elem*>(a.x) + n.global * a.C;
  float m = NEG_INF, sum = 0.0f;
  bool bad = false;  // NaN or +inf seen
  const int cnt = VEC ? a.C >> 3 : a.C;
  for (int i = g; i < cnt; i += 64) {
    float q[8];
    if (VEC) widen8<BF>(reinterpret_cast<const GTNX_G u4*>(row)[i], q);
    else q[0] = widen<BF>(row[i]);
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
  if (g == 0) store_triple<BF>(a, r, n, row, any_bad ? POS_INF : M + logf(S));
}

// ---- rows16, unnormalised: the two entries of a node, nothing else is read ----
template <class D, bool BF>
__global__ __launch_bounds__(kWG) void transducer16_gather_kernel(Args a) {
  const int64_t r64 = static_cast<int64_t>(blockIdx.x) * kWG + threadIdx.x;
  if (r64 >= static_cast<int64_t>(a.count) * a.T * a.W) return;
  const int r = static_cast<int>(r64);
  Node n;
  if (!D::node(a, r, n)) return;
  const GTNX_G Elem* row = static_cast<const GTNX_G Elem*>(a.x) + n.global * a.C;
  const int tok = label_of(a, n);
  float lb = widen<BF>(row[a.blank]), ll = tok >= 0 ? widen<BF>(row[tok]) : NEG_INF;
  if (!(lb < POS_INF) || !(ll < POS_INF)) lb = ll = NEG_INF;  // (NaN or +inf: a node no path leaves)
  GTNX_G float* out = a.rows + static_cast<int64_t>(r) * 3;
  out[0] = lb;
  out[1] = ll;
  out[2] = 0.0f;
}

// ---- grad16: a group of G lanes per row of the slice; 8 elements (VEC) or 1 per load and store ----
template <class D, bool BF, int G, bool VEC>
__global__ __launch_bounds__(kWG) void transducer16_grad_kernel(Args a) {
  const int tid = static_cast<int>(threadIdx.x), g = tid & (G - 1);
  const int64_t r64 = static_cast<int64_t>(blockIdx.x) * (kWG / G) + tid / G;
  if (r64 >= static_cast<int64_t>(a.count) * a.T * a.W) return;
  const int r = static_cast<int>(r64);
  Node n;
  const bool live = D::node(a, r, n);
  float ob = 0.0f, ol = 0.0f, lse = 0.0f, w = 0.0f;
  int tok = -1;
  if (live) {
    const float sc = a.scores[n.b];
    if (sc > NEG_INF) {
      const GTNX_G float* p = a.rows + static_cast<int64_t>(r) * 3;
      const float al = a.alpha[r];
      float bb, bl;
      D::betas(a, r, n, bb, bl);
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
  const GTNX_G Elem* row = static_cast<const GTNX_G Elem*>(a.x) + off;
  GTNX_G Elem* out = static_cast<GTNX_G Elem*>(a.grad) + off;
  const int cnt = VEC ? a.C >> 3 : a.C;
  const int blank = a.blank;
  if (!(occ > 0.0f)) {  // never read, a -inf score, a dead row, or a node nothing passes through
    if (VEC) {
      const u4 z = {0u, 0u, 0u, 0u};
      for (int i = g; i < cnt; i += G) reinterpret_cast<GTNX_G u4*>(out)[i] = z;
    } else {
      for (int i = g; i < cnt; i += G) out[i] = Elem(0);
    }
    return;
  }
  const bool norm = a.normalize != 0;
  auto value = [&](int c, float x) {
    const float hit = (c == blank ? ob : 0.0f) + (c == tok ? ol : 0.0f);
    return w * (hit - (norm ? expf(x - lse) * occ : 0.0f));
  };
  if (VEC) {
#pragma unroll 2
    for (int i = g; i < cnt; i += G) {
      float q[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      if (norm) widen8<BF>(reinterpret_cast<const GTNX_G u4*>(row)[i], q);
#pragma unroll
      for (int k = 0; k < 8; ++k) q[k] = value(i * 8 + k, q[k]);
      const u4 o = {narrow2<BF>(q[0], q[1]), narrow2<BF>(q[2], q[3]), narrow2<BF>(q[4], q[5]), narrow2<BF>(q[6], q[7])};
      reinterpret_cast<GTNX_G u4*>(out)[i] = o;
    }
  } else {
#pragma unroll 4
    for (int i = g; i < cnt; i += G) out[i] = static_cast<Elem>(narrow<BF>(value(i, norm ? widen<BF>(row[i]) : 0.0f)));
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline unsigned blocks_for(const Args& a, int rows_per_block) {
  const int64_t total = static_cast<int64_t>(a.count) * a.T * a.W;
  return static_cast<unsigned>((total + rows_per_block - 1) / rows_per_block);
}

template <class D, bool BF, int G, int NV, bool VEC>
void rows_launch(const Args& a, hipStream_t st) {
  hipLaunchKernelGGL((transducer16_rows_kernel<D, BF, G, NV, VEC>), dim3(blocks_for(a, kWG / G)), dim3(kWG), 0, st, a);
}
template <class D, bool BF, int G, bool VEC>
void grad_launch(const Args& a, hipStream_t st) {
  hipLaunchKernelGGL((transducer16_grad_kernel<D, BF, G, VEC>), dim3(blocks_for(a, kWG / G)), dim3(kWG), 0, st, a);
}

// the rows16 table: labels per row -> (G, NV), the same on the 16-byte and on the 2-byte path
template <class D, bool BF, bool VEC>
void rows_table(const Args& a, hipStream_t st) {
  if (a.C > kRegRow)
    hipLaunchKernelGGL((transducer16_rows_wide_kernel<D, BF, VEC>), dim3(blocks_for(a, kWG / 64)), dim3(kWG), 0, st, a);
  else if (a.C <= 32) rows_launch<D, BF, 4, 1, VEC>(a, st);
  else if (a.C <= 128) rows_launch<D, BF, 16, 1, VEC>(a, st);
  else if (a.C <= 512) rows_launch<D, BF, 64, 1, VEC>(a, st);
  else if (a.C <= 1024) rows_launch<D, BF, 64, 2, VEC>(a, st);
  else if (a.C <= 2048) rows_launch<D, BF, 64, 4, VEC>(a, st);
  else rows_launch<D, BF, 64, 8, VEC>(a, st);
}
template <class D, bool BF>
void rows_dispatch(const Args& a, hipStream_t st) {
  if (!a.normalize)
    hipLaunchKernelGGL((transducer16_gather_kernel<D, BF>), dim3(blocks_for(a, kWG)), dim3(kWG), 0, st, a);
  else if ((a.C & 7) == 0 && aligned16(a.x)) rows_table<D, BF, true>(a, st);
  else rows_table<D, BF, false>(a, st);
}
// the grad16 table: 16-byte path G = 4 up to 32 labels, 16 up to 128, 64 above; 2-byte path G = 16 up to 32, 64 above
template <class D, bool BF>
void grad_dispatch(const Args& a, hipStream_t st) {
  if ((a.C & 7) == 0 && aligned16(a.x) && aligned16(a.grad)) {
    if (a.C <= 32) grad_launch<D, BF, 4, true>(a, st);
    else if (a.C <= 128) grad_launch<D, BF, 16, true>(a, st);
    else grad_launch<D, BF, 64, true>(a, st);
  } else {
    if (a.C <= 32) grad_launch<D, BF, 16, false>(a, st);
    else grad_launch<D, BF, 64, false>(a, st);
  }
}

}  // namespace

void launch_transducer16_rows(const Transducer16Args& a, hipStream_t st) {
  if (a.count <= 0) return;
  if (a.ranges) a.bf16 ? rows_dispatch<Band, true>(a, st) : rows_dispatch<Band, false>(a, st);
  else a.bf16 ? rows_dispatch<Full, true>(a, st) : rows_dispatch<Full, false>(a, st);
  HIP_CHECK(hipGetLastError());
}

void launch_transducer16_grad(const Transducer16Args& a, hipStream_t st) {
  if (a.count <= 0) return;
  if (a.ranges) a.bf16 ? grad_dispatch<Band, true>(a, st) : grad_dispatch<Band, false>(a, st);
  else a.bf16 ? grad_dispatch<Full, true>(a, st) : grad_dispatch<Full, false>(a, st);
  HIP_CHECK(hipGetLastError());
}

}  // namespace gtnx
