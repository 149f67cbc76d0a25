// asg_full.hip -- forwardScore(emissions_b o asgTransitions) and its gradient for a padded batch, every utterance at
// its OWN length, in one launch each way (SURVEY.md section 8 config C4 at letter-sized alphabets).
//
// The dense regime of lazy.hip steps all utterances of a group through a shared T, one launch per frame: a batch with
// B distinct lengths is B chains of launches.  Here ONE workgroup walks ONE utterance's T_b frames, the transitions
// stay on chip, and frame counts cost nothing: rows >= T_b of a slab are never addressed.
//
//   alpha_1[i] = start[i] + em_1[i];  alpha_t[i] = em_t[i] + logsumexp_j(W[i][j] + alpha_{t-1}[j]);
//   score = logsumexp_i alpha_T[i]                                       (tests/ctc_fp64.py: asg_fp64)
//
// Layout.  N <= 2 * JH labels, 4 * JH threads (JH = 16 / 32 / 64): thread = (row r = tid / 2, half h = tid % 2) holds
// JH entries of row r of a matrix in REGISTERS -- forward E[r][j] = exp(W[r][j] - rowmax_r) for j in its half, backward
// the same matrix transposed (E[i][r] for i in its half) plus the lane's tile of the xi accumulator.  The vector the
// matrix is applied to sits in LDS and is read as a broadcast (two addresses per wave instruction); the two halves of
// a row meet by one cross-lane add.
//
// Scaling.  Step t keeps q_t[i] = exp(alpha_t[i] - L_t) with L_t = sum of the per-step maxima, accumulated in float64:
// one log and one exp per row and step, one workgroup maximum, two barriers.  A term more than ~87 below its step's
// maximum is dropped (float32 exp), which is below the float32 resolution of the sum it would have entered -- unless
// the terms ABOVE it are all forbidden (-inf) transitions: an alphabet whose only live continuation is that far down
// loses it.  -inf entries are probability 0 throughout; an utterance without a finite path has score -inf and a
// gradient of zeros (the backward kernel stores them, it never forms 0 * inf).
//
// Backward.  beta runs in the same scaled form (bq, LB); gamma_t[i] = exp(la_t[i] + log bq_t[i] + L_t + LB_t - Z) goes
// straight into row t of the emission gradient (rows < T_b only), gamma_1 into the start arcs, and
//   xi_t[i][j] = exp(alpha_{t-1}[j] + mf_t + LB_t - Z) * f_t[i] * E[i][j]      (f_t: the scaled em_t + rowmax + beta_t)
// is accumulated as X[i] += c_j * f_t[i] per lane and multiplied by E once at the end.  Every utterance writes its own
// [N + N*N] slice of a partials buffer; asg_full_reduce_kernel adds the slices in utterance order -- no float atomics,
// the same bits run after run.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace gtnx {
namespace {

constexpr float NEG_INF = -__builtin_inff();
constexpr int kAsgFullMaxLabels = 128;

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x = fmaxf(x, __shfl_xor(x, o));
  return x;
}
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o);
  return x;
}
// the maximum / sum over the workgroup in every lane; `slots` [4] is free again after the caller's next barrier
template <int NW, bool MAX>
__device__ __forceinline__ float block_reduce(float x, float* slots) {
  x = MAX ? wave_max(x) : wave_sum(x);
  if (NW == 1) return x;
  if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = x;
  __syncthreads();
  float m = slots[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) m = MAX ? fmaxf(m, slots[w]) : m + slots[w];
  return m;
}

template <int JH>
__global__ __launch_bounds__(4 * JH) void asg_full_forward_kernel(AsgFullArgs a) {
  constexpr int NT = 4 * JH, NW = NT / 64, NP = 2 * JH;
  __shared__ __attribute__((aligned(16))) float q[NP];
  __shared__ float slots[4];
  const int b = blockIdx.x, tid = threadIdx.x, r = tid >> 1, h = tid & 1, j0 = h * JH;
  const int N = a.N, M = a.M;
  int T = a.rows ? a.rows[b] : M;
  T = T < 1 ? 1 : (T > M ? M : T);  // (the engine has refused such counts: nothing outside the slab is addressed)
  const GTNX_G float* em = a.em + int64_t(b) * M * N;
  const GTNX_G float* W = a.w + N;
  GTNX_G float* la_out = a.la ? a.la + int64_t(b) * M * N : nullptr;
  GTNX_G double* L_out = a.L ? a.L + int64_t(b) * M : nullptr;
  const bool row = r < N;

  float E[JH];
  float rm = NEG_INF;
#pragma unroll
  for (int k = 0; k < JH; ++k) {
    const int j = j0 + k;
    E[k] = (row && j < N) ? W[int64_t(r) * N + j] : NEG_INF;
    rm = fmaxf(rm, E[k]);
  }
  rm = fmaxf(rm, __shfl_xor(rm, 1));
  if (rm == NEG_INF) rm = 0.0f;  // (a label nothing leads to: the row is all zeros)
#pragma unroll
  for (int k = 0; k < JH; ++k) E[k] = expf(E[k] - rm);
  for (int k = tid; k < NP; k += NT) q[k] = 0.0f;  // (entries [N, NP) stay zero: the rows' tails multiply them)

  double L = 0.0;
  float av = row ? a.w[r] + em[r] : NEG_INF;
  float qv = 0.0f;
  for (int t = 0;;) {
    const float m = block_reduce<NW, true>(av, slots);
    const float la = av - (m == NEG_INF ? 0.0f : m);
    L += double(m);
    qv = expf(la);
    if (row && h == 0) {
      q[r] = qv;
      if (la_out) la_out[int64_t(t) * N + r] = la;
    }
    if (tid == 0 && L_out) L_out[t] = L;
    if (++t >= T) break;
    const float e = row ? em[int64_t(t) * N + r] : NEG_INF;
    __syncthreads();
    float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
    for (int k = 0; k < JH; k += 4) {
      const float4 v = *reinterpret_cast<const float4*>(&q[j0 + k]);
      s0 = fmaf(E[k], v.x, s0);
      s1 = fmaf(E[k + 1], v.y, s1);
      s0 = fmaf(E[k + 2], v.z, s0);
      s1 = fmaf(E[k + 3], v.w, s1);
    }
    float s = s0 + s1;
    s += __shfl_xor(s, 1);
    av = s > 0.0f ? logf(s) + rm + e : NEG_INF;
  }
  __syncthreads();  // (slots: the last maximum has been read by every wave)
  const float sum = block_reduce<NW, false>((row && h == 0) ? qv : 0.0f, slots);
  if (tid == 0) {
    const double z = L + double(logf(sum));
    a.score[b] = float(z);
    if (a.zd) a.zd[b] = z;
  }
}

template <int JH, bool WANT_TR>
__global__ __launch_bounds__(4 * JH) void asg_full_backward_kernel(AsgFullArgs a) {
  constexpr int NT = 4 * JH, NW = NT / 64, NP = 2 * JH;
  __shared__ __attribute__((aligned(16))) float f[NP];
  __shared__ float rmv[NP];
  __shared__ float slots[4];
  const int b = blockIdx.x, tid = threadIdx.x, r = tid >> 1, h = tid & 1, i0 = h * JH;
  const int N = a.N, M = a.M;
  int T = a.rows ? a.rows[b] : M;
  T = T < 1 ? 1 : (T > M ? M : T);
  const int64_t A = int64_t(N) + int64_t(N) * N;
  const GTNX_G float* em = a.em + int64_t(b) * M * N;
  const GTNX_G float* W = a.w + N;
  const GTNX_G float* la = a.la + int64_t(b) * M * N;
  const GTNX_G double* Ls = a.L + int64_t(b) * M;
  GTNX_G float* ge = a.grad_em ? a.grad_em + int64_t(b) * M * N : nullptr;
  GTNX_G float* part = a.partial ? a.partial + int64_t(b) * A : nullptr;
  const double Z = a.zd[b];
  const float delta = a.delta[b];
  const bool row = r < N;

  if (!(Z > double(NEG_INF) && Z < double(-NEG_INF))) {
    // no finite path: the gradient is zero everywhere (rows < T of the emissions, every arc of the transitions)
    if (ge)
      for (int64_t k = tid; k < int64_t(T) * N; k += NT) ge[k] = 0.0f;
    if (part)
      for (int64_t k = tid; k < A; k += NT) part[k] = 0.0f;
    return;
  }

  float ET[JH], X[JH];
  float rm = NEG_INF;
#pragma unroll
  for (int k = 0; k < JH; ++k) {
    const int j = i0 + k;
    rm = fmaxf(rm, (row && j < N) ? W[int64_t(r) * N + j] : NEG_INF);
  }
  rm = fmaxf(rm, __shfl_xor(rm, 1));
  if (rm == NEG_INF) rm = 0.0f;
  for (int k = tid; k < NP; k += NT) f[k] = 0.0f;
  if (h == 0) rmv[r] = row ? rm : 0.0f;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < JH; ++k) {
    const int i = i0 + k;
    ET[k] = (row && i < N) ? expf(W[int64_t(i) * N + r] - rmv[i]) : 0.0f;
    X[k] = 0.0f;
  }

  float bq = row ? 1.0f : 0.0f;
  double LB = 0.0;
  float la_t = row ? la[int64_t(T - 1) * N + r] : NEG_INF;
  double L_t = Ls[T - 1];
  for (int t = T - 1;; --t) {
    const float lbq = bq > 0.0f ? logf(bq) : NEG_INF;
    const float gam = expf(la_t + lbq + float(L_t + LB - Z)) * delta;
    if (t == 0) {
      if (part && row && h == 0) part[r] = gam;
      if (ge && row && h == 0) ge[r] = gam;
      break;
    }
    if (ge && row && h == 0) ge[int64_t(t) * N + r] = gam;
    const float la_p = row ? la[int64_t(t - 1) * N + r] : NEG_INF;
    const double L_p = Ls[t - 1];
    const float g = (row ? em[int64_t(t) * N + r] : NEG_INF) + rm + lbq;
    const float mf = block_reduce<NW, true>(g, slots);
    const float fv = expf(g - (mf == NEG_INF ? 0.0f : mf));
    if (row && h == 0) f[r] = fv;
    __syncthreads();
    // (c is at most 1 / E of the best continuation: finite unless that one is forbidden -- kept finite so that a zero
    // of f stays a zero of the product)
    const float c = fminf(expf(la_p + float(L_p + double(mf) + LB - Z)), 3.0e38f);
    float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
    for (int k = 0; k < JH; k += 4) {
      const float4 v = *reinterpret_cast<const float4*>(&f[i0 + k]);
      s0 = fmaf(ET[k], v.x, s0);
      s1 = fmaf(ET[k + 1], v.y, s1);
      s0 = fmaf(ET[k + 2], v.z, s0);
      s1 = fmaf(ET[k + 3], v.w, s1);
      if (WANT_TR) {
        X[k] = fmaf(c, v.x, X[k]);
        X[k + 1] = fmaf(c, v.y, X[k + 1]);
        X[k + 2] = fmaf(c, v.z, X[k + 2]);
        X[k + 3] = fmaf(c, v.w, X[k + 3]);
      }
    }
    float s = s0 + s1;
    s += __shfl_xor(s, 1);
    bq = s;
    LB += double(mf);
    la_t = la_p;
    L_t = L_p;
    // (no barrier here: the next step rewrites slots after its own products and f behind the reduction's barrier)
  }
  if (WANT_TR && part && row) {
#pragma unroll
    for (int k = 0; k < JH; ++k) {
      const int i = i0 + k;
      if (i < N) part[int64_t(N) + int64_t(i) * N + r] = ET[k] > 0.0f ? ET[k] * X[k] * delta : 0.0f;
    }
  }
}

// out[k] = sum over utterances of partial[b][k], in utterance order
__global__ __launch_bounds__(256) void asg_full_reduce_kernel(const float* __restrict__ partial, int n, int64_t A,
                                                             float* __restrict__ out) {
  const int64_t k = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (k >= A) return;
  double s = 0.0;
  for (int b = 0; b < n; ++b) s += double(partial[int64_t(b) * A + k]);
  out[k] = float(s);
}

}  // namespace

int asg_full_max_labels() { return kAsgFullMaxLabels; }

void launch_asg_full_forward(const AsgFullArgs& a, hipStream_t st) {
  if (a.n <= 0) return;
  const dim3 grid(static_cast<unsigned>(a.n));
  if (a.N <= 32)
    hipLaunchKernelGGL(asg_full_forward_kernel<16>, grid, dim3(64), 0, st, a);
  else if (a.N <= 64)
    hipLaunchKernelGGL(asg_full_forward_kernel<32>, grid, dim3(128), 0, st, a);
  else
    hipLaunchKernelGGL(asg_full_forward_kernel<64>, grid, dim3(256), 0, st, a);
}

void launch_asg_full_backward(const AsgFullArgs& a, hipStream_t st) {
  if (a.n <= 0) return;
  const dim3 grid(static_cast<unsigned>(a.n));
  const bool tr = a.partial != nullptr;
#define GTNX_ASG_FULL_BWD(JH)                                                                       \
  do {                                                                                              \
    if (tr)                                                                                         \
      hipLaunchKernelGGL((asg_full_backward_kernel<JH, true>), grid, dim3(4 * JH), 0, st, a);       \
    else                                                                                            \
      hipLaunchKernelGGL((asg_full_backward_kernel<JH, false>), grid, dim3(4 * JH), 0, st, a);      \
  } while (0)
  if (a.N <= 32)
    GTNX_ASG_FULL_BWD(16);
  else if (a.N <= 64)
    GTNX_ASG_FULL_BWD(32);
  else
    GTNX_ASG_FULL_BWD(64);
#undef GTNX_ASG_FULL_BWD
}

void launch_asg_full_reduce(const float* partial, int n, int N, float* out, hipStream_t st) {
  const int64_t A = int64_t(N) + int64_t(N) * N;
  if (n <= 0 || A <= 0) return;
  hipLaunchKernelGGL(asg_full_reduce_kernel, dim3(static_cast<unsigned>((A + 255) / 256)), dim3(256), 0, st,
                     partial, n, A, out);
}

}  // namespace gtnx
