// asg_full_wide.hip -- the ASG full-connect score forwardScore(emissions_b[:T_b] o asgTransitions(table)) of a padded
// batch for alphabets of 1 .. 1024 labels, and its gradients with respect to the emissions and the [C + C * C] table
// under caller-supplied weights (DESIGN section 41 holds the contract).  The recursion is section 19's scaled
// linear-domain one: q_t[i] = exp(alpha_t[i] - L_t), E[i][j] = exp(W[i][j] - rmax[i]) (rmax 0 for a dead row), L_t the
// running sum of the per-frame maxima in float64, Z = L_{T-1} + log sum q_{T-1}; the backward is the same form (f', LB).
//
//   prep:     rmax[i] and E, zero-padded to Cpad (a multiple of 32), stored twice in the operand layout of
//             v_mfma_f32_16x16x4_f32: matrix A[r][k] lies at ((r / 16 * KB + k / 16) * 64 + r % 16 + 16 * (k % 16 / 4)) * 4
//             + k % 4, so that a wave's load of a 16 x 16 tile is 1 KiB of consecutive 16-byte reads.  e_fwd is E
//             (row = the label entered), e_bwd is E transposed (row = the label left).
//   forward:  one workgroup of 8 waves per group of G consecutive utterances walks the frames 0 .. max T_b of the group.
//             q[.][u] of the G utterances sits in LDS (double-buffered, k-quads interleaved: a lane's B operand of four
//             MFMA steps is one ds_read_b128); E streams from L2, two k blocks ahead of its use.  A wave owns the tiles
//             of 16 output labels it, it + 8, ...; a tile's product is 16 labels x 16 utterance columns, columns at or
//             past G are zero.  A column's sums read nothing but that column, in an order fixed by Cpad alone: an
//             utterance's bits do not depend on G, on its neighbours or on the slice.  Per frame: one log and one exp
//             per label, one workgroup maximum per utterance, two barriers.  An utterance past its own T_b stops
//             loading and storing; its score is written at its own last frame.
//   backward: the same grouping, frames descending from each utterance's own T_b - 1, with e_bwd.  It writes w * gamma_t
//             into the emission-gradient rows < T_b (and zeros into every row at or past T_b), w * gamma_0 into the
//             utterance's start row, and w * f_t[i] (xi_t[i][j] = c_t[j] * f_t[i] * E[i][j], c_t = exp(la_{t-1})) into
//             the second plane.
//   table:    X[i][j] = sum over (b, 1 <= t < T_b) of (w_b f_{b,t}[i]) * c_{b,t}[j] as v_mfma_f32_32x32x2_f32 tiles.  One
//             workgroup per (128 x 128 block of X, block of 16 consecutive utterances); the operands are staged through
//             double-buffered LDS 16 frames at a time, c exponentiated once on the way in.  Each workgroup stores one
//             partial.
//   reduce:   adds the partials in block order in float64, multiplies by E, adds the start rows in utterance order and
//             writes grad_table.  The order is that of the blocks, never of the slices.
// Every store is a plain C++ store; there are no atomics and no inline assembly, and no workgroup waits on another.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "kernels.h"

namespace gtnx {
namespace {

constexpr float NEG_INF = -__builtin_inff();
constexpr int kWG = 512;        // the sweeps' workgroup
constexpr int kWaves = kWG / 64;
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int64_t tiled_index(int r, int k, int KB) {
  return ((static_cast<int64_t>(r >> 4) * KB + (k >> 4)) * 64 + (r & 15) + 16 * ((k & 15) >> 2)) * 4 + (k & 3);
}

// ---- prep: one workgroup per padded row ----
__global__ __launch_bounds__(256) void asg_full_wide_prep_kernel(AsgFullWideArgs a) {
  __shared__ float s_red[256];
  const int tid = static_cast<int>(threadIdx.x);
  const int i = static_cast<int>(blockIdx.x);
  const int C = a.C, Cpad = a.Cpad, KB = Cpad >> 4;
  const GTNX_G float* row = a.table + static_cast<int64_t>(C) + static_cast<int64_t>(i) * C;
  float m = NEG_INF;
  if (i < C)
    for (int j = tid; j < C; j += 256) m = fmaxf(m, row[j]);
  s_red[tid] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) s_red[tid] = fmaxf(s_red[tid], s_red[tid + s]);
    __syncthreads();
  }
  m = s_red[0];
  if (!(m > NEG_INF)) m = 0.0f;  // (a dead row, or a pad row)
  if (tid == 0) a.rmax[i] = m;
  for (int j = tid; j < Cpad; j += 256) {
    const float e = (i < C && j < C) ? expf(row[j] - m) : 0.0f;
    a.e_fwd[tiled_index(i, j, KB)] = e;
    a.e_bwd[tiled_index(j, i, KB)] = e;
  }
}

// ---- the contraction both sweeps share: 16 rows of the tiled matrix times the G columns in LDS ----
template <int G>
__device__ __forceinline__ f4 contract_tile(const GTNX_G f4* tiles, int KB, const float* q, int lane) {
  const int u = lane & 15, rq = lane >> 4;
  const GTNX_G f4* p = tiles + lane;
  const f4* qv = reinterpret_cast<const f4*>(q) + rq * G + u;
  f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  f4 a0 = p[0], a1 = p[64];  // (KB is even: Cpad is a multiple of 32)
  for (int kb = 0; kb < KB; kb += 2) {
    const f4 c0 = a0, c1 = a1;
    if (kb + 2 < KB) {
      a0 = p[static_cast<int64_t>(kb + 2) * 64];
      a1 = p[static_cast<int64_t>(kb + 3) * 64];
    }
    f4 b0 = {0.0f, 0.0f, 0.0f, 0.0f}, b1 = b0;
    if (u < G) {
      b0 = qv[kb * 4 * G];
      b1 = qv[(kb + 1) * 4 * G];
    }
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(c0.x, b0.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(c0.y, b0.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(c0.z, b0.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(c0.w, b0.w, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(c1.x, b1.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(c1.y, b1.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(c1.z, b1.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(c1.w, b1.w, acc, 0, 0, 0);
  }
  return acc;
}

// the maximum / the sum over the four lanes that hold one utterance column
__device__ __forceinline__ float column_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float column_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}
__device__ __forceinline__ int group_max(int v) {
  for (int off = 1; off < 16; off <<= 1) v = max(v, __shfl_xor(v, off, 64));
  return v;
}

// ---- forward ----
template <int G>
__global__ __launch_bounds__(kWG) void asg_full_wide_forward_kernel(AsgFullWideArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_f[];
  const int C = a.C, Cpad = a.Cpad, KB = Cpad >> 4, NT = Cpad >> 4;
  float* s_q = s_f;                     // [2][Cpad * G]
  float* s_max = s_f + 2 * Cpad * G;    // [kWaves][16]
  float* s_sum = s_max + kWaves * 16;   // [kWaves][16]
  const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
  const int u = lane & 15, rq = lane >> 4;
  const int end = a.utt0 + a.count;
  const int b = a.utt0 + static_cast<int>(blockIdx.x) * G + u;
  const bool has = u < G && b < end;
  const int Tu = has ? min(max(a.frames[b], 0), a.M) : 0;
  const int Tmax = group_max(Tu);
  if (has && Tu == 0 && wave == 0 && rq == 0) a.scores[b] = NEG_INF;
  const GTNX_G float* em = a.em + static_cast<int64_t>(has ? b : 0) * a.M * C;
  const int64_t plane = static_cast<int64_t>(has ? b - a.utt0 : 0) * a.M * Cpad;
  const GTNX_G f4* ef = reinterpret_cast<const GTNX_G f4*>(a.e_fwd);
  double L = 0.0;
  int cur = 0;
  for (int t = 0; t < Tmax; ++t) {
    const bool live = t < Tu;
    const float* qc = s_q + cur * Cpad * G;
    f4* qn = reinterpret_cast<f4*>(s_q + (cur ^ 1) * Cpad * G);
    float lmax = NEG_INF;
    for (int it = wave; it < NT; it += kWaves) {
      const int i0 = it * 16 + rq * 4;
      float e[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) e[r] = (live && i0 + r < C) ? em[static_cast<int64_t>(t) * C + i0 + r] : NEG_INF;
      f4 v;
      if (t == 0) {  // (uniform) the start scores
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = (live && i0 + r < C) ? a.table[i0 + r] + e[r] : NEG_INF;
      } else {
        const f4 acc = contract_tile<G>(ef + static_cast<int64_t>(it) * KB * 64, KB, qc, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = live ? a.rmax[i0 + r] + logf(acc[r]) + e[r] : NEG_INF;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) lmax = fmaxf(lmax, v[r]);
      if (u < G) qn[(i0 >> 2) * G + u] = v;
    }
    lmax = column_max(lmax);
    if (rq == 0) s_max[wave * 16 + u] = lmax;
    __syncthreads();
    float m = s_max[u];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) m = fmaxf(m, s_max[w * 16 + u]);
    const bool alive = m > NEG_INF;
    L += static_cast<double>(m);
    float lsum = 0.0f;
    if (u < G) {
      for (int it = wave; it < NT; it += kWaves) {
        const int i0 = it * 16 + rq * 4;
        const f4 v = qn[(i0 >> 2) * G + u];
        f4 la, q;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          la[r] = alive ? v[r] - m : NEG_INF;
          q[r] = alive ? expf(la[r]) : 0.0f;
          lsum += q[r];
        }
        qn[(i0 >> 2) * G + u] = q;
        if (a.la && live) *reinterpret_cast<GTNX_G f4*>(a.la + plane + static_cast<int64_t>(t) * Cpad + i0) = la;
      }
    }
    lsum = column_sum(lsum);
    if (rq == 0) s_sum[wave * 16 + u] = lsum;
    if (a.lt && live && wave == 0 && rq == 0) a.lt[static_cast<int64_t>(b - a.utt0) * a.M + t] = L;
    __syncthreads();
    if (has && t == Tu - 1 && wave == 0 && rq == 0) {
      float s = s_sum[u];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) s += s_sum[w * 16 + u];
      a.scores[b] = static_cast<float>(L + static_cast<double>(logf(s)));
    }
    cur ^= 1;
  }
}

// ---- backward ----
template <int G>
__global__ __launch_bounds__(kWG) void asg_full_wide_backward_kernel(AsgFullWideArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_f[];
  const int C = a.C, Cpad = a.Cpad, KB = Cpad >> 4, NT = Cpad >> 4, M = a.M;
  float* s_q = s_f;                   // [2][Cpad * G]
  float* s_max = s_f + 2 * Cpad * G;  // [kWaves][16]
  const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
  const int u = lane & 15, rq = lane >> 4;
  const int end = a.utt0 + a.count;
  const int bg = a.utt0 + static_cast<int>(blockIdx.x) * G;
  // the rows no frame of the sweep writes: every row of an utterance that contributes nothing, the pad rows of the others
  for (int uu = 0; uu < G && bg + uu < end; ++uu) {
    const int bb = bg + uu;
    const int T = min(max(a.frames[bb], 0), M);
    const bool act = T > 0 && a.weights[bb] != 0.0f && a.scores[bb] > NEG_INF;  // (uniform)
    if (a.grad) {
      const int r0 = act ? T : 0;
      GTNX_G float* z = a.grad + (static_cast<int64_t>(bb) * M + r0) * C;
      const int64_t cells = static_cast<int64_t>(M - r0) * C;
      for (int64_t i = tid; i < cells; i += kWG) z[i] = 0.0f;
    }
    if (a.start_rows && !act)
      for (int i = tid; i < Cpad; i += kWG) a.start_rows[static_cast<int64_t>(bb) * Cpad + i] = 0.0f;
  }
  const int b = bg + u;
  const bool has = u < G && b < end;
  int Tu = has ? min(max(a.frames[b], 0), M) : 0;
  const float w = has ? a.weights[b] : 0.0f;
  const float Zf = has ? a.scores[b] : NEG_INF;
  if (w == 0.0f || !(Zf > NEG_INF)) Tu = 0;  // exact zeros, and 0 * inf is never formed
  const double Z = Tu > 0 ? static_cast<double>(Zf) : 0.0;
  const int Tmax = group_max(Tu);
  const GTNX_G float* em = a.em + static_cast<int64_t>(has ? b : 0) * M * C;
  const int64_t plane = static_cast<int64_t>(has ? b - a.utt0 : 0) * M * Cpad;
  const int64_t ltrow = static_cast<int64_t>(has ? b - a.utt0 : 0) * M;
  const GTNX_G f4* eb = reinterpret_cast<const GTNX_G f4*>(a.e_bwd);
  double LB = 0.0;
  int cur = 0;
  for (int t = Tmax - 1; t >= 0; --t) {
    const bool live = t < Tu, first = t == Tu - 1;
    const float* qc = s_q + cur * Cpad * G;
    f4* qn = reinterpret_cast<f4*>(s_q + (cur ^ 1) * Cpad * G);
    float cg = 0.0f, cf = 0.0f;
    if (live) {
      cg = static_cast<float>(a.lt[ltrow + t] + LB - Z);
      if (t > 0) cf = static_cast<float>(a.lt[ltrow + t - 1] + LB - Z);
    }
    float lmax = NEG_INF;
    for (int it = wave; it < NT; it += kWaves) {
      const int i0 = it * 16 + rq * 4;
      float e[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) e[r] = (live && i0 + r < C) ? em[static_cast<int64_t>(t) * C + i0 + r] : NEG_INF;
      f4 lav = {NEG_INF, NEG_INF, NEG_INF, NEG_INF};
      if (live) lav = *reinterpret_cast<const GTNX_G f4*>(a.la + plane + static_cast<int64_t>(t) * Cpad + i0);
      f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
      if (t < Tmax - 1) acc = contract_tile<G>(eb + static_cast<int64_t>(it) * KB * 64, KB, qc, lane);  // (uniform)
      f4 h, gam, fw;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float lb = first ? 0.0f : logf(acc[r]);
        gam[r] = live ? w * expf(lav[r] + lb + cg) : 0.0f;
        h[r] = live ? a.rmax[i0 + r] + e[r] + lb : NEG_INF;
        fw[r] = live ? w * expf(h[r] + cf) : 0.0f;
        lmax = fmaxf(lmax, h[r]);
      }
      if (live) {
        if (a.grad) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (i0 + r < C) a.grad[(static_cast<int64_t>(b) * M + t) * C + i0 + r] = gam[r];
        }
        if (a.start_rows && t == 0) *reinterpret_cast<GTNX_G f4*>(a.start_rows + static_cast<int64_t>(b) * Cpad + i0) = gam;
        if (a.fw && t > 0) *reinterpret_cast<GTNX_G f4*>(a.fw + plane + static_cast<int64_t>(t) * Cpad + i0) = fw;
      }
      if (u < G) qn[(i0 >> 2) * G + u] = h;
    }
    if (t == 0) break;  // (uniform) nothing reads f' of frame 0
    lmax = column_max(lmax);
    if (rq == 0) s_max[wave * 16 + u] = lmax;
    __syncthreads();
    float m = s_max[u];
#pragma unroll
    for (int wv = 1; wv < kWaves; ++wv) m = fmaxf(m, s_max[wv * 16 + u]);
    const bool alive = m > NEG_INF;
    if (live) LB += static_cast<double>(m);
    if (u < G) {
      for (int it = wave; it < NT; it += kWaves) {
        const int i0 = it * 16 + rq * 4;
        f4 v = qn[(i0 >> 2) * G + u];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = alive ? expf(v[r] - m) : 0.0f;
        qn[(i0 >> 2) * G + u] = v;
      }
    }
    __syncthreads();
    cur ^= 1;
  }
}

// ---- table: X = sum over the frames of the block's utterances of (w f)(i) c(j) ----
constexpr int kTB = 128;  // the block of X a workgroup owns
constexpr int kTK = 16;   // frames staged at a time

__global__ __launch_bounds__(256) void asg_full_wide_table_kernel(AsgFullWideArgs a) {
  __shared__ __attribute__((aligned(16))) float s_a[2][kTK][kTB];
  __shared__ __attribute__((aligned(16))) float s_b[2][kTK][kTB];
  __shared__ int s_T[kAsgFullWideBlock];
  const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
  const int Cpad = a.Cpad, M = a.M;
  const int i0 = static_cast<int>(blockIdx.x) * kTB, j0 = static_cast<int>(blockIdx.y) * kTB;
  const int blk = static_cast<int>(blockIdx.z);
  const int bu = a.utt0 + blk * kAsgFullWideBlock;
  if (tid < kAsgFullWideBlock) {
    const int b = bu + tid;
    int T = 0;
    if (b < a.utt0 + a.count) {
      T = min(max(a.frames[b], 0), M);
      if (a.weights[b] == 0.0f || !(a.scores[b] > NEG_INF)) T = 0;  // (the backward's test: its plane was not written)
    }
    s_T[tid] = T;
  }
  __syncthreads();
  const int c4 = (tid & 31) * 4, kk = tid >> 5;  // this thread stages rows kk and kk + 8, four columns from c4
  const bool in_a = i0 + c4 < Cpad, in_b = j0 + c4 < Cpad;
  f4 ra[2], rb[2];
  const f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  auto fetch = [&](int uu, int t0) {
    const int64_t plane = static_cast<int64_t>(bu - a.utt0 + uu) * M * Cpad;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int t = t0 + kk + 8 * h;
      ra[h] = rb[h] = zero;
      if (t < s_T[uu]) {
        if (in_a) ra[h] = *reinterpret_cast<const GTNX_G f4*>(a.fw + plane + static_cast<int64_t>(t) * Cpad + i0 + c4);
        if (in_b) {
          const f4 l = *reinterpret_cast<const GTNX_G f4*>(a.la + plane + static_cast<int64_t>(t - 1) * Cpad + j0 + c4);
#pragma unroll
          for (int r = 0; r < 4; ++r) rb[h][r] = expf(l[r]);
        }
      }
    }
  };
  // the chunks in order: utterances ascending, frames 1 .. T_b - 1 ascending, kTK at a time
  auto advance = [&](int& uu, int& t0) {
    t0 += kTK;
    while (uu < kAsgFullWideBlock && t0 >= s_T[uu]) {
      ++uu;
      t0 = 1;
    }
  };
  int uu = 0, t0 = 1 - kTK;
  advance(uu, t0);
  f16 acc[2][2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[x][y][r] = 0.0f;
  const int wi = (wave >> 1) * 64, wj = (wave & 1) * 64, l32 = lane & 31, kh = lane >> 5;
  if (uu < kAsgFullWideBlock) fetch(uu, t0);
  int buf = 0;
  while (uu < kAsgFullWideBlock) {  // (uniform)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      *reinterpret_cast<f4*>(&s_a[buf][kk + 8 * h][c4]) = ra[h];
      *reinterpret_cast<f4*>(&s_b[buf][kk + 8 * h][c4]) = rb[h];
    }
    __syncthreads();
    advance(uu, t0);
    if (uu < kAsgFullWideBlock) fetch(uu, t0);
#pragma unroll
    for (int k = 0; k < kTK; k += 2) {
      const float a0 = s_a[buf][k + kh][wi + l32], a1 = s_a[buf][k + kh][wi + 32 + l32];
      const float b0 = s_b[buf][k + kh][wj + l32], b1 = s_b[buf][k + kh][wj + 32 + l32];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    buf ^= 1;
  }
  GTNX_G float* out = a.partial + static_cast<int64_t>(bu / kAsgFullWideBlock) * Cpad * Cpad;
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = i0 + wi + x * 32 + (r >> 2) * 8 + kh * 4 + (r & 3);
        const int j = j0 + wj + y * 32 + l32;
        if (i < Cpad && j < Cpad) out[static_cast<int64_t>(i) * Cpad + j] = acc[x][y][r];
      }
}

// ---- reduce: the partials in block order, times E; the start rows in utterance order ----
__global__ __launch_bounds__(256) void asg_full_wide_reduce_kernel(AsgFullWideArgs a) {
  const int C = a.C, Cpad = a.Cpad;
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= static_cast<int64_t>(C) + static_cast<int64_t>(C) * C) return;
  double s = 0.0;
  if (idx < C) {
    for (int b = 0; b < a.n; ++b) s += static_cast<double>(a.start_rows[static_cast<int64_t>(b) * Cpad + idx]);
    a.grad_table[idx] = static_cast<float>(s);
    return;
  }
  const int i = static_cast<int>((idx - C) / C), j = static_cast<int>((idx - C) % C);
  const int blocks = (a.n + kAsgFullWideBlock - 1) / kAsgFullWideBlock;
  const int64_t cell = static_cast<int64_t>(i) * Cpad + j;
  for (int k = 0; k < blocks; ++k) s += static_cast<double>(a.partial[static_cast<int64_t>(k) * Cpad * Cpad + cell]);
  const float e = a.e_fwd[tiled_index(i, j, Cpad >> 4)];
  a.grad_table[idx] = e > 0.0f ? static_cast<float>(s * static_cast<double>(e)) : 0.0f;
}

size_t sweep_lds(int Cpad, int G) { return sizeof(float) * (2 * size_t(Cpad) * size_t(G) + 2 * kWaves * 16); }

template <int G>
void launch_sweep(bool backward, const AsgFullWideArgs& a, hipStream_t st) {
  const size_t lds = sweep_lds(a.Cpad, G);
  const void* fn = backward ? reinterpret_cast<const void*>(asg_full_wide_backward_kernel<G>)
                            : reinterpret_cast<const void*>(asg_full_wide_forward_kernel<G>);
  if (lds > 64 * 1024) HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
  const dim3 grid(static_cast<unsigned>((a.count + G - 1) / G));
  if (backward) hipLaunchKernelGGL(asg_full_wide_backward_kernel<G>, grid, dim3(kWG), lds, st, a);
  else hipLaunchKernelGGL(asg_full_wide_forward_kernel<G>, grid, dim3(kWG), lds, st, a);
  HIP_CHECK(hipGetLastError());  // (a launch that is refused is this call's error, not the next caller's)
}

void dispatch_sweep(bool backward, const AsgFullWideArgs& a, hipStream_t st) {
  if (a.count <= 0) return;
  if (a.G == 4) launch_sweep<4>(backward, a, st);
  else if (a.G == 8) launch_sweep<8>(backward, a, st);
  else launch_sweep<16>(backward, a, st);
}

}  // namespace

// The fewest utterances per workgroup that still give every compute unit (256 as the working figure) at most one
// workgroup: the contraction is the same MFMA tile for every G, so a workgroup's frame costs the same whatever G is, and
// a smaller group only adds workgroups while units are idle.
int asg_full_wide_group(int n) {
  if (n <= 4 * 256) return 4;
  if (n <= 8 * 256) return 8;
  return 16;
}

void launch_asg_full_wide_prep(const AsgFullWideArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(asg_full_wide_prep_kernel, dim3(static_cast<unsigned>(a.Cpad)), dim3(256), 0, st, a);
  HIP_CHECK(hipGetLastError());
}

void launch_asg_full_wide_forward(const AsgFullWideArgs& a, hipStream_t st) { dispatch_sweep(false, a, st); }

void launch_asg_full_wide_backward(const AsgFullWideArgs& a, hipStream_t st) { dispatch_sweep(true, a, st); }

void launch_asg_full_wide_table(const AsgFullWideArgs& a, hipStream_t st) {
  if (a.count <= 0) return;
  const unsigned tiles = static_cast<unsigned>((a.Cpad + kTB - 1) / kTB);
  const unsigned blocks = static_cast<unsigned>((a.count + kAsgFullWideBlock - 1) / kAsgFullWideBlock);
  hipLaunchKernelGGL(asg_full_wide_table_kernel, dim3(tiles, tiles, blocks), dim3(256), 0, st, a);
  HIP_CHECK(hipGetLastError());
}

void launch_asg_full_wide_reduce(const AsgFullWideArgs& a, hipStream_t st) {
  const int64_t cells = int64_t(a.C) + int64_t(a.C) * a.C;
  hipLaunchKernelGGL(asg_full_wide_reduce_kernel, dim3(static_cast<unsigned>((cells + 255) / 256)), dim3(256), 0, st, a);
  HIP_CHECK(hipGetLastError());
}

}  // namespace gtnx
