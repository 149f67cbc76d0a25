// transducer_add.hip -- the transducer (RNN-T) log score of a padded batch under an ADDITIVE joint, without the joint
// tensor: logits z[b,t,u,c] = am[b,t,c] + lm[b,u,c] with am [B][T][C] and lm [B][U+1][C] on the device, and the gradient
// with respect to am and lm under caller-supplied weights (DESIGN section 43 holds the contract; section 42 and
// transducer.hip hold the lattice and its sweep, which is reused unchanged).  Everything factorises over the rows:
//   lse[t,u] = ma[t] + ml[u] + log S[t,u],  S = Ea El^T,  Ea = exp(am - ma),  El = exp(lm - ml)  (ma, ml the row maxima)
//   grad_am  = -Ea o (A El)   + sparse,     grad_lm = -El o (A^T Ea) + sparse,   A = w (occ_b + occ_l) / S
// so the work is three float32 matrix products on v_mfma_f32_32x32x2_f32 and the inputs are B (T + U + 1) C floats.
//
// DOMAIN.  S is summed in float32.  The accuracy of the contract holds while every live row of am and of lm spans at most
// 40 nats (maximum minus smallest finite entry): then every product Ea El at the joint maximum is at least e^-80, a
// normal float32.  -inf entries (masked labels) are allowed and contribute 0.  A node whose sum underflows to 0 is a dead
// node, (-inf, -inf, 0), never NaN.
//
//   max:   one wave per live row of am and of lm: the row maximum into ma [count][T] / ml [count][U+1] (16-byte loads
//          when C % 4 == 0 and the tensors are aligned).  A row with NaN or +inf, or nothing but -inf, stores +inf, the
//          marker of a dead row: its exponentials are staged as zeros and its nodes get (-inf, -inf, 0).
//   norm:  a workgroup of 4 waves per 64 (t) x 64 (u) tile of S of one utterance, a 32 x 32 block of accumulators per
//          wave.  The loop over C stages 32 labels of 64 am rows and 64 lm rows through LDS, transposed ([label][row],
//          stride 66: the staging writes and the operand reads both spread over the banks), exp(x - rowmax) applied on
//          the way in, the tail of C and the rows past the lengths as zeros (never read).  Two LDS buffers: the global
//          loads of chunk i + 1 are issued before the MFMAs of chunk i, one barrier per chunk.  The epilogue gathers the
//          blank and label entries of the two rows and stores transducer.hip's compact triple (lp_blank, lp_label, lse)
//          into the same plane [count][T][U+1][3].  Tiles wholly outside t < T_b, u <= U_b leave at once.
//   grad:  one tile routine for both products, out[m, c] = -exp(x[m, c] - max[m]) sum_n A[m, n] exp(y[n, c] - max[n]),
//          (m, n) = (t, u) for grad_am and (u, t) for grad_lm.  A workgroup owns a 64 (m) x 64 (c) tile of the output; the
//          loop over n stages 32 columns of A (built from alpha, beta, the triple and the score on the way in) and 32
//          rows of y.  The tile goes through LDS once more, where the workgroup adds the sparse terms it owns (column
//          blank: w sum_n occ_b, four partial sums per row added in a fixed order; column y[u]: w occ_l, for grad_am in
//          ascending u by the row's one thread) and is then stored with 16-byte stores: every element of grad_am and
//          grad_lm exactly once, rows past the lengths and utterances that score -inf as zeros without a load.
// Every store is a plain C++ store; there are no atomics and no inline assembly, and no workgroup waits on another.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "common.h"
#include "kernels.h"

namespace gtnx {
namespace {

constexpr float NEG_INF = -__builtin_inff();
constexpr float POS_INF = __builtin_inff();
constexpr int kWG = 256;
constexpr int kTile = 64;  // the edge of a workgroup's tile
constexpr int kKC = 32;    // the reduction chunk staged at a time
constexpr int kLdT = 66;   // LDS stride of a transposed operand [k][64 rows]
constexpr int kLdC = 68;   // LDS stride of an operand [k][64 labels] and of the output tile (16-byte rows)
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ bool utt_ok(const TransducerAddArgs& a, int Tb, int Ub) {
  return Tb >= 1 && Tb <= a.T && Ub >= 0 && Ub < a.U1;
}
// y[u] for u < U_b, or -1 where there is no label to leave the column by (never becomes an address)
__device__ __forceinline__ int label_at(const TransducerAddArgs& a, int b, int u, int Ub) {
  if (u >= Ub) return -1;
  const int tok = a.targets[static_cast<int64_t>(b) * (a.U1 - 1) + u];
  return (tok >= 0 && tok < a.C && tok != a.blank) ? tok : -1;
}
// labels c .. c + 3 of a row (c % 4 == 0), -inf past C
template <int W>
__device__ __forceinline__ f4 load4(const GTNX_G float* row, int c, int C) {
  f4 q = {NEG_INF, NEG_INF, NEG_INF, NEG_INF};
  if (W == 4) {
    if (c < C) q = *reinterpret_cast<const GTNX_G f4*>(row + c);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c + k < C) q[k] = row[c + k];
  }
  return q;
}

// ---- max: one wave per row of the slice's am and lm ----
template <int W>
__global__ __launch_bounds__(kWG) void transducer_add_max_kernel(TransducerAddArgs a) {
  const int lane = static_cast<int>(threadIdx.x) & 63;
  const int per = a.T + a.U1;
  const int64_t r = static_cast<int64_t>(blockIdx.x) * (kWG / 64) + (threadIdx.x >> 6);
  if (r >= static_cast<int64_t>(a.count) * per) return;
  const int lb = static_cast<int>(r / per), rem = static_cast<int>(r - static_cast<int64_t>(lb) * per);
  const int b = a.utt0 + lb;
  const int Tb = a.frames[b], Ub = a.tlen[b];
  if (!utt_ok(a, Tb, Ub)) return;
  const bool is_am = rem < a.T;
  const int idx = is_am ? rem : rem - a.T;
  if (is_am ? idx >= Tb : idx > Ub) return;  // (never read)
  const GTNX_G float* row = is_am ? a.am + (static_cast<int64_t>(b) * a.T + idx) * a.C
                                  : a.lm + (static_cast<int64_t>(b) * a.U1 + idx) * a.C;
  float m = NEG_INF;
  bool bad = false;  // NaN or +inf seen
  for (int c = lane * 4; c < a.C; c += 256) {
    const f4 q = load4<W>(row, c, a.C);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      bad |= !(q[k] < POS_INF);
      m = fmaxf(m, q[k]);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  const bool dead = __any(bad) || !(m > NEG_INF);
  if (lane == 0) {
    if (is_am) a.ma[static_cast<int64_t>(lb) * a.T + idx] = dead ? POS_INF : m;
    else a.ml[static_cast<int64_t>(lb) * a.U1 + idx] = dead ? POS_INF : m;
  }
}

// ---- norm: a 64 x 64 tile of S = Ea El^T per workgroup, then the compact triples ----
template <int W>
__global__ __launch_bounds__(kWG) void transducer_add_norm_kernel(TransducerAddArgs a, int tilesT, int tilesU) {
  __shared__ float s_a[2][kKC][kLdT];
  __shared__ float s_b[2][kKC][kLdT];
  const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
  int blk = static_cast<int>(blockIdx.x);
  const int ut = blk % tilesU;
  blk /= tilesU;
  const int tt = blk % tilesT, lb = blk / tilesT, b = a.utt0 + lb;
  const int Tb = uni(a.frames[b]), Ub = uni(a.tlen[b]);
  if (!utt_ok(a, Tb, Ub)) return;
  const int t0 = tt * kTile, u0 = ut * kTile;
  if (t0 >= Tb || u0 > Ub) return;
  const int C = a.C;

  // staging: a thread takes the labels 4 sq .. 4 sq + 3 of the rows sr and sr + 32 of both operands
  const int sr = tid >> 3, sq = tid & 7;
  const GTNX_G float* pa[2];
  const GTNX_G float* pb[2];
  float mxa[2], mxb[2];
  bool la[2], lv[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int t = t0 + sr + 32 * h, u = u0 + sr + 32 * h;
    mxa[h] = t < Tb ? a.ma[static_cast<int64_t>(lb) * a.T + t] : POS_INF;
    mxb[h] = u <= Ub ? a.ml[static_cast<int64_t>(lb) * a.U1 + u] : POS_INF;
    la[h] = mxa[h] < POS_INF;  // (a row past the length or a dead row: zeros, nothing is loaded)
    lv[h] = mxb[h] < POS_INF;
    pa[h] = a.am + (static_cast<int64_t>(b) * a.T + (la[h] ? t : 0)) * C;
    pb[h] = a.lm + (static_cast<int64_t>(b) * a.U1 + (lv[h] ? u : 0)) * C;
    if (!la[h]) mxa[h] = 0.0f;
    if (!lv[h]) mxb[h] = 0.0f;
  }
  const f4 none = {NEG_INF, NEG_INF, NEG_INF, NEG_INF};
  f4 ra[2], rb[2];
  auto fetch = [&](int c0) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      ra[h] = la[h] ? load4<W>(pa[h], c0 + 4 * sq, C) : none;
      rb[h] = lv[h] ? load4<W>(pb[h], c0 + 4 * sq, C) : none;
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        s_a[buf][4 * sq + k][sr + 32 * h] = expf(ra[h][k] - mxa[h]);
        s_b[buf][4 * sq + k][sr + 32 * h] = expf(rb[h][k] - mxb[h]);
      }
  };

  f16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32, l32 = lane & 31, kh = lane >> 5;
  const int chunks = (C + kKC - 1) / kKC;
  fetch(0);
  stage(0);
  __syncthreads();
  int buf = 0;
  for (int ch = 0; ch < chunks; ++ch) {
    const bool more = ch + 1 < chunks;
    if (more) fetch((ch + 1) * kKC);
#pragma unroll
    for (int k = 0; k < kKC; k += 2)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(s_a[buf][k + kh][wi + l32], s_b[buf][k + kh][wj + l32], acc, 0, 0, 0);
    if (more) stage(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }

  // the triples of the wave's 32 x 32 block: the lane's column u, 16 rows t
  const int u = u0 + wj + l32;
  if (u > Ub) return;
  const float mlu = a.ml[static_cast<int64_t>(lb) * a.U1 + u];
  const GTNX_G float* lrow = a.lm + (static_cast<int64_t>(b) * a.U1 + u) * C;
  const int tok = label_at(a, b, u, Ub);
  const bool ulive = mlu < POS_INF;
  const float lmb = ulive ? lrow[a.blank] - mlu : 0.0f;
  const float lml = ulive && tok >= 0 ? lrow[tok] - mlu : 0.0f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int t = t0 + wi + (r >> 2) * 8 + kh * 4 + (r & 3);
    if (t >= Tb) continue;
    const float mat = a.ma[static_cast<int64_t>(lb) * a.T + t];
    const float ls = logf(acc[r]);  // (a sum that is 0: -inf)
    const float lse = mat + mlu + ls;
    GTNX_G float* out = a.rows + ((static_cast<int64_t>(lb) * a.T + t) * a.U1 + u) * 3;
    if (!ulive || !(mat < POS_INF) || !(fabsf(lse) < POS_INF)) {  // a dead row, or a sum that underflowed
      out[0] = NEG_INF;
      out[1] = NEG_INF;
      out[2] = 0.0f;
      continue;
    }
    const GTNX_G float* arow = a.am + (static_cast<int64_t>(b) * a.T + t) * C;
    out[0] = (arow[a.blank] - mat) + lmb - ls;
    out[1] = tok >= 0 ? (arow[tok] - mat) + lml - ls : NEG_INF;
    out[2] = lse;
  }
}

// ---- grad ----
// occ_b and occ_l of the live node (t, u) of an utterance with a finite score, as transducer.hip's gradient has them
__device__ __forceinline__ void occupancy(const TransducerAddArgs& a, int lb, int t, int u, int Tb, int Ub, float sc,
                                          float& ob, float& ol) {
  const int64_t r = (static_cast<int64_t>(lb) * a.T + t) * a.U1 + u;
  const GTNX_G float* p = a.rows + r * 3;
  const float al = a.alpha[r];
  const float bb = t + 1 < Tb ? a.beta[r + a.U1] : (u == Ub ? 0.0f : NEG_INF);
  const float bl = u < Ub ? a.beta[r + 1] : NEG_INF;
  ob = expf(al + p[0] + bb - sc);  // (every term is finite or -inf, so is the sum)
  ol = expf(al + p[1] + bl - sc);
}

// TRANS false: grad_am, rows m = t, reduction n = u.  TRANS true: grad_lm, rows m = u, reduction n = t.
template <bool TRANS, int W>
__global__ __launch_bounds__(kWG) void transducer_add_grad_kernel(TransducerAddArgs a, int tilesM, int tilesC) {
  __shared__ float s_a[2][kKC][kLdT];  // A^T: [n][m]
  __shared__ __attribute__((aligned(16))) float s_b[2][kKC][kLdC];  // exp(y - max): [n][c]
  __shared__ __attribute__((aligned(16))) float s_o[kTile][kLdC];   // the output tile
  __shared__ float s_p[2][4][kTile];   // partial sums of the sparse terms: (blank, label) x four threads x row
  const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
  int blk = static_cast<int>(blockIdx.x);
  const int ct = blk % tilesC;
  blk /= tilesC;
  const int mt = blk % tilesM, lb = blk / tilesM, b = a.utt0 + lb;
  const int Tb = uni(a.frames[b]), Ub = uni(a.tlen[b]);
  const int C = a.C, T = a.T, U1 = a.U1;
  const int M = TRANS ? U1 : T, N = TRANS ? T : U1;
  const int m0 = mt * kTile, c0 = ct * kTile;
  const GTNX_G float* xm = (TRANS ? a.lm : a.am) + static_cast<int64_t>(b) * M * C;
  const GTNX_G float* xn = (TRANS ? a.am : a.lm) + static_cast<int64_t>(b) * N * C;
  const GTNX_G float* mxm = TRANS ? a.ml + static_cast<int64_t>(lb) * U1 : a.ma + static_cast<int64_t>(lb) * T;
  const GTNX_G float* mxn = TRANS ? a.ma + static_cast<int64_t>(lb) * T : a.ml + static_cast<int64_t>(lb) * U1;
  GTNX_G float* out = (TRANS ? a.grad_lm : a.grad_am) + static_cast<int64_t>(b) * M * C;
  const int orow = tid >> 4, oc = c0 + 4 * (tid & 15);  // the thread's part of the tile: rows orow + 16 h, four labels

  const bool ok = utt_ok(a, Tb, Ub);
  const float sc = ok ? a.scores[b] : NEG_INF;
  const int Mb = TRANS ? Ub + 1 : Tb, Nb = TRANS ? Tb : Ub + 1;  // the live rows and the live reduction length
  if (!ok || !(sc > NEG_INF) || m0 >= Mb) {  // (uniform) zeros, nothing is read
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int m = m0 + orow + 16 * h;
      if (m >= M) continue;
      GTNX_G float* o = out + static_cast<int64_t>(m) * C + oc;
      if (W == 4) {
        const f4 z = {0.0f, 0.0f, 0.0f, 0.0f};
        if (oc < C) *reinterpret_cast<GTNX_G f4*>(o) = z;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (oc + k < C) o[k] = 0.0f;
      }
    }
    return;
  }
  const float w = a.weights[b];

  // A: eight nodes per thread and chunk.  (t, u) -> the lanes run along u, the planes' fast axis.
  float n_al[8], n_pb[8], n_pl[8], n_bb[8], n_bl[8], n_sh[8];  // (n_sh: ma + ml - lse)
  auto a_index = [&](int j, int& mm, int& nn) {
    if (TRANS) {
      mm = tid & 63;
      nn = (tid >> 6) * 8 + j;
    } else {
      nn = tid & 31;
      mm = (tid >> 5) + 8 * j;
    }
  };
  auto fetch_a = [&](int n0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int mm, nn;
      a_index(j, mm, nn);
      const int t = TRANS ? n0 + nn : m0 + mm, u = TRANS ? m0 + mm : n0 + nn;
      n_al[j] = n_pb[j] = n_pl[j] = n_bb[j] = n_bl[j] = NEG_INF;
      n_sh[j] = 0.0f;
      if (t < Tb && u <= Ub) {
        const int64_t r = (static_cast<int64_t>(lb) * T + t) * U1 + u;
        const GTNX_G float* p = a.rows + r * 3;
        n_al[j] = a.alpha[r];
        n_pb[j] = p[0];
        n_pl[j] = p[1];
        n_bb[j] = t + 1 < Tb ? a.beta[r + U1] : (u == Ub ? 0.0f : NEG_INF);
        n_bl[j] = u < Ub ? a.beta[r + 1] : NEG_INF;
        n_sh[j] = a.ma[static_cast<int64_t>(lb) * T + t] + a.ml[static_cast<int64_t>(lb) * U1 + u] - p[2];
      }
    }
  };
  auto stage_a = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int mm, nn;
      a_index(j, mm, nn);
      const float occ = expf(n_al[j] + n_pb[j] + n_bb[j] - sc) + expf(n_al[j] + n_pl[j] + n_bl[j] - sc);
      // (a dead node has occ 0 and a marker in n_sh: 0 * inf is never formed)
      s_a[buf][nn][mm] = occ > 0.0f ? w * occ * expf(n_sh[j]) : 0.0f;
    }
  };
  // y: the labels oc .. oc + 3 of the rows orow and orow + 16 of the chunk
  f4 rb[2];
  float mb[2];
  const f4 none = {NEG_INF, NEG_INF, NEG_INF, NEG_INF};
  auto fetch_b = [&](int n0) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int n = n0 + orow + 16 * h;
      const float mx = n < Nb ? mxn[n] : POS_INF;
      const bool live = mx < POS_INF;
      mb[h] = live ? mx : 0.0f;
      rb[h] = live ? load4<W>(xn + static_cast<int64_t>(n) * C, oc, C) : none;
    }
  };
  auto stage_b = [&](int buf) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f4 e;
#pragma unroll
      for (int k = 0; k < 4; ++k) e[k] = expf(rb[h][k] - mb[h]);
      *reinterpret_cast<f4*>(&s_b[buf][orow + 16 * h][4 * (tid & 15)]) = e;
    }
  };

  f16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32, l32 = lane & 31, kh = lane >> 5;
  const int chunks = (Nb + kKC - 1) / kKC;  // (at least 1)
  fetch_a(0);
  fetch_b(0);
  stage_a(0);
  stage_b(0);
  __syncthreads();
  int buf = 0;
  for (int ch = 0; ch < chunks; ++ch) {
    const bool more = ch + 1 < chunks;
    if (more) {
      fetch_a((ch + 1) * kKC);
      fetch_b((ch + 1) * kKC);
    }
#pragma unroll
    for (int k = 0; k < kKC; k += 2)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(s_a[buf][k + kh][wi + l32], s_b[buf][k + kh][wj + l32], acc, 0, 0, 0);
    if (more) {
      stage_a(buf ^ 1);
      stage_b(buf ^ 1);
    }
    __syncthreads();
    buf ^= 1;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) s_o[wi + (r >> 2) * 8 + kh * 4 + (r & 3)][wj + l32] = acc[r];
  __syncthreads();

  // the dense term: -exp(x - max) times the product; zeros in the rows past the length and in dead rows
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const int i = orow + 16 * h, m = m0 + i;
    const float mx = m < Mb ? mxm[m] : POS_INF;
    f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (mx < POS_INF) {
      const f4 x = load4<W>(xm + static_cast<int64_t>(m) * C, oc, C);
      const f4 o = *reinterpret_cast<const f4*>(&s_o[i][4 * (tid & 15)]);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = 0.0f - expf(x[k] - mx) * o[k];
    }
    *reinterpret_cast<f4*>(&s_o[i][4 * (tid & 15)]) = v;
  }

  // the sparse terms of this tile.  Four threads per row sum over n = q, q + 4, ...; thread q == 0 adds them in order.
  {
    const int i = tid & 63, q = tid >> 6, m = m0 + i;
    const bool has_blank = a.blank >= c0 && a.blank < c0 + kTile;  // (uniform)
    int tok = -1;  // grad_lm: the row's own label, when its column lies in this tile
    if (TRANS && m < Mb) {
      tok = label_at(a, b, m, Ub);
      if (tok < c0 || tok >= c0 + kTile) tok = -1;
    }
    float sb = 0.0f, sl = 0.0f;
    if (m < Mb && (has_blank || tok >= 0)) {
      for (int n = q; n < Nb; n += 4) {
        float ob, ol;
        occupancy(a, lb, TRANS ? n : m, TRANS ? m : n, Tb, Ub, sc, ob, ol);
        sb += ob;
        sl += ol;
      }
    }
    s_p[0][q][i] = sb;
    s_p[1][q][i] = sl;
    __syncthreads();  // (the dense term is in place too)
    if (q == 0 && m < Mb) {
      if (has_blank) s_o[i][a.blank - c0] += w * (((s_p[0][0][i] + s_p[0][1][i]) + s_p[0][2][i]) + s_p[0][3][i]);
      if (tok >= 0) s_o[i][tok - c0] += w * (((s_p[1][0][i] + s_p[1][1][i]) + s_p[1][2][i]) + s_p[1][3][i]);
      if (!TRANS) {  // grad_am: every label whose column lies in this tile, in ascending u
        for (int u = 0; u < Ub; ++u) {
          const int tk = uni(label_at(a, b, u, Ub));
          if (tk < c0 || tk >= c0 + kTile) continue;
          float ob, ol;
          occupancy(a, lb, m, u, Tb, Ub, sc, ob, ol);
          s_o[i][tk - c0] += w * ol;
        }
      }
    }
    __syncthreads();
  }

#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const int i = orow + 16 * h, m = m0 + i;
    if (m >= M) continue;
    GTNX_G float* o = out + static_cast<int64_t>(m) * C + oc;
    if (W == 4) {
      if (oc < C) *reinterpret_cast<GTNX_G f4*>(o) = *reinterpret_cast<const f4*>(&s_o[i][4 * (tid & 15)]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (oc + k < C) o[k] = s_o[i][4 * (tid & 15) + k];
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline int tiles(int n) { return (n + kTile - 1) / kTile; }

// the utterances first .. first + n - 1 of the slice as a slice of their own
TransducerAddArgs part_of(const TransducerAddArgs& a, int first, int n) {
  TransducerAddArgs p = a;
  const int64_t nodes = static_cast<int64_t>(first) * a.T * a.U1;
  p.utt0 = a.utt0 + first;
  p.count = n;
  p.ma = a.ma + static_cast<int64_t>(first) * a.T;
  p.ml = a.ml + static_cast<int64_t>(first) * a.U1;
  p.rows = a.rows + nodes * 3;
  p.alpha = a.alpha + nodes;
  p.beta = a.beta + nodes;
  return p;
}

template <bool TRANS>
void grad_launch(const TransducerAddArgs& a, bool wide, hipStream_t st) {
  const int tm = tiles(TRANS ? a.U1 : a.T), tc = tiles(a.C);
  const int64_t per = static_cast<int64_t>(tm) * tc;  // (at most 2^24)
  const int step = static_cast<int>(std::max<int64_t>(1, (int64_t(1) << 30) / per));
  for (int first = 0; first < a.count; first += step) {
    const TransducerAddArgs p = part_of(a, first, std::min(step, a.count - first));
    const dim3 grid(static_cast<unsigned>(per * p.count));
    if (wide) hipLaunchKernelGGL((transducer_add_grad_kernel<TRANS, 4>), grid, dim3(kWG), 0, st, p, tm, tc);
    else hipLaunchKernelGGL((transducer_add_grad_kernel<TRANS, 1>), grid, dim3(kWG), 0, st, p, tm, tc);
  }
}

}  // namespace

void launch_transducer_add_max(const TransducerAddArgs& a, hipStream_t st) {
  if (a.count <= 0) return;
  const int64_t rows = static_cast<int64_t>(a.count) * (a.T + a.U1);
  const dim3 grid(static_cast<unsigned>((rows + kWG / 64 - 1) / (kWG / 64)));
  if ((a.C & 3) == 0 && aligned16(a.am) && aligned16(a.lm))
    hipLaunchKernelGGL(transducer_add_max_kernel<4>, grid, dim3(kWG), 0, st, a);
  else
    hipLaunchKernelGGL(transducer_add_max_kernel<1>, grid, dim3(kWG), 0, st, a);
  HIP_CHECK(hipGetLastError());
}

void launch_transducer_add_norm(const TransducerAddArgs& a, hipStream_t st) {
  if (a.count <= 0) return;
  const int tt = tiles(a.T), tu = tiles(a.U1);
  const dim3 grid(static_cast<unsigned>(static_cast<int64_t>(a.count) * tt * tu));  // (below count * T * U1 < 2^31)
  if ((a.C & 3) == 0 && aligned16(a.am) && aligned16(a.lm))
    hipLaunchKernelGGL(transducer_add_norm_kernel<4>, grid, dim3(kWG), 0, st, a, tt, tu);
  else
    hipLaunchKernelGGL(transducer_add_norm_kernel<1>, grid, dim3(kWG), 0, st, a, tt, tu);
  HIP_CHECK(hipGetLastError());
}

void launch_transducer_add_grad(const TransducerAddArgs& a, hipStream_t st) {
  if (a.count <= 0) return;
  const bool wide =
      (a.C & 3) == 0 && aligned16(a.am) && aligned16(a.lm) && aligned16(a.grad_am) && aligned16(a.grad_lm);
  grad_launch<false>(a, wide, st);
  grad_launch<true>(a, wide, st);
  HIP_CHECK(hipGetLastError());
}

}  // namespace gtnx
