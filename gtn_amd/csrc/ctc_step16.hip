// ctc_step16.hip -- one CTC criterion step over bfloat16 / float16 emissions in ONE launch (DESIGN section "CTC step on
// 16-bit emissions" holds the contract).  One workgroup of 512 lanes per utterance, nothing crosses utterances:
//
//   loss_b = forwardScore(E_b) - forwardScore(ctcGraph(target_b) o E_b),  E_b = float(emissions[b, :T_b]) (exact),
//   grad_b = d loss_b / d emissions[b], stored in the emissions' type (round to nearest even) or in float32.
//
// Waves 0 .. 3 are SWEEPERS: lane l owns the states l, l + 256, .. (PER of them, labels and skip flags in registers) of
// the 2 U + 1 <= 1023 states of ctcGraph(target).  Waves 4 .. 7 are STREAMERS: they move rows between HBM and a ring of
// kRing raw 16-bit rows in LDS, in 16-byte pieces of eight elements, four rows (one per wave) to a group.  The ring
// holds the raw rows, not float32: half the LDS (a row of 4096 labels is 8 KB), and the conversion at the sweepers'
// gather is one shift (bfloat16) or one convert (float16) per state.
//
// Both sweeps run in PHASES, one workgroup barrier each, position n = 0, 1, ..: frame n forward, frame T_b - 1 - n on
// the way back.  Group k (positions 4 k .. 4 k + 3) is loaded into the streamers' registers in phase 4 k - 5 and lands in
// the ring in phase 4 k - 2: the loads have three phases to arrive, a landed row is in place a phase before any sweeper
// gathers from it, and the slots it takes were last used in phase 4 k - 4.  Groups 0 and 1 land before phase 0.
//
//   forward:  a streamer wave reduces its row in registers -- maximum, then sum of exp(x - max), each by the lane's
//             elements in order and the wave's xor tree -- and leaves the row's log-sum-exp in LDS and in scratch.  The
//             sweepers run alpha_t[s] = logadd(logadd(alpha[s], alpha[s - 1]), alpha[s - 2] if skip) + e(t, label(s))
//             on a row that ping-pongs in LDS behind two -inf cells, store every row (float32, pooled scratch) and
//             lane 0 adds the row log-sum-exps in frame order: the normaliser.
//   backward: beta lives in LDS: m[s] = beta[s] + e(t, label(s)) ping-pongs, beta_{t-1}[s] = logadd(logadd(m[s],
//             m[s + 1]), m[s + 2] if skip).  The occupancies exp(alpha + beta - score) of a frame are summed per label in
//             ONE order: the even (blank) states by plane of 256 states, the wave's xor tree, waves and planes ascending;
//             a label's chain of equal tokens by its head, ascending index, the blank's sum in front when the label is
//             `blank`.  The head stores the sum into a dense row occ[position & 1][label] in LDS: one owner per label,
//             a plain store, the same labels in every phase, so every other entry keeps the zero it got at the start.
//             A phase later the 256 streamer lanes read the raw row from the ring and the sums and store
//             exp(x - lse_t) - occ as the gradient row.
// No atomics on floats anywhere; the lane -> state map does not depend on PER, so neither do the bits.  Rows t >= T_b
// of the emissions are never read; rows t >= T_b of the gradient are zeroed by the utterance's own workgroup.  An
// utterance whose target does not fit, with a row without a finite entry, or without an alignment of finite score has
// loss +inf and a gradient slab of zeros.  Every store is a plain C++ store; there is no inline assembly.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

#include "kernels.h"
#include "pair_kernels.h"

namespace gtnx {
namespace {

constexpr int kWG = 512, kSweep = 256, kRing = kCtcStep16Ring, kPieces = kCtcStep16MaxC / 8 / 64;
constexpr float POS_INF = __builtin_inff();

__device__ __forceinline__ float to_f32(uint32_t h, int bf16) {
  return bf16 ? __uint_as_float(h << 16) : __half2float(__ushort_as_half(static_cast<unsigned short>(h)));
}

// round to nearest even
__device__ __forceinline__ uint32_t to_16(float f, int bf16) {
  if (bf16) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
  }
  return __half_as_ushort(__float2half_rn(f));
}

__device__ __forceinline__ void unpack8(const uint4& q, int bf16, float (&v)[8]) {
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = to_f32(w[i] & 0xffffu, bf16);
    v[2 * i + 1] = to_f32(w[i] >> 16, bf16);
  }
}

// a streamer wave's row on its way to the ring: piece lane + 64 k in rg[k]
struct Row {
  uint4 rg[kPieces];
  float lse;
};

__device__ __forceinline__ void issue_row(Row& r, const GTNX_G uint16_t* row, int np, int lane) {
  const GTNX_G uint4* p = reinterpret_cast<const GTNX_G uint4*>(row);
#pragma unroll
  for (int k = 0; k < kPieces; ++k)
    if (lane + 64 * k < np) r.rg[k] = p[lane + 64 * k];
}

// the row into its slot; LSE: its log-sum-exp as well (in every lane), `bad` when its maximum is not finite
template <bool LSE>
__device__ __forceinline__ float land_row(const Row& r, uint16_t* slot, int np, int lane, int bf16, bool& bad) {
  uint4* q = reinterpret_cast<uint4*>(slot);
  float mx = NEG_INF;
#pragma unroll
  for (int k = 0; k < kPieces; ++k)
    if (lane + 64 * k < np) {
      q[lane + 64 * k] = r.rg[k];
      if (LSE) {
        float v[8];
        unpack8(r.rg[k], bf16, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) mx = fmaxf(mx, v[i]);
      }
    }
  bad = false;
  if (!LSE) return 0.0f;
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
  bad = !(mx > NEG_INF && mx < POS_INF);
  if (bad) return 0.0f;
  float sum = 0.0f;
#pragma unroll
  for (int k = 0; k < kPieces; ++k)
    if (lane + 64 * k < np) {
      float v[8];
      unpack8(r.rg[k], bf16, v);
#pragma unroll
      for (int i = 0; i < 8; ++i) sum += expf(v[i] - mx);
    }
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
  return mx + logf(sum);
}

template <int PER, bool G32>
__global__ __launch_bounds__(kWG) void ctc_step16_kernel(CtcStep16Desc d) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  const int C = d.C, UM = max(d.max_u, 1), W = 2 * d.max_u + 5, bf16 = d.bf16;
  // (the order of ctc_step16_lds)
  uint16_t* s_ring = reinterpret_cast<uint16_t*>(s_raw);   // [kRing][C] raw rows
  float* s_occ = reinterpret_cast<float*>(s_raw + 2 * size_t(kRing) * C);  // [2][C]: a frame's occupancy sums per label
  float* s_a = s_occ + 2 * C;                                // [2][W]: alpha, then m; cells 0, 1 and S + 2, S + 3 are -inf
  float* s_g = s_a + 2 * W;                                  // [2][UM]: the occupancies of the odd states
  float* s_part = s_g + 2 * UM;                              // [2][16]: the waves' sums over the even states, per plane
  float* s_lse = s_part + 32;                                // [kRing]: the log-sum-exp of the ring's rows
  float* s_sc = s_lse + kRing;                               // [2]: the score
  int* s_nxt = reinterpret_cast<int*>(s_sc + 2);             // [UM]
  int* s_tok = s_nxt + UM;                                   // [UM]
  int* s_flag = s_tok + UM;                                  // [2]: the utterance is dead; a chain's head carries `blank`

  const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
  const bool sweeper = tid < kSweep;
  const int sw = wave - kSweep / 64;  // a streamer wave's row within a group
  const int64_t blk = blockIdx.x;
  const GTNX_G int* ent = d.stage + 4 * blk;
  const int U = ent[1], T = ent[2], S = 2 * U + 1, np = C >> 3;
  const GTNX_G int* target = d.labels + ent[0];
  const GTNX_G uint16_t* em = d.em + blk * d.T * C;
  GTNX_G float* alpha = d.alpha + blk * d.alpha_stride;
  GTNX_G float* rowlse = d.rowlse + blk * d.T;

  for (int i = tid; i < U; i += kWG) s_tok[i] = target[i];
  for (int i = tid; i < 2 * C; i += kWG) s_occ[i] = 0.0f;
  if (tid < 2) {
    s_flag[tid] = 0;
    for (int r = 0; r < 2; ++r) s_a[r * W + tid] = s_a[r * W + 2 + S + tid] = NEG_INF;
  }
  __syncthreads();

  // ---- what a sweeper lane keeps of its states s = tid + j * 256; the chains of equal tokens (ascending index, the
  // first one is the head)
  int lab[PER];
  bool skf[PER], skb[PER], head[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int s = tid + j * kSweep;
    lab[j] = d.blank;
    skf[j] = skb[j] = head[j] = false;
    if (sweeper && s < S && (s & 1)) {
      const int i = s >> 1, v = s_tok[i];
      lab[j] = v;
      skf[j] = i > 0 && s_tok[i - 1] != v;
      skb[j] = i + 1 < U && s_tok[i + 1] != v;
      bool seen = false;
      for (int q = 0; q < i && !seen; ++q) seen = s_tok[q] == v;
      int nx = -1;
      for (int q = i + 1; q < U && nx < 0; ++q)
        if (s_tok[q] == v) nx = q;
      s_nxt[i] = nx;
      head[j] = !seen;
      if (!seen && v == d.blank) s_flag[1] = 1;
    }
  }

  // ---- forward
  Row row;
  row.lse = 0.0f;
  if (!sweeper)
    for (int r = sw; r < kRing && r < T; r += 4) {
      bool bad;
      issue_row(row, em + int64_t(r) * C, np, lane);
      const float lse = land_row<true>(row, s_ring + r * C, np, lane, bf16, bad);
      if (lane == 0) {
        s_lse[r] = rowlse[r] = lse;
        if (bad) s_flag[0] = 1;
      }
    }
  __syncthreads();
  float norm = 0.0f;
  int cur = 0;
  for (int n = 0; n < T; ++n) {
    if (sweeper) {
      const uint16_t* e_row = s_ring + (n & (kRing - 1)) * C;
      const float* prev = s_a + cur * W;
      float* next = s_a + (cur ^ 1) * W;
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        const int s = tid + j * kSweep;
        if (s < S) {
          const float e = to_f32(e_row[lab[j]], bf16);
          float v;
          if (n == 0) {
            v = s < 2 ? e : NEG_INF;
          } else {
            float x = logadd(prev[2 + s], prev[1 + s]);
            if (skf[j]) x = logadd(x, prev[s]);
            v = x == NEG_INF ? NEG_INF : x + e;
          }
          next[2 + s] = v;
          alpha[int64_t(n) * d.NS + s] = v;
        }
      }
      if (tid == 0) norm += s_lse[n & (kRing - 1)];
      cur ^= 1;
    } else {
      if ((n & 3) == 3 && n + 5 + sw < T) issue_row(row, em + int64_t(n + 5 + sw) * C, np, lane);
      if ((n & 3) == 2 && n >= 6 && n + 2 + sw < T) {
        const int r = n + 2 + sw;
        bool bad;
        const float lse = land_row<true>(row, s_ring + (r & (kRing - 1)) * C, np, lane, bf16, bad);
        if (lane == 0) {
          s_lse[r & (kRing - 1)] = rowlse[r] = lse;
          if (bad) s_flag[0] = 1;
        }
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float* last = s_a + cur * W + 2;
    const float sc = S == 1 ? last[0] : logadd(last[S - 1], last[S - 2]);
    const bool ok = s_flag[0] == 0 && sc > NEG_INF && sc < POS_INF;
    s_sc[0] = sc;
    s_flag[0] = ok ? 0 : 1;
    d.loss[blk] = ok ? norm - sc : POS_INF;
  }
  __syncthreads();
  const bool dead = s_flag[0] != 0;
  const float sc = s_sc[0];
  const bool blank_in_chain = s_flag[1] != 0;

  // ---- the rows nothing is computed for: the pad rows, or the whole slab of a dead utterance
  constexpr int64_t GS = G32 ? 4 : 2;
  GTNX_G unsigned char* gslab = static_cast<GTNX_G unsigned char*>(d.grad) + blk * d.T * C * GS;
  {
    const int t0 = dead ? 0 : T;
    GTNX_G uint4* z = reinterpret_cast<GTNX_G uint4*>(gslab + int64_t(t0) * C * GS);
    const int64_t cnt = int64_t(d.T - t0) * C * GS / 16;
    for (int64_t i = tid; i < cnt; i += kWG) z[i] = make_uint4(0u, 0u, 0u, 0u);
  }
  if (dead) return;

  // ---- backward: position n is frame T - 1 - n
  if (!sweeper)
    for (int r = sw; r < kRing && r < T; r += 4) {
      bool bad;
      issue_row(row, em + int64_t(T - 1 - r) * C, np, lane);
      land_row<false>(row, s_ring + r * C, np, lane, bf16, bad);
      if (lane == 0) s_lse[r] = rowlse[T - 1 - r];
    }
  __syncthreads();
  float beta[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int s = tid + j * kSweep;
    beta[j] = s < S && s >= S - 2 ? 0.0f : NEG_INF;
  }
  // a position's occupancies and m = beta + e into the buffers `pp`
  auto emit = [&](int n, int pp) {
    const uint16_t* e_row = s_ring + (n & (kRing - 1)) * C;
    const GTNX_G float* a_row = alpha + int64_t(T - 1 - n) * d.NS;
    float* m = s_a + pp * W + 2;
    float* g = s_g + pp * UM;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int s = tid + j * kSweep;
      float ev = 0.0f;
      if (s < S) {
        const float e = to_f32(e_row[lab[j]], bf16);
        const float av = a_row[s];
        const float x = av > NEG_INF && beta[j] > NEG_INF ? expf(av + beta[j] - sc) : 0.0f;
        m[s] = beta[j] == NEG_INF ? NEG_INF : beta[j] + e;
        if (s & 1) g[s >> 1] = x;
        else ev = x;
      }
      for (int off = 32; off > 0; off >>= 1) ev += __shfl_xor(ev, off);
      if (lane == 0) s_part[pp * 16 + j * 4 + wave] = ev;
    }
  };
  if (sweeper) emit(0, 0);
  __syncthreads();
  int pp = 0;
  for (int n = 0; n <= T; ++n) {
    if (sweeper) {
      if (n < T) {
        const float* m = s_a + pp * W + 2;
        const float* g = s_g + pp * UM;
        float* occ = s_occ + (n & 1) * C;
        float evs = 0.0f;
        for (int q = 0; q < PER * 4; ++q) evs += s_part[pp * 16 + q];
#pragma unroll
        for (int j = 0; j < PER; ++j) {
          const int s = tid + j * kSweep;
          if (s < S) {
            float x = logadd(m[s], m[s + 1]);
            if (skb[j]) x = logadd(x, m[s + 2]);
            beta[j] = x;
            if (head[j]) {
              const int i = s >> 1;
              float sum = g[i];
              if (lab[j] == d.blank) sum = evs + sum;
              for (int q = s_nxt[i]; q >= 0; q = s_nxt[q]) sum += g[q];
              occ[lab[j]] = sum;
            }
          }
        }
        if (tid == 0 && !blank_in_chain) occ[d.blank] = evs;
        if (n + 1 < T) emit(n + 1, pp ^ 1);
        pp ^= 1;
      }
    } else {
      if (n >= 1) {  // the gradient row of position n - 1
        const int p = n - 1, t = T - 1 - p;
        const uint4* raw = reinterpret_cast<const uint4*>(s_ring + (p & (kRing - 1)) * C);
        const float4* occ = reinterpret_cast<const float4*>(s_occ + (p & 1) * C);
        const float lse = s_lse[p & (kRing - 1)];
        GTNX_G unsigned char* out = gslab + int64_t(t) * C * GS;
        for (int i = tid - kSweep; i < np; i += kWG - kSweep) {
          float v[8];
          unpack8(raw[i], bf16, v);
          const float4 o0 = occ[2 * i], o1 = occ[2 * i + 1];
          const float o[8] = {o0.x, o0.y, o0.z, o0.w, o1.x, o1.y, o1.z, o1.w};
#pragma unroll
          for (int k = 0; k < 8; ++k) v[k] = expf(v[k] - lse) - o[k];
          if (G32) {
            GTNX_G float4* o32 = reinterpret_cast<GTNX_G float4*>(out);
            o32[2 * i] = make_float4(v[0], v[1], v[2], v[3]);
            o32[2 * i + 1] = make_float4(v[4], v[5], v[6], v[7]);
          } else {
            uint4 w;
            w.x = to_16(v[0], bf16) | (to_16(v[1], bf16) << 16);
            w.y = to_16(v[2], bf16) | (to_16(v[3], bf16) << 16);
            w.z = to_16(v[4], bf16) | (to_16(v[5], bf16) << 16);
            w.w = to_16(v[6], bf16) | (to_16(v[7], bf16) << 16);
            reinterpret_cast<GTNX_G uint4*>(out)[i] = w;
          }
        }
      }
      if ((n & 3) == 3 && n + 5 + sw < T) {
        const int t = T - 1 - (n + 5 + sw);
        issue_row(row, em + int64_t(t) * C, np, lane);
        if (lane == 0) row.lse = rowlse[t];
      }
      if ((n & 3) == 2 && n >= 6 && n + 2 + sw < T) {
        const int r = n + 2 + sw;
        bool bad;
        land_row<false>(row, s_ring + (r & (kRing - 1)) * C, np, lane, bf16, bad);
        if (lane == 0) s_lse[r & (kRing - 1)] = row.lse;
      }
    }
    __syncthreads();
  }
}

template <int PER, bool G32>
void launch(const CtcStep16Desc& d, int count, hipStream_t st) {
  static std::atomic<uint64_t> done{0};
  if (gtnx_first_on_device first{done})
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(ctc_step16_kernel<PER, G32>),
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              int(ctc_step16_lds(kCtcStep16MaxC, kCtcStep16MaxU)));
  hipLaunchKernelGGL((ctc_step16_kernel<PER, G32>), dim3(static_cast<unsigned>(count)), dim3(kWG),
                     ctc_step16_lds(d.C, d.max_u), st, d);
}

}  // namespace

size_t ctc_step16_lds(int C, int max_u) {
  const size_t UM = size_t(max_u > 1 ? max_u : 1), W = 2 * size_t(max_u) + 5;
  return 2 * size_t(kRing) * C + 4 * (2 * size_t(C) + 2 * W + 2 * UM + 32 + kRing + 2) + 4 * (2 * UM + 2);
}

// the states a sweeper lane owns come from the CALL's longest target, so a call cut into slices launches one kernel
void launch_ctc_step16(const CtcStep16Desc& d, int count, bool grad32, hipStream_t st) {
  if (count <= 0) return;
  const int S = 2 * d.max_u + 1;
  if (S <= kSweep) grad32 ? launch<1, true>(d, count, st) : launch<1, false>(d, count, st);
  else if (S <= 2 * kSweep) grad32 ? launch<2, true>(d, count, st) : launch<2, false>(d, count, st);
  else grad32 ? launch<4, true>(d, count, st) : launch<4, false>(d, count, st);
}

}  // namespace gtnx
