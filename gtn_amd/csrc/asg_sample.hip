// asg_sample.hip -- N alignments of every chain of a padded [n][M][C] batch drawn from the posterior of the ASG model
// emissions o transitions, plus the merge of equal neighbours, results left on the device.  ASG frames are not
// independent, so the sample is exact only by forward filtering, backward sampling: a log-semiring forward sweep that
// keeps every alpha plane, then one categorical draw per frame from the last frame down, each given the label drawn
// for the frame after it.
//
// The contract.
//   model:   table [C + C * C]: table[c] the start score of label c, table[C + i * C + j] the score of moving from
//            label j to label i.  s(y) = table[y0] + x[0,y0] + sum_{t>=1} (table[C + y_t * C + y_{t-1}] + x[t,y_t]);
//            an alignment is drawn with probability exp(s(y) / temperature - logZ).
//   mass:    only finite entries carry mass.  A -inf, +inf or NaN emission or table entry makes every alignment
//            through it impossible, and it is never drawn.
//   no path: an utterance without an alignment of finite score, or with T_b = 0: every sample of it gets -1 rows,
//            length 0, logq -inf, and logz is -inf.  No output is ever NaN.
//   filter:  alpha_0[i] = (table[i] + x[0,i]) / temperature; alpha_t[i] = x[t,i] / temperature + logsumexp_j(table[C +
//            i * C + j] / temperature + alpha_{t-1}[j]), kept per frame in a rescaled form: the plane la_t = alpha_t -
//            L_t in float32, the running reference L_t (the sum of the per-frame maxima) in float64, as asg_full.hip
//            does.  logZ = L_{T-1} + log sum_i exp(la_{T-1}[i]).  A term more than ~87 below its frame's maximum is
//            dropped from the sums (float32 exp), as there.
//   draw:    backward, one uniform per (b, k, t).  Frame T_b - 1 has masses exp(la[j] - ref) over j, frame t below it,
//            given i = y_{t+1}, masses exp(la_t[j] + table[C + i * C + j] / temperature - ref), ref the largest
//            exponent.  Inverse CDF in label order: the smallest j whose cumulative mass over 0 .. j exceeds u * total,
//            total as the in-wave scan summed it; if rounding leaves none, the last label with mass.  A label without
//            mass is never returned.
//   random:  Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (t, b, k >> 2, 1), sample k uses output word
//            k & 3, u = (2 * (word >> 9) + 1) * 2^-24 (ctc_sample.hip has 0 in the last counter word).  b is the index
//            in the whole batch.  Nothing depends on launch geometry, strides, slicing, the other utterances' frame
//            counts or what pad rows hold.
//   logq:    the sum of log(mass_j / total) of the drawn labels, added in draw order (frame T_b - 1 first) from 0 in
//            float32.
//   collapse: equal neighbours merged; ASG has no blank.
//
// The launches.
//   prep (C > 128): rmax[i] = max_j table[C + i * C + j] / temperature over the finite entries and the transposed
//              et[j][i] = exp(table[C + i * C + j] / temperature - rmax[i]), padded with zeros to [roundup4(C)][256 *
//              ceil(C / 256)], once per call.
//   filter:    C <= 128: the shape of asg_full_forward_kernel -- one workgroup per utterance, thread (row, half) holds
//              its part of exp(W / temperature - rowmax) in registers, the vector q = exp(la) in LDS.  C > 128: one
//              workgroup of 256 * ceil(C / 256) threads carries kWideU utterances through the frames together, thread
//              tid owns row tid; it walks j over the columns, reads et[j][row] (coalesced, from L2) once for all the
//              utterances and q[u][j] from LDS as a broadcast: serial sums in j, no cross-lane reduction.  An utterance
//              past its own T_b stops storing; its arithmetic does not depend on its neighbours.
//   draw:      one wave per (b, k), lane l holds labels l * V .. l * V + V - 1 (V = 1 .. 16 by C) of plane row t and of
//              the table row of y_{t+1} in registers; the next plane row is loaded before this frame's label is known.
//              Lane-local running sums, one in-wave scan of the lane totals, the label by ballot.  The uniforms of 64
//              frames come from one Philox call per lane.  The label goes to the label rows, the term to scratch in
//              draw order.
//   collapse:  one wave per (b, k), the two passes of ctc_sample_collapse_kernel with keep = label != predecessor.
// Every store is a plain C++ store; there are no atomics and there is no inline assembly.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace gtnx {
namespace {

constexpr float NEG_INF = -__builtin_inff();
constexpr int kWideU = 4;  // utterances a wide filter workgroup carries

__device__ __forceinline__ bool finite(float v) { return __builtin_fabsf(v) < __builtin_inff(); }  // (NaN: false)
__device__ __forceinline__ float san(float v) { return finite(v) ? v : NEG_INF; }
// v / temperature of an entry that carries mass, else -inf
__device__ __forceinline__ float scaled(float v, float inv_tau) {
  if (!finite(v)) return NEG_INF;
  return san(v * inv_tau);
}
// (0 * inf would be NaN)
__device__ __forceinline__ float inverse(float tau) { return __builtin_fminf(1.0f / tau, 3.402823466e+38f); }

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

// Philox4x32-10 (Salmon et al., SC'11): ten rounds, the key bumped between them
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                              unsigned k1, unsigned (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

__device__ __forceinline__ int frames_of(const AsgSampleArgs& a, int b) {
  const int T = a.frames[b];
  return T < 0 ? 0 : (T > a.M ? a.M : T);  // (the engine has refused such counts: nothing outside the slab is addressed)
}

// ---- filter, C <= 2 * JH <= 128: thread (row r, half h) holds JH entries of row r of exp(W / temperature - rowmax)
template <int JH>
__global__ __launch_bounds__(4 * JH) void asg_sample_filter_kernel(AsgSampleArgs a) {
  constexpr int NT = 4 * JH, NW = NT / 64, NP = 2 * JH;
  __shared__ __attribute__((aligned(16))) float q[NP];
  __shared__ float slots[4];
  const int b = blockIdx.x, tid = threadIdx.x, r = tid >> 1, h = tid & 1, j0 = h * JH;
  const int C = a.C, M = a.M;
  const int T = frames_of(a, b);
  if (T == 0) {  // no frames: no path
    if (tid == 0 && a.logz) a.logz[b] = NEG_INF;
    return;
  }
  const float inv_tau = inverse(a.temperature);
  const GTNX_G float* em = a.em + int64_t(b) * M * C;
  const GTNX_G float* W = a.table + C;
  GTNX_G float* plane = a.planes + int64_t(b) * M * C;
  const bool row = r < C;

  float E[JH];
  float rm = NEG_INF;
#pragma unroll
  for (int k = 0; k < JH; ++k) {
    const int j = j0 + k;
    E[k] = (row && j < C) ? scaled(W[int64_t(r) * C + j], inv_tau) : NEG_INF;
    rm = fmaxf(rm, E[k]);
  }
  rm = fmaxf(rm, __shfl_xor(rm, 1));
  if (rm == NEG_INF) rm = 0.0f;  // (a label nothing leads to: the row is all zeros)
#pragma unroll
  for (int k = 0; k < JH; ++k) E[k] = expf(E[k] - rm);
  for (int k = tid; k < NP; k += NT) q[k] = 0.0f;  // (entries [C, NP) stay zero: the rows' tails multiply them)

  double L = 0.0;
  float av = row ? scaled(san(a.table[r]) + san(em[r]), inv_tau) : NEG_INF;
  float qv = 0.0f;
  for (int t = 0;;) {
    const float m = block_reduce<NW, true>(av, slots);
    const float la = av - (m == NEG_INF ? 0.0f : m);
    L += double(m);
    qv = expf(la);
    if (row && h == 0) {
      q[r] = qv;
      plane[int64_t(t) * C + r] = la;
    }
    if (++t >= T) break;
    const float e = row ? scaled(em[int64_t(t) * C + r], inv_tau) : NEG_INF;
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
  if (tid == 0 && a.logz) a.logz[b] = sum > 0.0f ? float(L + double(logf(sum))) : NEG_INF;
}

// ---- prep, C > 128: one workgroup per column i of et (row i of the table), pads included
__global__ __launch_bounds__(256) void asg_sample_prep_kernel(AsgSampleArgs a, int Cp) {
  __shared__ float slots[4];
  const int i = blockIdx.x, tid = threadIdx.x;
  const int C = a.C, Cq = (C + 3) & ~3;
  if (i >= C) {
    for (int j = tid; j < Cq; j += 256) a.et[int64_t(j) * Cp + i] = 0.0f;
    if (tid == 0) a.rmax[i] = 0.0f;
    return;
  }
  const float inv_tau = inverse(a.temperature);
  const GTNX_G float* W = a.table + C + int64_t(i) * C;
  float rm = NEG_INF;
  for (int j = tid; j < C; j += 256) rm = fmaxf(rm, scaled(W[j], inv_tau));
  rm = block_reduce<4, true>(rm, slots);
  if (rm == NEG_INF) rm = 0.0f;
  for (int j = tid; j < Cq; j += 256) a.et[int64_t(j) * Cp + i] = j < C ? expf(scaled(W[j], inv_tau) - rm) : 0.0f;
  if (tid == 0) a.rmax[i] = rm;
}

// ---- filter, C > 128: 256 * NQ threads carry U utterances; thread tid owns row tid
template <int NQ, int U>
__global__ __launch_bounds__(256 * NQ) void asg_sample_filter_wide_kernel(AsgSampleArgs a) {
  constexpr int Cp = 256 * NQ, NW = 4 * NQ;
  __shared__ __attribute__((aligned(16))) float q[U][1024];
  __shared__ float slots[U][NW];
  __shared__ float slots2[NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = a.C, M = a.M, Cq = (C + 3) & ~3;
  const float inv_tau = inverse(a.temperature);
  const bool row = tid < C;
  int T[U], Tmax = 0;
  int64_t base[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int b = blockIdx.x * U + u;
    T[u] = b < a.n ? frames_of(a, b) : 0;
    base[u] = int64_t(b < a.n ? b : 0) * M * C;
    Tmax = T[u] > Tmax ? T[u] : Tmax;
    if (tid == 0 && b < a.n && T[u] == 0 && a.logz) a.logz[b] = NEG_INF;  // no frames: no path
  }
  if (Tmax == 0) return;
  for (int i = tid; i < U * 1024; i += Cp) (&q[0][0])[i] = 0.0f;  // (entries [C, Cq) stay zero)
  const float rm = row ? a.rmax[tid] : 0.0f;
  float av[U], qv[U];
  double L[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    av[u] = (row && T[u] > 0) ? scaled(san(a.table[tid]) + san(a.em[base[u] + tid]), inv_tau) : NEG_INF;
    qv[u] = 0.0f;
    L[u] = 0.0;
  }
  for (int t = 0;;) {
    // the frame's maximum of every utterance
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float x = wave_max(av[u]);
      if (lane == 0) slots[u][wave] = x;
    }
    __syncthreads();  // (every thread is through the sums that read q)
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (t >= T[u]) continue;  // (uniform over the workgroup)
      float m = slots[u][0];
#pragma unroll
      for (int w = 1; w < NW; ++w) m = fmaxf(m, slots[u][w]);
      const float la = av[u] - (m == NEG_INF ? 0.0f : m);
      L[u] += double(m);
      qv[u] = expf(la);
      if (row) {
        q[u][tid] = qv[u];
        a.planes[base[u] + int64_t(t) * C + tid] = la;
      }
      if (t == T[u] - 1) {  // the utterance's last frame: logZ
        const float s = wave_sum(row ? qv[u] : 0.0f);
        if (lane == 0) slots2[wave] = s;
        __syncthreads();
        if (tid == 0 && a.logz) {
          float sum = slots2[0];
#pragma unroll
          for (int w = 1; w < NW; ++w) sum += slots2[w];
          a.logz[blockIdx.x * U + u] = sum > 0.0f ? float(L[u] + double(logf(sum))) : NEG_INF;
        }
        __syncthreads();
      }
    }
    if (++t >= Tmax) break;
    float e[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
      e[u] = (row && t < T[u]) ? scaled(a.em[base[u] + int64_t(t) * C + tid], inv_tau) : NEG_INF;
    __syncthreads();  // (q of this frame is whole; slots are free)
    float s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) s[u] = 0.0f;
    const GTNX_G float* et = a.et + tid;
#pragma unroll 2
    for (int j = 0; j < Cq; j += 4) {
      const float E0 = et[int64_t(j) * Cp], E1 = et[int64_t(j + 1) * Cp], E2 = et[int64_t(j + 2) * Cp],
                  E3 = et[int64_t(j + 3) * Cp];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float4 v = *reinterpret_cast<const float4*>(&q[u][j]);
        s[u] = fmaf(E0, v.x, s[u]);
        s[u] = fmaf(E1, v.y, s[u]);
        s[u] = fmaf(E2, v.z, s[u]);
        s[u] = fmaf(E3, v.w, s[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) av[u] = s[u] > 0.0f ? logf(s[u]) + rm + e[u] : NEG_INF;
  }
}

// ---- draw: one wave per (b, k), lane l holds labels l * V .. l * V + V - 1
template <int V>
__global__ __launch_bounds__(64) void asg_sample_draw_kernel(AsgSampleArgs a) {
  const int pair = blockIdx.x, l = threadIdx.x;
  const int b = pair / a.N, k = pair - b * a.N;
  const int C = a.C, M = a.M;
  const int T = frames_of(a, b);
  if (T == 0) return;  // (the collapse writes the rows of an utterance without frames)
  const float inv_tau = inverse(a.temperature);
  const GTNX_G float* plane = a.planes + int64_t(b) * M * C;
  const GTNX_G float* W = a.table + C;
  GTNX_G int* lrow = a.labels + int64_t(pair) * a.label_stride;
  GTNX_G float* trow = a.terms + int64_t(pair) * M;
  const int j0 = l * V;
  float cur[V], nxt[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    cur[v] = j0 + v < C ? plane[int64_t(T - 1) * C + j0 + v] : NEG_INF;
    nxt[v] = NEG_INF;
  }
  int prev = -1;
  unsigned mine = 0;  // the word of frame t0 - l, t0 the first frame of the block of 64 in draw order
  for (int t = T - 1; t >= 0; --t) {
    const int idx = T - 1 - t;
    if ((idx & 63) == 0) {
      unsigned word[4];
      philox4x32_10(unsigned(t - l), unsigned(a.b0 + b), unsigned(k >> 2), 1u, a.seed_lo, a.seed_hi, word);
      const int sel = k & 3;
      mine = sel == 0 ? word[0] : (sel == 1 ? word[1] : (sel == 2 ? word[2] : word[3]));  // (lanes past frame 0: unused)
    }
    const unsigned w = __shfl(mine, idx & 63);
    const float u = float(2u * (w >> 9) + 1u) * 5.9604644775390625e-08f;  // (exact: 24 bits, then 2^-24)
    if (t > 0) {
#pragma unroll
      for (int v = 0; v < V; ++v)
        if (j0 + v < C) nxt[v] = plane[int64_t(t - 1) * C + j0 + v];
    }
    float x[V];
    float mx = NEG_INF;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      x[v] = cur[v];
      if (prev >= 0 && j0 + v < C) x[v] += scaled(W[int64_t(prev) * C + j0 + v], inv_tau);
      // (a plane entry is finite or -inf and the table's term is finite or -inf: no NaN)
      mx = fmaxf(mx, x[v]);
    }
    mx = wave_max(mx);
    if (mx == NEG_INF) {  // no path (only the last frame of an utterance without one comes here)
      for (int i = l; i < T; i += 64) {
        lrow[i] = -1;
        trow[i] = 0.0f;
      }
      return;
    }
    float ms[V], c[V];  // the masses and their running sums within the lane
    float run = 0.0f;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      ms[v] = x[v] > NEG_INF ? expf(x[v] - mx) : 0.0f;
      run += ms[v];
      c[v] = run;
    }
    float incl = run;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float o = __shfl_up(incl, off);
      if (l >= off) incl += o;
    }
    const float total = __shfl(incl, 63);
    const float up = __shfl_up(incl, 1);
    const float before = l == 0 ? 0.0f : up;  // the mass of the lanes before
    const float target = u * total;
    // the first label of the lane that has mass and whose cumulative mass exceeds the target (the scan's sums and the
    // lanes' own may differ in the last bit: asking for mass keeps a label without it from ever being returned)
    int pick = -1;
    float xp = 0.0f;
#pragma unroll
    for (int v = V - 1; v >= 0; --v)
      if (ms[v] > 0.0f && before + c[v] > target) {
        pick = j0 + v;
        xp = x[v];
      }
    unsigned long long at = __builtin_amdgcn_ballot_w64(pick >= 0);
    if (at == 0) {  // rounding left none: the last label with mass
#pragma unroll
      for (int v = 0; v < V; ++v)
        if (ms[v] > 0.0f) {
          pick = j0 + v;
          xp = x[v];
        }
      at = __builtin_amdgcn_ballot_w64(pick >= 0);
      const int last = 63 - __builtin_clzll(at);  // (not empty: mx is finite)
      pick = __shfl(pick, last);
      xp = __shfl(xp, last);
    } else {
      const int first = __builtin_ctzll(at);
      pick = __shfl(pick, first);
      xp = __shfl(xp, first);
    }
    if (l == 0) {
      lrow[t] = pick;
      trow[idx] = (xp - mx) - logf(total);
    }
    prev = pick;
#pragma unroll
    for (int v = 0; v < V; ++v) cur[v] = nxt[v];
  }
}

// ---- collapse: one wave per (b, k)
__global__ __launch_bounds__(64) void asg_sample_collapse_kernel(AsgSampleArgs a) {
  const int pair = blockIdx.x, l = threadIdx.x;
  const int b = pair / a.N;
  const int M = a.M;
  const int T = frames_of(a, b);
  GTNX_G int* lrow = a.labels + int64_t(pair) * a.label_stride;
  GTNX_G int* crow = a.tokens + int64_t(pair) * a.row_stride;
  const GTNX_G float* trow = a.terms + int64_t(pair) * M;
  // ---- pass 1: the log-probability, in draw order, and whether every frame found a label
  float logq = 0.0f;
  bool none = T == 0;  // (a chain without frames has no path)
  for (int base = 0; base < T; base += 64) {
    const int idx = base + l;
    const float tv = idx < T ? trow[idx] : 0.0f;
    const int lab = idx < T ? lrow[idx] : 0;
    none |= __builtin_amdgcn_ballot_w64(lab < 0) != 0;
    const int cnt = T - base < 64 ? T - base : 64;
    for (int k = 0; k < cnt; ++k) logq += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tv), k));
  }
  if (none) {  // no path: every entry of every row -1
    for (int i = l; i < M; i += 64) {
      crow[i] = -1;
      if (a.fill_labels) lrow[i] = -1;
    }
    if (l == 0) {
      a.lengths[pair] = 0;
      if (a.logq) a.logq[pair] = NEG_INF;
    }
    return;
  }
  if (a.fill_labels)
    for (int i = T + l; i < M; i += 64) lrow[i] = -1;
  if (l == 0 && a.logq) a.logq[pair] = logq;
  // ---- pass 2: merge equal neighbours (labels of a path are >= 0, so -1 stands for "no predecessor")
  int count = 0, carry = -1;
  for (int base = 0; base < T; base += 64) {
    const int idx = base + l;
    const int v = idx < T ? lrow[idx] : -1;
    const int up = __shfl_up(v, 1);
    const int before = l == 0 ? carry : up;
    const bool keep = idx < T && v != before;
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
    const int pos = count + __builtin_popcountll(mask & ((1ull << l) - 1ull));
    if (keep) crow[pos] = v;  // pos <= idx < M
    count += __builtin_popcountll(mask);
    carry = __builtin_amdgcn_readlane(v, 63);
  }
  for (int i = count + l; i < M; i += 64) crow[i] = -1;
  if (l == 0) a.lengths[pair] = count;
}

template <int NQ>
void launch_wide(const AsgSampleArgs& a, hipStream_t st) {
  const unsigned groups = static_cast<unsigned>((a.n + kWideU - 1) / kWideU);
  hipLaunchKernelGGL((asg_sample_filter_wide_kernel<NQ, kWideU>), dim3(groups), dim3(256 * NQ), 0, st, a);
}

template <int V>
void launch_draw(const AsgSampleArgs& a, hipStream_t st) {
  // (n * N fits an int: the engine has refused the rest)
  hipLaunchKernelGGL(asg_sample_draw_kernel<V>, dim3(static_cast<unsigned>(a.n) * static_cast<unsigned>(a.N)), dim3(64),
                     0, st, a);
}

}  // namespace

int asg_sample_et_stride(int C) { return C > kAsgSampleRegisterC ? 256 * ((C + 255) / 256) : 0; }

void launch_asg_sample(const AsgSampleArgs& a, int which, hipStream_t st) {
  if (a.C < 1 || a.C > kAsgSampleMaxC) return;  // (the engine has refused such a call)
  const int Cp = asg_sample_et_stride(a.C);
  if (which == 0) {  // once per call, whatever the slices
    if (Cp > 0) hipLaunchKernelGGL(asg_sample_prep_kernel, dim3(static_cast<unsigned>(Cp)), dim3(256), 0, st, a, Cp);
    return;
  }
  if (a.n <= 0 || a.N <= 0) return;
  if (which == 1) {  // (a batch without rows: every utterance takes the T_b = 0 exit)
    const unsigned n = static_cast<unsigned>(a.n);
    if (a.C <= 32) hipLaunchKernelGGL(asg_sample_filter_kernel<16>, dim3(n), dim3(64), 0, st, a);
    else if (a.C <= 64) hipLaunchKernelGGL(asg_sample_filter_kernel<32>, dim3(n), dim3(128), 0, st, a);
    else if (a.C <= 128) hipLaunchKernelGGL(asg_sample_filter_kernel<64>, dim3(n), dim3(256), 0, st, a);
    else if (Cp == 256) launch_wide<1>(a, st);
    else if (Cp == 512) launch_wide<2>(a, st);
    else if (Cp == 768) launch_wide<3>(a, st);
    else launch_wide<4>(a, st);
    return;
  }
  if (which == 2) {
    if (a.C <= 64) launch_draw<1>(a, st);
    else if (a.C <= 128) launch_draw<2>(a, st);
    else if (a.C <= 256) launch_draw<4>(a, st);
    else if (a.C <= 512) launch_draw<8>(a, st);
    else launch_draw<16>(a, st);
    return;
  }
  hipLaunchKernelGGL(asg_sample_collapse_kernel, dim3(static_cast<unsigned>(a.n) * static_cast<unsigned>(a.N)), dim3(64),
                     0, st, a);
}

}  // namespace gtnx
