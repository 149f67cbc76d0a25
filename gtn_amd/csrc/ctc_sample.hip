// ctc_sample.hip -- N alignments of every chain of a padded [n][M][C] batch drawn from its frame posteriors, plus the
// CTC collapse, results left on the device (an exact sample of P(y | x): the frames of a CTC alignment are independent).
//
// The contract.
//   mass:    only finite entries carry mass.  -inf, +inf and NaN are never chosen and are left out of Z.  A frame
//            without a finite entry, or T_b = 0, leaves the utterance without a path: every sample of it gets -1 rows,
//            length 0, logq -inf (what linear_decode.hip does).  No output is ever NaN.
//   draw:    inverse CDF in label order.  With u the uniform of (b, k, t), the label is the smallest c whose cumulative
//            mass over labels 0 .. c exceeds u * Z; if rounding leaves none, the last label with mass.  A label without
//            mass is never returned.
//   random:  Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (t, b, k >> 2, 0), sample k uses output word
//            k & 3, u = (2 * (word >> 9) + 1) * 2^-24: strictly inside (0, 1) and exact in float32.  Nothing depends on
//            launch geometry, strides, slicing, the other utterances' frame counts or what pad rows hold.
//   logq:    sum_t (x[b,t,c_t] / temperature - log Z[b,t]), added in frame order from 0 in float32.
//
// Two launches.
//   rows:      the shape of linear_decode_rows_kernel.  A group of LPR lanes (8 / 16 / 32 / 64, by C) owns one row:
//              scalar head up to the next 16-byte boundary, 16-byte loads, scalar tail.  Walk 1: the maximum over the
//              finite entries and the last of them.  Walk 2: Z = sum exp((x - max) / temperature), each mass good to an
//              ulp of float32, added in float64 (the maximum contributes exactly 1, so log Z keeps its relative
//              accuracy on a peaked row).  Walk 3 (the row is in cache), in tiles of LPR * 4 consecutive labels,
//              float32 masses: an in-group prefix scan and
//              a running carry give the cumulative mass in label order; every lane holds the four targets u_k * Z of
//              one Philox call, and a target finds its label by ballot within the tile where the carry passes it.  More
//              than 4 * LPR samples take walk 3 again.  HBM traffic stays one read of the rows that count.  The label
//              and the term x / temperature - log Z of each (b, k, t) go to the label rows and to scratch.
//   collapse:  one wave per (b, k), the two passes of linear_decode_collapse_kernel.  Pass 1 adds the terms in frame
//              order (lane by lane through readlane: the association is the contract) and looks for a label of -1.
//              Pass 2 takes 64 frames at a time: keep = label != predecessor && label != blank, a ballot and a prefix
//              count give the position, the predecessor of lane 0 is carried from the block before.  Then the -1
//              entries.
// Every store is a plain C++ store; there are no atomics and there is no inline assembly.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace gtnx {
namespace {

constexpr float NEG_INF = -__builtin_inff();
constexpr int kRowBlock = 256;  // threads of a row-kernel workgroup
constexpr int kRowTrips = 4;    // rows each lane group takes, one after the other

__device__ __forceinline__ bool finite(float v) { return __builtin_fabsf(v) < __builtin_inff(); }  // (NaN: false)

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

// the bits of this lane group in a ballot of the wave
template <int LPR>
__device__ __forceinline__ unsigned long long group_bits(unsigned long long wave, int shift) {
  if (LPR == 64) return wave;
  return (wave >> shift) & ((1ull << LPR) - 1ull);
}

// the four samples a lane owns during one walk 3
struct Draw {
  float target[4];  // u_k * Z
  int lab[4];
  bool pend[4];
  float carry;      // the cumulative mass before the tile
};

// one tile of walk 3: lane `lane` holds the masses m0 .. m3 of labels c .. c + 3 (0 where there is none), bit j of
// `fin` says that entry j is finite.  Everything below is uniform over the lane group.
template <int LPR>
__device__ __forceinline__ void tile(Draw& d, int lane, int shift, float m0, float m1, float m2, float m3, unsigned fin,
                                     int c) {
  float incl = ((m0 + m1) + m2) + m3;
#pragma unroll
  for (int off = 1; off < LPR; off <<= 1) {
    const float o = __shfl_up(incl, off, LPR);
    if (lane >= off) incl += o;
  }
  float excl = __shfl_up(incl, 1, LPR);
  excl = lane == 0 ? d.carry : excl + d.carry;
  incl += d.carry;
  // a lane without a finite entry is never the place of a label; `hi`: the furthest a lane with one reaches
  const float qual = fin ? incl : -1.0f;
  float hi = qual;
#pragma unroll
  for (int off = LPR / 2; off >= 1; off >>= 1) hi = __builtin_fmaxf(hi, __shfl_xor(hi, off, LPR));
  const float c0 = excl + m0, c1 = c0 + m1, c2 = c1 + m2;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    unsigned long long mask = group_bits<LPR>(__builtin_amdgcn_ballot_w64(d.pend[j] && d.target[j] < hi), shift);
    while (mask) {
      const int owner = __builtin_ctzll(mask);
      mask &= mask - 1ull;
      const float tg = __shfl(d.target[j], owner, LPR);
      // (not empty: the lane that holds `hi` is in it; were it, the sample would stay without a label and take the
      //  row's last one below)
      const unsigned long long at = group_bits<LPR>(__builtin_amdgcn_ballot_w64(qual > tg), shift);
      const int first = at ? __builtin_ctzll(at) : 0;
      // the first finite entry of the lane whose cumulative mass exceeds the target, else its last finite entry
      int pick = fin ? c + (31 - __builtin_clz(fin)) : -1;
      if ((fin & 4u) && c2 > tg) pick = c + 2;
      if ((fin & 2u) && c1 > tg) pick = c + 1;
      if ((fin & 1u) && c0 > tg) pick = c;
      const int res = __shfl(pick, first, LPR);
      if (lane == owner) {
        d.lab[j] = at ? res : -1;
        d.pend[j] = false;
      }
    }
  }
  d.carry = __shfl(incl, LPR - 1, LPR);
}

template <int LPR>
__global__ __launch_bounds__(kRowBlock) void ctc_sample_rows_kernel(CtcSampleArgs a) {
  constexpr int GROUPS = kRowBlock / LPR;  // rows in flight per workgroup
  const int b = blockIdx.y;
  int T = a.frames[b];
  T = T < 0 ? 0 : (T > a.M ? a.M : T);  // (the engine has refused such counts: nothing outside the slab is addressed)
  const int C = a.C, N = a.N;
  const int lane = threadIdx.x % LPR, group = threadIdx.x / LPR;
  const int shift = (threadIdx.x & 63) / LPR * LPR;
  const int t0 = blockIdx.x * (GROUPS * kRowTrips);
  // (0 * inf would be NaN where x equals the maximum)
  const float inv_tau = __builtin_fminf(1.0f / a.temperature, 3.402823466e+38f);
  const double inv_tau_d = 1.0 / double(a.temperature);
  for (int trip = 0; trip < kRowTrips; ++trip) {
    const int t = t0 + trip * GROUPS + group;
    if (t >= T) break;  // (whole lane groups leave together: the shuffles below stay inside a group)
    const GTNX_G float* p = a.em + (int64_t(b) * a.M + t) * C;
    int head = int((4 - ((reinterpret_cast<uintptr_t>(p) >> 2) & 3)) & 3);
    if (head > C) head = C;
    const GTNX_G gtnx_f4* v = reinterpret_cast<const GTNX_G gtnx_f4*>(p + head);
    const int nv = (C - head) >> 2;
    const int done = head + 4 * nv;
    const int tail = C - done;
    const int64_t lbase = int64_t(b) * N * a.label_stride + t;
    const int64_t tbase = int64_t(b) * N * a.M + t;
    // ---- walk 1: the maximum over the finite entries, and the last of them
    float m = NEG_INF;
    int lastfin = -1;
    auto seen = [&](float x, int c) {
      if (finite(x)) {
        m = __builtin_fmaxf(m, x);
        lastfin = c;  // (a lane's labels rise)
      }
    };
    if (lane < head) seen(p[lane], lane);
    for (int i = lane; i < nv; i += LPR) {
      const gtnx_f4 x = v[i];
      const int c = head + 4 * i;
      seen(x.x, c);
      seen(x.y, c + 1);
      seen(x.z, c + 2);
      seen(x.w, c + 3);
    }
    if (lane < tail) seen(p[done + lane], done + lane);
#pragma unroll
    for (int off = LPR / 2; off >= 1; off >>= 1) {
      m = __builtin_fmaxf(m, __shfl_xor(m, off, LPR));
      const int ol = __shfl_xor(lastfin, off, LPR);
      lastfin = ol > lastfin ? ol : lastfin;
    }
    if (lastfin < 0) {  // no finite entry: no path through this frame
      for (int k = lane; k < N; k += LPR) {
        a.labels[lbase + int64_t(k) * a.label_stride] = -1;
        a.terms[tbase + int64_t(k) * a.M] = 0.0f;
      }
      continue;
    }
    // (x - m is <= 0; kept finite, so that a product with a flushed 1 / temperature is 0 and never NaN)
    auto arg = [&](float x) { return __builtin_fmaxf(x - m, -3.402823466e+38f) * inv_tau; };
    auto mass = [&](float x) { return finite(x) ? __expf(arg(x)) : 0.0f; };
    // ---- walk 2: Z (relative to the maximum, whose mass is exactly 1)
    double zs = 0.0;
    // (the argument in float64, its float32 part through expf, the rest to first order: a mass keeps the relative
    //  accuracy of expf however far below the maximum it lies, so log Z is good to a few ulp of log Z on a peaked row)
    auto zmass = [&](float x) {
      if (!finite(x)) return 0.0;
      const double ad = (double(x) - double(m)) * inv_tau_d;
      const float hi = float(ad);
      if (!(hi > -110.0f)) return 0.0;  // (below the smallest float32: no mass; also keeps the product off 0 * inf)
      const double e = double(expf(hi));
      return e + e * (ad - double(hi));
    };
    if (lane < head) zs += zmass(p[lane]);
    for (int i = lane; i < nv; i += LPR) {
      const gtnx_f4 x = v[i];
      zs += (zmass(x.x) + zmass(x.y)) + (zmass(x.z) + zmass(x.w));
    }
    if (lane < tail) zs += zmass(p[done + lane]);
#pragma unroll
    for (int off = LPR / 2; off >= 1; off >>= 1) zs += __shfl_xor(zs, off, LPR);
    const float zf = float(zs);
    const double log_zs = log(zs);
    // ---- walk 3, once per 4 * LPR samples
    for (int g0 = 0; 4 * g0 < N; g0 += LPR) {
      const int g = g0 + lane;  // this lane's Philox call: samples 4 g .. 4 g + 3
      unsigned word[4];
      philox4x32_10(unsigned(t), unsigned(a.b0 + b), unsigned(g), 0u, a.seed_lo, a.seed_hi, word);
      Draw d;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float u = float(2u * (word[j] >> 9) + 1u) * 5.9604644775390625e-08f;  // (exact: 24 bits, then 2^-24)
        d.target[j] = u * zf;
        d.lab[j] = -1;
        d.pend[j] = 4 * g + j < N;
      }
      d.carry = 0.0f;
      if (head > 0) {
        const bool in = lane < head;
        const float x = in ? p[lane] : NEG_INF;
        tile<LPR>(d, lane, shift, mass(x), 0.0f, 0.0f, 0.0f, finite(x) ? 1u : 0u, lane);
      }
      for (int i0 = 0; i0 < nv; i0 += LPR) {
        const int i = i0 + lane;
        gtnx_f4 x = {NEG_INF, NEG_INF, NEG_INF, NEG_INF};
        if (i < nv) x = v[i];
        const unsigned fin = (finite(x.x) ? 1u : 0u) | (finite(x.y) ? 2u : 0u) | (finite(x.z) ? 4u : 0u) |
                             (finite(x.w) ? 8u : 0u);
        tile<LPR>(d, lane, shift, mass(x.x), mass(x.y), mass(x.z), mass(x.w), fin, head + 4 * i);
      }
      if (tail > 0) {
        const bool in = lane < tail;
        const float x = in ? p[done + lane] : NEG_INF;
        tile<LPR>(d, lane, shift, mass(x), 0.0f, 0.0f, 0.0f, finite(x) ? 1u : 0u, done + lane);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = 4 * g + j;
        if (k < N) {
          const int c = d.lab[j] < 0 ? lastfin : d.lab[j];  // (rounding left none: the last label with mass)
          const double term = (double(p[c]) - double(m)) * inv_tau_d - log_zs;
          a.labels[lbase + int64_t(k) * a.label_stride] = c;
          a.terms[tbase + int64_t(k) * a.M] = float(term);
        }
      }
    }
  }
}

__global__ __launch_bounds__(64) void ctc_sample_collapse_kernel(CtcSampleArgs a) {
  const int pair = blockIdx.x, l = threadIdx.x;
  const int b = pair / a.N;
  const int M = a.M;
  int T = a.frames[b];
  T = T < 0 ? 0 : (T > M ? M : T);
  GTNX_G int* lrow = a.labels + int64_t(pair) * a.label_stride;
  GTNX_G int* crow = a.tokens + int64_t(pair) * a.row_stride;
  const GTNX_G float* trow = a.terms + int64_t(pair) * M;
  // ---- pass 1: the log-probability, in frame order, and whether every frame found a label
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
  // ---- pass 2: merge repeats, drop blanks (labels of a path are >= 0, so -1 stands for "no predecessor")
  int count = 0, carry = -1;
  for (int base = 0; base < T; base += 64) {
    const int idx = base + l;
    const int v = idx < T ? lrow[idx] : -1;
    const int up = __shfl_up(v, 1);
    const int before = l == 0 ? carry : up;
    const bool keep = idx < T && v != before && v != a.blank;
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
    const int pos = count + __builtin_popcountll(mask & ((1ull << l) - 1ull));
    if (keep) crow[pos] = v;  // pos <= idx < M
    count += __builtin_popcountll(mask);
    carry = __builtin_amdgcn_readlane(v, 63);
  }
  for (int i = count + l; i < M; i += 64) crow[i] = -1;
  if (l == 0) a.lengths[pair] = count;
}

template <int LPR>
void launch_rows(const CtcSampleArgs& a, hipStream_t st) {
  const int per_block = (kRowBlock / LPR) * kRowTrips;
  const unsigned gx = static_cast<unsigned>((a.M + per_block - 1) / per_block);
  // (grid.y holds at most 65535 utterances per launch)
  for (int b0 = 0; b0 < a.n; b0 += 65535) {
    CtcSampleArgs s = a;
    const int nb = a.n - b0 < 65535 ? a.n - b0 : 65535;
    s.em += int64_t(b0) * a.M * a.C;
    s.frames += b0;
    s.labels += int64_t(b0) * a.N * a.label_stride;
    s.terms += int64_t(b0) * a.N * a.M;
    s.b0 = a.b0 + b0;
    hipLaunchKernelGGL(ctc_sample_rows_kernel<LPR>, dim3(gx, static_cast<unsigned>(nb)), dim3(kRowBlock), 0, st, s);
  }
}

}  // namespace

void launch_ctc_sample(const CtcSampleArgs& a, int which, hipStream_t st) {
  if (a.n <= 0 || a.N <= 0) return;
  if (which == 0) {
    if (a.M <= 0) return;
    // lanes per row: every lane of a group gets at least one 16-byte load where the row has that many
    if (a.C <= 32) launch_rows<8>(a, st);
    else if (a.C <= 64) launch_rows<16>(a, st);
    else if (a.C <= 128) launch_rows<32>(a, st);
    else launch_rows<64>(a, st);
    return;
  }
  // (n * N fits an int: the engine has refused the rest)
  hipLaunchKernelGGL(ctc_sample_collapse_kernel, dim3(static_cast<unsigned>(a.n) * static_cast<unsigned>(a.N)), dim3(64),
                     0, st, a);
}

}  // namespace gtnx
