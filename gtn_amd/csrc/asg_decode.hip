// asg_decode.hip -- viterbiPath(emissions_b o transitions) of a whole batch with the results left on the device
// (the decode an ASG model runs at inference).
//
// The max-plus sweeps of maxplus.hip store every alpha[t] plane of a group, and maxplus_path_kernel re-derives the
// winning arc of each visited state from those planes (no back-pointers).  The decode of utterance b at its OWN length
// T_b is therefore a back-trace that starts from row T_b of the planes ONE shared sweep over the padded batch has
// written: nothing of the sweep changes, and a batch with B distinct lengths costs one chain of launches, not B.
//
// One wave per utterance.  Start: the maximum of alpha[T_b][b][.] over the accept nodes, of equal maxima the first in
// accept_list order (lazy_final_kernel's rule) -- that value is the score; lazy_final's score / best (row M) are not
// used.  Step t = T_b .. 1: x = alpha[t-1][s] + w + e in that association over the node's real in-row, the comparison
// maxplus_path_kernel makes; of equal maxima the smallest source node wins (LazyGroup::tie_by_node, the order the
// reference's queue visits the sources of an ASG transitions graph: ops_lazy.cpp dense_ties_by_node_order).  Rows are
// staged exactly as there: alpha[t-1] / the emission row in LDS, requested two steps ahead, counted waits.
//
// Outputs go straight into the caller's rows, 64 entries at a time: labels[b][t] for t < T_b and -1 from T_b to the
// row's width M; scores[b]; optionally the collapsed sequence (runs of equal consecutive frame labels merged), -1 from
// its length to M, and the length.  The trace runs back to front, so the collapsed positions are known only at its
// end: a second pass of the same wave over its own label row (every lane re-reads the entries IT stored) with a ballot
// and a prefix count per 64 entries.  Without an accepting path (T_b = 0, or alpha[T_b] = -inf on every accept node):
// every entry -1, score -inf, length 0.
//
// Pad rows.  The sweep runs all M rows of every slab and so reads the rows past T_b; whatever it made of them sits in
// alpha[t > T_b][b], which this kernel never addresses: alpha rows 0 .. T_b and emission rows 0 .. T_b - 1 only (the
// clamps of fetch() go DOWN to row 0).  What the pad rows hold never changes a bit of any output.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "kernels.h"

namespace gtnx {
namespace {

constexpr float NEG_INF = -__builtin_inff();

// wave-wide reductions by DPP (result in every lane), as in maxplus.hip
#define AD_DPP6(op)                                            \
  "s_nop 1\n\t" op " %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"  \
  op " %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"                \
  op " %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"                \
  op " %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"                \
  op " %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\ts_nop 1\n\t"             \
  op " %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\ts_nop 1"
__device__ __forceinline__ float wave_max63(float x) {
  asm volatile(AD_DPP6("v_max_f32_dpp") : "+v"(x));
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
}
__device__ __forceinline__ int wave_min63(int x) {
  asm volatile(AD_DPP6("v_min_i32_dpp") : "+v"(x));
  return __builtin_amdgcn_readlane(x, 63);
}

constexpr int AD_EMROW = 1024;  // emission rows up to this many labels are staged (else one load per step)

template <int RMAX>  // 64-lane slices of the staged rows: ceil(max(N, staged C) / 64), rounded up to 4 / 8 / 10 / 12 / 16
__global__ __launch_bounds__(64) void asg_decode_kernel(LazyGroup g, const int* __restrict__ frames, int* labels,
                                                       int64_t row_stride, float* scores, int* collapsed, int* lengths) {
  extern __shared__ float lds[];
  const int b = blockIdx.x, l = threadIdx.x;
  const int N = g.N, C = g.C, M = g.T;
  const bool stage_em = C <= AD_EMROW;
  float* rows = lds;                                   // [2][N] alpha[t-1] / alpha[t-2]
  float* erows = rows + 2 * N;                         // [2][C] (stage_em)
  int* ioff = reinterpret_cast<int*>(erows + (stage_em ? 2 * C : 0));  // [N + 1]
  int* nlab = ioff + N + 1;                            // [N]
  const int64_t plane = int64_t(g.nb) * N;
  int* lrow = labels + int64_t(b) * row_stride;
  int* crow = collapsed ? collapsed + int64_t(b) * row_stride : nullptr;
  int T = frames[b];
  T = T < 0 ? 0 : (T > M ? M : T);  // (the engine has refused such counts: nothing outside the planes is addressed)
  // ---- start of the trace: first maximal accept node of row T
  int node = -1;
  float top = NEG_INF;
  if (T >= 1) {
    const float* last = g.alpha + int64_t(T) * plane + int64_t(b) * N;
    float m = NEG_INF;
    int bk = INT_MAX;
    for (int k = l; k < g.g.n_accept; k += 64) {
      const float v = last[g.g.accept_list[k]];
      if (v > m) {
        m = v;
        bk = k;
      }
    }
    top = wave_max63(m);
    bk = wave_min63((m == top && top > NEG_INF) ? bk : INT_MAX);
    if (bk != INT_MAX) node = g.g.accept_list[bk];
  }
  auto no_path = [&]() {
    for (int i = l; i < M; i += 64) lrow[i] = -1;
    if (crow)
      for (int i = l; i < M; i += 64) crow[i] = -1;
    if (l == 0) {
      if (scores) scores[b] = NEG_INF;
      if (lengths) lengths[b] = 0;
    }
  };
  if (node < 0) {
    no_path();
    return;
  }
  // entries from T to the row's width (entry i always by lane i & 63, like the trace's own stores)
  for (int i = (T & ~63) + l; i < M; i += 64)
    if (i >= T) lrow[i] = -1;
  for (int n = l; n <= N; n += 64) ioff[n] = g.g.in_off[n];
  for (int n = l; n < N; n += 64) nlab[n] = g.nlab[n];
  const GTNX_G float* em = (const GTNX_G float*)g.em[b];
  const float* arow = g.alpha + int64_t(b) * N;
  constexpr int RB = 9;  // records per lane per batch: 576 cover the 513-arc in-rows of C4 in ONE trip to memory
  struct Rows {
    float a[RMAX], e[RMAX];
  };
  // (always valid addresses, no branches: a conditional request would turn the counted wait for the
  // records, which are requested BEFORE these rows and so return before them, into a wait for everything)
  auto fetch = [&](Rows& r, int t) {  // alpha[t] and the emission row of step t
#pragma unroll
    for (int i = 0; i < RMAX; ++i) {
      const int n = l + 64 * i;
      r.a[i] = arow[int64_t(t) * plane + (n < N ? n : N - 1)];
      r.e[i] = stage_em ? em[int64_t(t) * C + (n < C ? n : C - 1)] : 0.0f;
    }
  };
  auto park = [&](const Rows& r, int buf) {
#pragma unroll
    for (int i = 0; i < RMAX; ++i) {
      const int n = l + 64 * i;
      if (n < N) rows[buf * N + n] = r.a[i];
      if (stage_em && n < C) erows[buf * C + n] = r.e[i];
    }
  };
  // Rows are requested TWO steps before they are parked (a step's own chain is shorter than a trip to HBM),
  // into two register sets that alternate: step t requests the rows of step t - 3 and parks those of t - 2.
  Rows r0, r1;
  fetch(r0, T - 1);
  park(r0, (T - 1) & 1);
  fetch(r1, T >= 2 ? T - 2 : 0);
  __syncthreads();
  bool failed = false;
  int keep_lab = 0;
  auto step = [&](int t, Rows& rq, const Rows& rp) {  // rq: set to request into, rp: set to park
    const float* prev = rows + ((t - 1) & 1) * N;
    const int lab = nlab[node];  // every matched in-arc of `node` carries this label
    const float e = lab < 0 ? 0.0f : (stage_em ? erows[((t - 1) & 1) * C + lab] : em[int64_t(t - 1) * C + lab]);
    const int k0 = ioff[node], k1 = ioff[node + 1];
    float m = NEG_INF;
    int bsrc = INT_MAX;
    // the in-row, nine records per lane at a time, all requested before the first is looked at; the rows of
    // the step after next queue up behind the first batch
    for (int kb = k0; kb == k0 || kb < k1; kb += 64 * RB) {
      gtnx_i4 r[RB];
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        const int k = kb + l + 64 * i;
        r[i] = g.lrec_in[k < k1 ? k : (k1 > 0 ? k1 - 1 : 0)];
      }
      if (kb == k0) {
        __builtin_amdgcn_sched_barrier(0);
        fetch(rq, t >= 3 ? t - 3 : 0);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        const int k = kb + l + 64 * i;
        if (k < k1 && r[i].y >= 0) {
          const float x = prev[r[i].x] + __int_as_float(r[i].z) + e;
          // of equal maxima the one from the SMALLEST source node
          if (x > m || (x == m && r[i].x < bsrc)) {
            m = x;
            bsrc = r[i].x;
          }
        }
      }
    }
    const float mx = wave_max63(m);
    // the lane's own best is already its smallest source; across lanes the smallest source node holding the maximum
    const int src = wave_min63((m == mx && mx > NEG_INF) ? bsrc : INT_MAX);
    if (src == INT_MAX) {  // cannot happen below a finite best score
      failed = true;
      return;
    }
    // the step's label goes to the lane that owns frame t - 1 (a select: a lane-0 store here would put a branch
    // join between the requests above and the counted wait of park() below); every 64 steps the lanes write
    // their entries out together
    keep_lab = ((t - 1) & 63) == l ? lab : keep_lab;
    node = src;
    park(rp, t & 1);  // step t-2's rows -> the buffers step t's sat in ((t - 2) & 1 == t & 1)
    __syncthreads();
    if (((t - 1) & 63) == 0) {
      const int idx = (t - 1) + l;
      if (idx < T) lrow[idx] = keep_lab;
    }
  };
  for (int t = T; t >= 1 && !failed; t -= 2) {
    step(t, r0, r1);
    if (t >= 2 && !failed) step(t - 1, r1, r0);
  }
  if (failed) {
    no_path();
    return;
  }
  if (l == 0 && scores) scores[b] = top;
  if (!crow) return;
  // ---- collapsed sequence: entry i of the label row was stored by lane i & 63, which reads it back here
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
  if (l == 0 && lengths) lengths[b] = count;
}

}  // namespace

void launch_asg_decode(const LazyGroup& g, const int* d_frames, int* labels, int64_t row_stride, float* scores,
                       int* collapsed, int* lengths, hipStream_t st) {
  if (g.nb <= 0) return;
  const size_t lds = sizeof(float) * (size_t(4) * g.N + 1 + (g.C <= AD_EMROW ? size_t(2) * g.C : 0));
  const int slices = (std::max(g.N, g.C <= AD_EMROW ? g.C : 0) + 63) / 64;
#define AD_LAUNCH(R)                                                                                              \
  hipLaunchKernelGGL(asg_decode_kernel<R>, dim3(g.nb), dim3(64), lds, st, g, d_frames, labels, row_stride, scores, \
                     collapsed, lengths)
  if (slices <= 4) AD_LAUNCH(4);
  else if (slices <= 8) AD_LAUNCH(8);
  else if (slices <= 10) AD_LAUNCH(10);
  else if (slices <= 12) AD_LAUNCH(12);
  else AD_LAUNCH(16);
#undef AD_LAUNCH
}

}  // namespace gtnx
