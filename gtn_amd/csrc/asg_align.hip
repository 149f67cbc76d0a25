// asg_align.hip -- batched ASG forced alignment whose results stay on the device.
//
// What the reference does per utterance with viterbiPath (shortest.cpp:190-272) over compose(emissions,
// compose(forceAlign(labels), transitions)) (examples/asg.cpp:50-68) and a host loop over the path graph's arcs, as ONE
// launch for a whole batch.  The sibling of band_viterbi_align_kernel (align.hip) for the other criterion: per utterance
// one wave runs the tropical recursion over the U + 1 nodes of the force-alignment acceptor -- node n is "the first n
// labels are consumed", its two in-arcs are the self-loop (BandNode.aid[0]) and the step from node n - 1 (aid[1]), both
// matching label n - 1 and both weighted by the transitions (Batch::asg_force_align gathers them into `w`, arc-id
// order; the step into node 1 carries the start weight).  Same arithmetic as band_viterbi_wave_kernel and align.hip,
// alpha + (w + e) with exact maxima, so scores are bit-identical to those routes.
//   * two candidates per node: ONE back-pointer bit per (time, node), a word row of 64 lanes per 32 / NPL steps;
//   * exact ties: the step wins (k = c1 >= c0).  In the reference's queue node n - 1 leaves before node n in every
//     layer and only a strictly greater candidate replaces the first, so of equals the one from n - 1 stays -- no
//     ranks, no flag, no second launch.  One accept node (U): no accept tie;
//   * the chase holds the path's node of step t in lane t % 64; the frame's label is BandNode.lab of the node the step
//     ENTERS, its token that node - 1 -- never -1 inside a path: there are no blanks.  The <= 512 node labels are
//     staged in LDS where the emission ring was, and every 64 steps the wave stores 64 labels and 64 tokens;
//   * frames[b] <= T_full rows are aligned, entries from frames[b] on are written -1 by the same wave;
//   * an utterance without an accepting path (fewer frames than labels, or no labels and a frame): score -inf, every
//     entry -1.
// Algorithmic bytes per utterance: 4 T C (emissions, once) + T N / 4 (back-pointers out and in) + 8 T (the two rows).
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace gtnx {
namespace {

constexpr int VBLK = 2048;  // floats per staged block (C <= VBLK, C % 4 == 0, 16-byte aligned tensor)

__device__ __forceinline__ void settle(float& x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void settle(int& x) { asm volatile("" : "+v"(x)); }
// lane i <- lane i-1 (lane 0 takes `fill`)
__device__ __forceinline__ float wave_shr1(float x, float fill) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(x), 0x138, 0xf, 0xf, false));
}

template <int NPL>
__global__ __launch_bounds__(64) void asg_viterbi_align_kernel(const AsgAlignArgs* __restrict__ pairs) {
  const AsgAlignArgs P = pairs[blockIdx.x];
  const int T = P.T, TF = P.T_full, C = P.C, N = P.N;
  const int lane = threadIdx.x;
  constexpr int SPW = 32 / NPL;  // steps per back-pointer word
  constexpr int NLD = VBLK / 256;
  __shared__ __attribute__((aligned(16))) float ring[3 * VBLK];
  const float NINF = -__builtin_inff();
  const GTNX_G gtnx_i4* nodes = reinterpret_cast<const GTNX_G gtnx_i4*>(P.nodes);
  int loff[NPL];  // byte offset of the node's label inside an emission row
  float w0[NPL], w1[NPL], alpha[NPL];
#pragma unroll
  for (int j = 0; j < NPL; ++j) {
    const int m = lane * NPL + j;
    loff[j] = 0;
    w0[j] = w1[j] = NINF;  // (nodes past N, and node 0, keep -inf: every candidate of theirs is -inf)
    alpha[j] = NINF;
    if (m < N) {
      const gtnx_i4 q = nodes[m];
      loff[j] = 4 * (q.x >= 0 ? q.x : 0);
      if (q.y >= 0) w0[j] = P.w[q.y];
      if (q.z >= 0) w1[j] = P.w[q.z];
      if (P.nflags[m] & NF_START) alpha[j] = 0.0f;  // shortest.cpp:201-207 (paths begin at start nodes, time 0)
    }
  }
#pragma unroll
  for (int j = 0; j < NPL; ++j) {
    settle(w0[j]);
    settle(w1[j]);
    settle(loff[j]);
    settle(alpha[j]);
  }
  const int R = max(1, VBLK / C);  // rows per block
  const int NB = (T + R - 1) / R;
  const int64_t total = int64_t(T) * C;
  auto issue = [&](int b) {
    const int64_t f0 = int64_t(b) * R * C;
    float* dst = ring + (b % 3) * VBLK;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      int64_t f = f0 + i * 256 + lane * 4;
      f = f + 4 <= total ? f : total - 4;  // (past the end: the last 16 bytes again, never read from LDS)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(P.em + f),
                                       (__attribute__((address_space(3))) void*)(dst + i * 256), 16, 0, 0);
    }
  };
  GTNX_G unsigned* bp32 = P.bp;
  unsigned word = 0;
  if (NB > 0) issue(0);
  if (NB > 1) issue(1);
  for (int b = 0; b < NB; ++b) {
    // a block is eight vector-memory operations, always: everything older than the sixteen newest has landed
    if (b + 2 < NB) {
      issue(b + 2);
      asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    } else if (b + 1 < NB) {
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    const char* buf = reinterpret_cast<const char*>(ring + (b % 3) * VBLK);
    const int t0 = b * R, rows = min(R, T - t0);
    float e[NPL];
#pragma unroll
    for (int j = 0; j < NPL; ++j) e[j] = *reinterpret_cast<const float*>(buf + loff[j]);
    for (int i = 0; i < rows; ++i) {
      const int t = t0 + i;
      // the next row's emissions while this row is reduced (the last row of the block reads its own again)
      const char* nrow = buf + (i + 1 < rows ? i + 1 : i) * (C * 4);
      float en[NPL];
#pragma unroll
      for (int j = 0; j < NPL; ++j) en[j] = *reinterpret_cast<const float*>(nrow + loff[j]);
      const float s1 = wave_shr1(alpha[NPL - 1], NINF);
      float na[NPL];
      unsigned codes = 0;
#pragma unroll
      for (int j = 0; j < NPL; ++j) {
        const float p1 = j > 0 ? alpha[j > 0 ? j - 1 : 0] : s1;
        const float c0 = alpha[j] + (w0[j] + e[j]), c1 = p1 + (w1[j] + e[j]);
        // of two equal candidates the step: its source left the reference's queue first
        codes |= (c1 >= c0 ? 1u : 0u) << j;
        na[j] = fmaxf(c0, c1);
      }
      word |= codes << ((t % SPW) * NPL);
#pragma unroll
      for (int j = 0; j < NPL; ++j) {
        alpha[j] = na[j];
        e[j] = en[j];
      }
      if ((t % SPW) == SPW - 1 || t == T - 1) {
        bp32[int64_t(t / SPW) * 64 + lane] = word;
        word = 0;
      }
    }
  }
  // the accept node (NF_ACCEPT: node N - 1, the only one)
  float lv = NINF;
#pragma unroll
  for (int j = 0; j < NPL; ++j)
    if (lane * NPL + j == N - 1 && (P.nflags[N - 1] & NF_ACCEPT)) lv = alpha[j];
  const float fin = __shfl(lv, (N - 1) / NPL);
  const bool has = fin > NINF;  // (uniform)
  if (lane == 0 && P.score) P.score[0] = has ? fin : NINF;
  // entries the path does not cover: from T on, or every one when there is no path
  for (int t = (has ? T : 0) + lane; t < TF; t += 64) {
    P.labels[t] = -1;
    if (P.tokens) P.tokens[t] = -1;
  }
  if (!has || T == 0) return;
  // (the back-pointer words this wave stored are what it loads next: its own stores, waited for)
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  // the nodes' labels, where the emission ring was (every block has landed and been swept)
  int* llab = reinterpret_cast<int*>(ring);  // [64 NPL]
#pragma unroll
  for (int j = 0; j < NPL; ++j) llab[lane * NPL + j] = loff[j] >> 2;
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  // ---- chase the pointers: a scalar walk over the word rows, RB rows per batch, loaded by all lanes before the walk,
  // the next batch in flight meanwhile.  Lane t % 64 keeps the node step t enters; every 64 steps the wave stores the
  // labels and tokens of steps t .. t + 63
  unsigned node = unsigned(N - 1);
  const int NW = (T + SPW - 1) / SPW;
  constexpr int RB = NPL == 1 ? 8 : 16;  // word rows per batch (at most 256 steps unrolled)
  unsigned cur[RB], nxt[RB];
  const int nbatch = (NW + RB - 1) / RB;
  auto fetch = [&](unsigned (&dst)[RB], int q) {  // rows q RB .. q RB + RB - 1 (those past the end: the last row again)
#pragma unroll
    for (int r = 0; r < RB; ++r) dst[r] = bp32[int64_t(min(q * RB + r, NW - 1)) * 64 + lane];
  };
  fetch(cur, nbatch - 1);
  int pn = 0;
  for (int q = nbatch - 1; q >= 0; --q) {
    if (q > 0) fetch(nxt, q - 1);
#pragma unroll
    for (int r = RB - 1; r >= 0; --r) {
      const int wi = q * RB + r;
      if (wi < NW) {
#pragma unroll
        for (int u = SPW - 1; u >= 0; --u) {
          const int t = wi * SPW + u;
          if (t < T) {
            if (lane == (t & 63)) pn = int(node);
            const unsigned wv = unsigned(__builtin_amdgcn_readlane(int(cur[r]), int(node / NPL)));
            const unsigned k = (wv >> (u * NPL + (node % NPL))) & 1u;
            node -= min(k, node);
            if ((t & 63) == 0) {  // steps t .. t + 63, one per lane
              if (t + lane < T) {
                P.labels[t + lane] = llab[pn];
                if (P.tokens) P.tokens[t + lane] = pn - 1;
              }
            }
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < RB; ++r) cur[r] = nxt[r];
  }
}

}  // namespace

int asg_align_npl(int max_nodes) { return max_nodes <= 64 ? 1 : (max_nodes <= 128 ? 2 : (max_nodes <= 256 ? 4 : 8)); }
int asg_align_max_labels() { return VBLK; }
bool asg_align_ok(int max_nodes, int max_labels, int vec) {
  return vec && max_nodes <= 512 && max_labels <= VBLK && max_labels >= 4;
}
size_t asg_align_plane_bytes(int T, int npl) {
  const size_t spw = size_t(32 / npl);
  return ((size_t(T) + spw - 1) / spw * 256 + 256 + 255) / 256 * 256;
}
void launch_asg_align(const AsgAlignArgs* d_args, int n, int max_nodes, hipStream_t st) {
  if (n <= 0) return;
  switch (asg_align_npl(max_nodes)) {
    case 1: hipLaunchKernelGGL(asg_viterbi_align_kernel<1>, dim3(n), dim3(64), 0, st, d_args); break;
    case 2: hipLaunchKernelGGL(asg_viterbi_align_kernel<2>, dim3(n), dim3(64), 0, st, d_args); break;
    case 4: hipLaunchKernelGGL(asg_viterbi_align_kernel<4>, dim3(n), dim3(64), 0, st, d_args); break;
    default: hipLaunchKernelGGL(asg_viterbi_align_kernel<8>, dim3(n), dim3(64), 0, st, d_args); break;
  }
}

}  // namespace gtnx
