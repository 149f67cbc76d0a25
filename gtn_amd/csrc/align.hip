// align.hip -- batched CTC forced alignment whose results stay on the device.
//
// What the reference does per utterance with viterbiPath (shortest.cpp:190-272) over compose(ctcGraph(labels),
// linearGraph(T, C)) and a host loop over the path graph's arcs, as ONE launch for a whole batch: per utterance one
// wave runs the tropical recursion of band_viterbi_wave_kernel<NPL, RANKED = true> (band.hip) -- same arithmetic,
// alpha + (w + e) with exact maxima, so scores are bit-identical to that route -- and what leaves the kernel is the
// label and the token index of every frame, written from the pointer chase into the caller's rows:
//   * the chase holds the path's node of step t in lane t % 64; the frame's label is the label of the node the step
//     ENTERS (BandNode.lab), its token (node - 1) / 2 for an odd node and -1 for a blank one.  The <= 512 node labels
//     are staged in LDS once the emission ring is free (a lane already holds its nodes' labels as row offsets), so a
//     store of 64 frames gathers from LDS, and there is no third phase: no path nodes, arcs or weights in HBM;
//   * frames[b] <= T_full rows are aligned, entries from frames[b] on are written -1 by the same wave;
//   * exact ties are always decided in the launch, by the closed-form queue ranks of ops_band.cpp (tie_ranks) computed
//     here from the utterance's records and p, the number of leading strict ascents of its label sequence; the
//     accept list's order is the creation order, i.e. the smaller node;
//   * an utterance without an accepting path: score -inf, every entry -1.
// Algorithmic bytes per utterance: 4 T C (emissions, once) + T N / 2 (back-pointers out and in) + 8 T (the two rows).
// The sweep is kept here and not shared with band.hip through an include: that kernel also carries the unranked tie
// codes, the micro-benchmark switches and the third phase, and its instantiations must keep compiling to what they
// were.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace gtnx {
namespace {

constexpr int VBLK = 2048;  // floats per staged block (C <= VBLK, C % 4 == 0, 16-byte aligned tensor)

// (band.hip: a use in front of the main loop, so that the wait for a prologue load is not placed inside it)
__device__ __forceinline__ void settle(float& x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void settle(int& x) { asm volatile("" : "+v"(x)); }
// lane i <- lane i-1 (lane 0 takes `fill`)
__device__ __forceinline__ float wave_shr1(float x, float fill) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(x), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_max(float x) {  // uniform result
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o));
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}

// position of node m in the reference's queue, every layer (ops_band.cpp tie_ranks, the closed form): with U labels,
// N = 2U + 1 nodes and p leading strict ascents
//   0 | (2i, 2i-1) for i = 1..p | N-1 | for i = U-1 down to p+1: (2i, 2i+1) if label i differs from label i-1 (a skip
//   arc enters 2i+1, BandNode.aid[2]) else (2i+1, 2i) | 2p+1
__device__ __forceinline__ int queue_rank(int m, int N, int p, const GTNX_G gtnx_i4* nodes) {
  if (m < 0 || m >= N) return 0x7ffffffe;
  const int U = (N - 1) >> 1;
  if (m == 0) return 0;
  if (m == 2 * U) return 2 * p + 1;
  if (m == 2 * p + 1) return 2 * U;
  if (m <= 2 * p) return (m & 1) ? m + 1 : m - 1;
  const int i = m >> 1;  // nodes 2i and 2i+1, p < i < U
  const bool skip = nodes[2 * i + 1].w >= 0;
  const bool even = (m & 1) == 0;
  return 2 * p + 2 + 2 * (U - 1 - i) + (even == skip ? 0 : 1);
}

template <int NPL>
__global__ __launch_bounds__(64) void band_viterbi_align_kernel(const AlignArgs* __restrict__ pairs) {
  const AlignArgs P = pairs[blockIdx.x];
  const int T = P.T, TF = P.T_full, C = P.C, N = P.N;
  const int lane = threadIdx.x;
  constexpr int SPW = 16 / NPL;  // steps per back-pointer word
  constexpr int NLD = VBLK / 256;
  __shared__ __attribute__((aligned(16))) float ring[3 * VBLK];
  const float NINF = -__builtin_inff();
  const GTNX_G gtnx_i4* nodes = reinterpret_cast<const GTNX_G gtnx_i4*>(P.nodes);
  int loff[NPL];  // byte offset of the node's label inside an emission row
  float w0[NPL], w1[NPL], w2[NPL], alpha[NPL];
  bool acc[NPL];
#pragma unroll
  for (int j = 0; j < NPL; ++j) {
    const int m = lane * NPL + j;
    loff[j] = 0;
    w0[j] = w1[j] = w2[j] = NINF;  // (nodes past N keep -inf: every candidate of theirs is -inf)
    alpha[j] = NINF;
    acc[j] = false;
    if (m < N) {
      const gtnx_i4 q = nodes[m];
      loff[j] = 4 * (q.x >= 0 ? q.x : 0);
      if (q.y >= 0) w0[j] = 0.0f;  // (a CTC target's arcs weigh nothing)
      if (q.z >= 0) w1[j] = 0.0f;
      if (q.w >= 0) w2[j] = 0.0f;
      const uint8_t f = P.nflags[m];
      if (f & NF_START) alpha[j] = 0.0f;  // shortest.cpp:201-207 (paths begin at start nodes, time 0)
      acc[j] = (f & NF_ACCEPT) != 0;
    }
  }
  int r0[NPL], r1[NPL], r2[NPL];  // ranks of the three source nodes of every node of this lane
#pragma unroll
  for (int j = 0; j < NPL; ++j) {
    const int m = lane * NPL + j;
    r0[j] = m < N ? queue_rank(m, N, P.p, nodes) : 0x7ffffffe;
    r1[j] = m - 1 < N ? queue_rank(m - 1, N, P.p, nodes) : 0x7ffffffe;
    r2[j] = m - 2 < N ? queue_rank(m - 2, N, P.p, nodes) : 0x7ffffffe;
  }
#pragma unroll
  for (int j = 0; j < NPL; ++j) {
    settle(w0[j]);
    settle(w1[j]);
    settle(w2[j]);
    settle(loff[j]);
    settle(r0[j]);
    settle(r1[j]);
    settle(r2[j]);
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
      float s1, s2;
      if (NPL >= 2) {
        s1 = wave_shr1(alpha[NPL - 1], NINF);
        s2 = wave_shr1(alpha[NPL >= 2 ? NPL - 2 : 0], NINF);
      } else {
        s1 = wave_shr1(alpha[0], NINF);
        s2 = wave_shr1(s1, NINF);
      }
      float na[NPL];
      const int sh = (t % SPW) * 2 * NPL;
      unsigned codes = 0;
#pragma unroll
      for (int j = 0; j < NPL; ++j) {
        const float p1 = j > 0 ? alpha[j > 0 ? j - 1 : 0] : s1;
        const float p2 = j > 1 ? alpha[j > 1 ? j - 2 : 0] : (j == 1 ? s1 : s2);
        const float c0 = alpha[j] + (w0[j] + e[j]), c1 = p1 + (w1[j] + e[j]), c2 = p2 + (w2[j] + e[j]);
        const float best = fmaxf(fmaxf(c0, c1), c2);
        // of the candidates that reach the maximum, the one from the source with the smallest rank
        const int q0 = c0 == best ? r0[j] : 0x7fffffff, q1 = c1 == best ? r1[j] : 0x7fffffff,
                  q2 = c2 == best ? r2[j] : 0x7fffffff;
        unsigned k = (q0 <= q1 && q0 <= q2) ? 0u : (q1 <= q2 ? 1u : 2u);
        k = best == NINF ? 3u : k;
        codes |= k << (2 * j);
        na[j] = best;
      }
      word |= codes << sh;
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
  // the best accept node (shortest.cpp:233-244): maximum, first in the accept list among equals -- the smaller node
  float lv = NINF;
#pragma unroll
  for (int j = 0; j < NPL; ++j) lv = fmaxf(lv, acc[j] ? alpha[j] : NINF);
  const float wmx = wave_max(lv);
  int bm = 1 << 30;
#pragma unroll
  for (int j = NPL - 1; j >= 0; --j)
    if (acc[j] && alpha[j] == wmx && wmx > NINF) bm = lane * NPL + j;
  for (int o = 32; o > 0; o >>= 1) bm = min(bm, __shfl_xor(bm, o));
  const int best = bm == (1 << 30) ? -1 : bm;  // (uniform)
  if (lane == 0 && P.score) P.score[0] = best >= 0 ? wmx : NINF;
  // entries the path does not cover: from T on, or every one when there is no path
  for (int t = (best >= 0 ? T : 0) + lane; t < TF; t += 64) {
    P.labels[t] = -1;
    if (P.tokens) P.tokens[t] = -1;
  }
  if (best < 0 || T == 0) return;
  // (the back-pointer words this wave stored are what it loads next: its own stores, waited for)
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  // the nodes' labels, where the emission ring was (every block has landed and been swept)
  int* llab = reinterpret_cast<int*>(ring);  // [64 NPL]
#pragma unroll
  for (int j = 0; j < NPL; ++j) llab[lane * NPL + j] = loff[j] >> 2;
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  // ---- chase the pointers: a scalar walk over the word rows -- sixteen rows (16 SPW steps) per batch, loaded by
  // all lanes before the walk, the next batch in flight meanwhile.  Lane t % 64 keeps the node step t enters; every
  // 64 steps the wave stores the labels and tokens of steps t .. t + 63
  unsigned node = unsigned(__builtin_amdgcn_readfirstlane(best));
  const int NW = (T + SPW - 1) / SPW;
  constexpr int RB = 16;  // word rows per batch
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
            unsigned k = (wv >> (u * 2 * NPL + 2 * (node % NPL))) & 3u;
            k = k == 3u ? 0u : k;  // (a dead node: the best path never runs through one)
            node -= min(k, node);
            if ((t & 63) == 0) {  // steps t .. t + 63, one per lane
              if (t + lane < T) {
                P.labels[t + lane] = llab[pn];
                if (P.tokens) P.tokens[t + lane] = (pn & 1) ? (pn - 1) >> 1 : -1;
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

int align_npl(int max_nodes) { return max_nodes <= 64 ? 1 : (max_nodes <= 128 ? 2 : (max_nodes <= 256 ? 4 : 8)); }
bool band_align_ok(int max_nodes, int max_labels, int vec) {
  return vec && max_nodes <= 512 && max_labels <= VBLK && max_labels >= 4;
}
void launch_band_align(const AlignArgs* d_args, int n, int max_nodes, hipStream_t st) {
  if (n <= 0) return;
  switch (align_npl(max_nodes)) {
    case 1: hipLaunchKernelGGL(band_viterbi_align_kernel<1>, dim3(n), dim3(64), 0, st, d_args); break;
    case 2: hipLaunchKernelGGL(band_viterbi_align_kernel<2>, dim3(n), dim3(64), 0, st, d_args); break;
    case 4: hipLaunchKernelGGL(band_viterbi_align_kernel<4>, dim3(n), dim3(64), 0, st, d_args); break;
    default: hipLaunchKernelGGL(band_viterbi_align_kernel<8>, dim3(n), dim3(64), 0, st, d_args); break;
  }
}

}  // namespace gtnx
