// lm_walk.h -- the device walk of a compiled LM graph (lm_graph.h has the words; DESIGN section 30 the contract),
// shared by the search kernels of the two prefix beam searches (ctc_beam.hip, asg_beam.hip): what ranks beside the
// acoustic score, the term of an extension, and the walks of one thread.  In both kernels wave v serves the prefixes
// v, v + 4, ... and its lane k member k of the token set, so a thread holds at most kWalkTrips walks, one per prefix
// of its wave.  For .hip files only; everything here is inlined, so a file's code object holds nothing it does not
// call.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "beam_common.h"
#include "kernels.h"
#include "pair_kernels.h"

namespace gtnx {

constexpr int kLmNone = 0, kLmTable = 1, kLmGraph = 2;  // what ranks beside the acoustic score

constexpr int kWalkTrips = 16;  // walks a thread holds at most: one per prefix of its wave (64 prefixes, 4 waves)

// lm_weight * w + lm_bonus: a product rounded, then a sum rounded -- never fused, the order of the host forms
__device__ __forceinline__ float lm_term(float weight, float w, float bonus) {
#pragma clang fp contract(off)
  const float scaled = weight * w;
  return scaled + bonus;
}

// The walks of one thread: label c from the states st[q] of the trips q < ntrip, trip q being live when act[q].  A walk
// is a chain of dependent loads (the state's two words, then one arc word per probe of the bisection, then the next
// state of the back-off chain), so they advance together: a round loads the next word of every walk, then every walk
// takes its step.  A walk that is over, or a trip without one, loads word 0.  at[q] is the word a walk reads next
// (below 2 * states: a state; above: an arc; -1: over), [lo, hi) the arcs that may still hold the label.
// kWalkChunk trips go together (the trips Q0 .. Q0 + kWalkChunk - 1 of one call): with all 16 in flight the kernel
// needs 346 registers, only one workgroup fits a compute unit where two of the table's do, and the batch takes twice
// as long -- measured, DESIGN section 30.  Eight cover a beam of 32 in one pass; a larger beam walks twice.
// Bounds, all compile-time: a walk visits at most kWalkStates states and probes a state's arcs at most kWalkBisect
// times, and the rounds stop at their product whatever the words hold.  A walk that runs out of either is forbidden.
constexpr int kWalkStates = 9, kWalkBisect = 32;
constexpr int kWalkRounds = kWalkStates * (1 + kWalkBisect);
constexpr int kWalkChunk = 8;
template <int Q0>
__device__ __forceinline__ void lm_walks(const GTNX_G gtnx_i4* g, int states2, int c, int ntrip,
                                         const int (&st)[kWalkTrips], const bool (&act)[kWalkTrips],
                                         float (&wsum)[kWalkTrips], int (&next)[kWalkTrips]) {
  const GTNX_G gtnx_i2* g2 = reinterpret_cast<const GTNX_G gtnx_i2*>(g);
  int at[kWalkChunk], lo[kWalkChunk], hi[kWalkChunk], epsd[kWalkChunk], epsw[kWalkChunk], seen[kWalkChunk];
#pragma unroll
  for (int q = 0; q < kWalkChunk; ++q) {
    at[q] = act[Q0 + q] ? 2 * st[Q0 + q] : -1;
    lo[q] = hi[q] = 0;
    epsd[q] = -1;
    epsw[q] = 0;
    seen[q] = 0;  // states visited so far, and from bit 8 the probes of this state's arcs
  }
  for (int round = 0; round < kWalkRounds; ++round) {
    gtnx_i4 w0[kWalkChunk];
    gtnx_i2 w1[kWalkChunk];
#pragma unroll
    for (int q = 0; q < kWalkChunk; ++q) {
      if (Q0 + q >= ntrip) continue;  // (the same in every thread)
      const int p = at[q] < 0 ? 0 : at[q];
      w0[q] = g[p];
      w1[q] = g2[2 * (p + 1)];  // (a state's second word: first label, dense; the form ends with a spare word)
    }
    bool more = false;
#pragma unroll
    for (int q = 0; q < kWalkChunk; ++q) {
      if (Q0 + q >= ntrip) continue;
      if (at[q] < 0) continue;
      const bool first = (seen[q] & 255) <= 1;  // no back-off weight yet: the sum starts from the first weight
      if (at[q] < states2) {
        seen[q] = (seen[q] & 255) + 1;
        epsd[q] = w0[q].z;
        epsw[q] = w0[q].w;
        lo[q] = w0[q].x;
        hi[q] = w0[q].x + w0[q].y;
        if (w1[q].y) {  // labels first .. first + count - 1: the one arc it can be
          const unsigned j = unsigned(c) - unsigned(w1[q].x);
          if (j < unsigned(w0[q].y)) {
            lo[q] += int(j);
            hi[q] = lo[q] + 1;
          } else {
            hi[q] = lo[q];
          }
        }
      } else {
        seen[q] += 256;
        if (w0[q].x == c) {
          const float w = __int_as_float(w0[q].z);
          wsum[Q0 + q] = first ? w : wsum[Q0 + q] + w;
          next[Q0 + q] = w0[q].y;
          at[q] = -1;
          continue;
        }
        if (w0[q].x < c) lo[q] = at[q] + 1;
        else hi[q] = at[q];
      }
      if (lo[q] < hi[q] && (seen[q] >> 8) < kWalkBisect) {
        at[q] = lo[q] + ((hi[q] - lo[q]) >> 1);
        more = true;
      } else if (epsd[q] >= 0 && (seen[q] & 255) < kWalkStates) {
        const float w = __int_as_float(epsw[q]);
        wsum[Q0 + q] = (seen[q] & 255) <= 1 ? w : wsum[Q0 + q] + w;
        at[q] = 2 * epsd[q];
        more = true;
      } else {
        wsum[Q0 + q] = NEG_INF;  // forbidden: the term is not finite, whatever the weight
        next[Q0 + q] = 0;
        at[q] = -1;
      }
    }
    if (!more) break;
  }
#pragma unroll
  for (int q = 0; q < kWalkChunk; ++q)
    if (at[q] >= 0) wsum[Q0 + q] = NEG_INF;  // (the rounds ran out)
}

}  // namespace gtnx
