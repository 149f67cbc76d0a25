// gtn/batch.h -- extension: B graphs held as one record (gtnx_batch_* in gtn_amd.h).
//
// What the reference writes as parallelMap over per-utterance graphs
// (benchmarks/ctc.cpp:150-165) reads the same here with one Batch per call:
//   using namespace gtn::batched;
//   auto loss = subtract(forwardScore(ems), forwardScore(intersect(targets, ems)));
//   backward(loss);
// Elements are ordinary graphs whenever somebody asks for one (operator[]).
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

#include "gtn/functions.h"

namespace gtn {

class Batch {
 public:
  Batch() = default;
  /** the graphs of a vector as one record (they stay what they are) */
  explicit Batch(const std::vector<Graph>& graphs) {
    auto h = detail::handles(graphs);
    detail::check(gtnx_batch_from_graphs(h.data(), static_cast<int>(h.size()), &h_));
  }
  Batch(const Batch&) = delete;
  Batch& operator=(const Batch&) = delete;
  Batch(Batch&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  Batch& operator=(Batch&& o) noexcept {
    if (this != &o) {
      reset();
      h_ = o.h_;
      o.h_ = nullptr;
    }
    return *this;
  }
  ~Batch() { reset(); }

  /** CTC target acceptors (benchmarks/ctc.cpp:40-58) of label sequences, built on the device */
  static Batch ctcTargets(const std::vector<std::vector<int>>& targets, int blank = 0, bool calcGrad = true) {
    std::vector<int> flat, len;
    len.reserve(targets.size());
    size_t total = 0;
    for (auto& t : targets) total += t.size();
    flat.reserve(total);
    for (auto& t : targets) {
      flat.insert(flat.end(), t.begin(), t.end());
      len.push_back(static_cast<int>(t.size()));
    }
    return ctcTargets(flat.data(), len.data(), static_cast<int>(targets.size()), blank, calcGrad);
  }
  static Batch ctcTargets(const int* labels, const int* lengths, int n, int blank = 0, bool calcGrad = true) {
    Batch b;
    detail::check(gtnx_batch_ctc_targets(labels, lengths, n, blank, calcGrad, &b.h_));
    return b;
  }
  /** compose(forceAlign(target), transitions) of examples/asg.cpp:50-68 for every label sequence, built on the
   *  device; `transitions` in the arc layout of examples/asg.cpp:36-47 over `numLabels` labels */
  static Batch asgForceAlign(const int* labels, const int* lengths, int n, const Graph& transitions, int numLabels) {
    Batch b;
    detail::check(gtnx_batch_asg_force_align(labels, lengths, n, transitions.handle(), numLabels, &b.h_));
    return b;
  }
  /** n linear graphs over one device tensor [n][M][N] (see linearGraphs); rows (host, [n]): a padded tensor --
   *  element b is linearGraph(rows[b], N) over the first rows[b] rows of its slab, its gradient keeps the [M][N]
   *  layout with zeros in the pad rows (gtnx_batch_linear_rows) */
  static Batch linear(int n, int M, int N, const void* deviceWeights, bool calcGrad = true, bool borrow = false,
                      const int* rows = nullptr) {
    Batch b;
    if (rows)
      detail::check(gtnx_batch_linear_rows(n, M, N, rows, calcGrad, deviceWeights, borrow, &b.h_));
    else
      detail::check(gtnx_batch_linear(n, M, N, calcGrad, deviceWeights, borrow, &b.h_));
    return b;
  }

  int size() const {
    int n = 0;
    if (h_) detail::check(gtnx_batch_size(h_, &n));
    return n;
  }
  /** element i as an ordinary graph */
  Graph operator[](int i) const {
    gtnx_graph_t g;
    detail::check(gtnx_batch_get(h_, i, &g));
    return Graph::fromHandle(g);
  }
  /** item() of every element */
  std::vector<float> items() const {
    std::vector<float> v(static_cast<size_t>(size()));
    if (!v.empty()) detail::check(gtnx_batch_items(h_, v.data()));
    return v;
  }
  void itemsToDevice(void* deviceOut) const { detail::check(gtnx_batch_items_device(h_, deviceOut)); }
  /** where the elements' gradients should end up (element i at deviceOut + offsets[i] floats): before backward a
   *  hint that lets kernels store there directly, afterwards the gather */
  void bindGrads(void* deviceOut, const int64_t* offsets) { detail::check(gtnx_batch_grads_bind_device(h_, deviceOut, offsets)); }
  void gradsToDevice(void* deviceOut, const int64_t* offsets) const {
    detail::check(gtnx_batch_grads_device(h_, deviceOut, offsets));
  }
  gtnx_batch_t handle() const { return h_; }
  static Batch fromHandle(gtnx_batch_t h) {
    Batch b;
    b.h_ = h;
    return b;
  }

 private:
  void reset() {
    if (h_) gtnx_batch_destroy(h_);
    h_ = nullptr;
  }
  gtnx_batch_t h_ = nullptr;
};

namespace detail {
template <class F>
Batch batchUnary(F f, const Batch& a) {
  gtnx_batch_t out;
  check(f(a.handle(), &out));
  return Batch::fromHandle(out);
}
template <class F>
Batch batchBinary(F f, const Batch& a, const Batch& b) {
  gtnx_batch_t out;
  check(f(a.handle(), b.handle(), &out));
  return Batch::fromHandle(out);
}
} // namespace detail

// (in gtn::batched like the vector forms: the plain names stay un-overloaded, reference callers
//  pass them as function pointers -- parallelMap(compose, a, b))
namespace batched {
inline Batch negate(const Batch& a) { return detail::batchUnary(&gtnx_batch_negate, a); }
inline Batch add(const Batch& a, const Batch& b) { return detail::batchBinary(&gtnx_batch_add, a, b); }
inline Batch subtract(const Batch& a, const Batch& b) { return detail::batchBinary(&gtnx_batch_subtract, a, b); }
// ... with the values written straight into device memory of the caller's (which must outlive the result)
inline Batch subtract(const Batch& a, const Batch& b, void* itemsDevice) {
  gtnx_batch_t out;
  detail::check(gtnx_batch_subtract_into(a.handle(), b.handle(), itemsDevice, &out));
  return Batch::fromHandle(out);
}
inline Batch compose(const Batch& a, const Batch& b) { return detail::batchBinary(&gtnx_batch_compose, a, b); }
inline Batch intersect(const Batch& a, const Batch& b) { return detail::batchBinary(&gtnx_batch_intersect, a, b); }
inline Batch forwardScore(const Batch& a) { return detail::batchUnary(&gtnx_batch_forward_score, a); }
inline Batch viterbiScore(const Batch& a) { return detail::batchUnary(&gtnx_batch_viterbi_score, a); }
inline Batch viterbiPath(const Batch& a) { return detail::batchUnary(&gtnx_batch_viterbi_path, a); }
/** Forced alignment with the results left on the device: row b of labelsDevice (int32, rowStride entries apart) gets
 *  the label of every frame of utterance b's best path, -1 past the path; tokensDevice the index into the label
 *  sequence (-1 on blank frames), scoresDevice the path scores; frames (host, [n]): emission rows to align per
 *  utterance.  One launch, no copy back and no wait for a product of Batch::ctcTargets with Batch::linear, and for a
 *  product of Batch::asgForceAlign with Batch::linear over the same alphabet (either argument order; tokens = index
 *  into the label sequence, never -1 inside an ASG path); other batches go through viterbiPath (tokensDevice and
 *  frames must be null there) -- gtnx_batch_viterbi_align */
inline void viterbiAlign(const Batch& product, int* labelsDevice, int64_t rowStride, int* tokensDevice = nullptr,
                         float* scoresDevice = nullptr, const int* frames = nullptr) {
  detail::check(gtnx_batch_viterbi_align(product.handle(), frames, labelsDevice, rowStride, tokensDevice, scoresDevice));
}
/** viterbiPath(compose(ems[b], transitions)) of the whole batch against ONE shared graph, results left on the device:
 *  row b of labelsDevice (int32, rowStride >= M entries apart) gets the label of every frame t < T_b and -1 from T_b
 *  to the row's width M; scoresDevice the path scores; collapsedDevice (rows like labelsDevice) the labels with runs of
 *  equal consecutive frames merged, then -1; lengthsDevice (needs collapsedDevice) how many; frames (host, [n]): T_b,
 *  null = the rows the batch carries.  No accepting path (T_b = 0 included): entries -1, score -inf, length 0.  A
 *  Batch::linear against an asgTransitions-shaped graph of 8 .. 1024 nodes: ONE sweep of the padded batch and one
 *  launch, no copy back, no wait; the pad rows never change a bit of any output; exact ties: first accept node, then
 *  the smallest source node.  Other graphs / batches go through viterbiPath and one upload (frames must be null
 *  there) -- gtnx_batch_viterbi_decode */
inline void viterbiDecode(const Batch& ems, const Graph& transitions, int* labelsDevice, int64_t rowStride,
                          float* scoresDevice = nullptr, const int* frames = nullptr, int* collapsedDevice = nullptr,
                          int* lengthsDevice = nullptr) {
  detail::check(gtnx_batch_viterbi_decode(ems.handle(), transitions.handle(), frames, labelsDevice, rowStride,
                                          scoresDevice, collapsedDevice, lengthsDevice));
}
/** viterbiPath(ems[b]) of a whole batch of chains plus the CTC collapse, results left on the device: row b of
 *  labelsDevice (int32, rowStride >= M entries apart) gets the first label holding the maximum of every frame t < T_b
 *  and -1 from T_b to the row's width M; scoresDevice the path scores (float32 sum in frame order); collapsedDevice
 *  (rows like labelsDevice) the labels with repeats merged and `blank` dropped (blank < 0: nothing dropped), then -1;
 *  startsDevice (rows alike; needs collapsedDevice) the first frame of each; lengthsDevice (needs collapsedDevice) how
 *  many; frames (host, [n]): T_b, null = the rows the batch carries.  A frame with nothing above -inf: no path --
 *  entries -1, score -inf, length 0; T_b = 0 likewise.  A Batch::linear: two launches, no copy
 *  back, no wait, rows from T_b on are never read.  Other batches go through viterbiPath and one upload (frames must
 *  be null there) -- gtnx_batch_linear_decode */
inline void linearDecode(const Batch& ems, int* labelsDevice, int64_t rowStride, float* scoresDevice = nullptr,
                         const int* frames = nullptr, int blank = -1, int* collapsedDevice = nullptr,
                         int* startsDevice = nullptr, int* lengthsDevice = nullptr) {
  detail::check(gtnx_batch_linear_decode(ems.handle(), frames, blank, labelsDevice, rowStride, scoresDevice,
                                         collapsedDevice, startsDevice, lengthsDevice));
}
/** numSamples alignments of every chain of a Batch::linear drawn from its frame posteriors (label c of frame t with
 *  probability exp(x / temperature) / Z over the finite entries, inverse CDF in label order, Philox4x32-10 keyed by
 *  `seed`), plus the CTC collapse, results left on the device: tokensDevice int32 [n][numSamples][rowStride] (the
 *  alignment with repeats merged and `blank` dropped, then -1 up to the row's width M), lengthsDevice int32
 *  [n][numSamples], logqDevice (may be null) float32 [n][numSamples] the log-probability of the drawn alignment,
 *  labelsDevice (may be null) int32 [n][numSamples][rowStride] the frame labels.  A frame without a finite entry or
 *  T_b = 0: -1, 0, -inf.  numSamples 1 .. 1024; frames (host, [n]): T_b, null = the rows the batch carries.  Two
 *  launches, no copy back, no wait, rows from T_b on are never read -- gtnx_batch_ctc_sample */
inline void ctcSample(const Batch& ems, int* tokensDevice, int64_t rowStride, int* lengthsDevice,
                      float* logqDevice = nullptr, int* labelsDevice = nullptr, int blank = 0, int numSamples = 4,
                      uint64_t seed = 0, float temperature = 1.0f, const int* frames = nullptr) {
  detail::check(gtnx_batch_ctc_sample(ems.handle(), frames, blank, numSamples, seed, temperature, tokensDevice,
                                      rowStride, lengthsDevice, logqDevice, labelsDevice));
}
/** CTC prefix beam search with N-best output over a Batch::linear, results left on the device: tokensDevice int32
 *  [n][nbest][rowStride] (the labels of hypothesis r, then -1 up to the row's width M), lengthsDevice int32 [n][nbest],
 *  scoresDevice float32 [n][nbest] (the log score summed over the alignments the beam kept); slots without a hypothesis:
 *  -1, 0, -inf.  beamSize 1 .. 64 prefixes, the cutoffTopN (1 .. 32) best labels of a frame plus blank, nbest <=
 *  beamSize; frames (host, [n]): T_b, null = the rows the batch carries.  Two launches, no copy back, no wait, rows from
 *  T_b on are never read -- gtnx_batch_ctc_beam_decode */
inline void ctcBeamDecode(const Batch& ems, int* tokensDevice, int64_t rowStride, int* lengthsDevice, float* scoresDevice,
                          int blank = 0, int beamSize = 16, int cutoffTopN = 16, int nbest = 1,
                          const int* frames = nullptr) {
  detail::check(gtnx_batch_ctc_beam_decode(ems.handle(), frames, blank, beamSize, cutoffTopN, nbest, tokensDevice,
                                           rowStride, lengthsDevice, scoresDevice));
}
/** The same search with a bigram over the labels fused into the ranking: lmDevice float32 [C + C * C] in the arc order
 *  of criteria::asgTransitions (lm[c]: c as first label; lm[C + i * C + j]: j followed by i); a prefix carries L = the
 *  sum over its labels of lmWeight * lm(...) + insertionBonus, candidates rank by acoustic total + L, -inf in the table
 *  forbids.  scoresDevice: acoustic + L; amScoresDevice (may be null): the acoustic total alone --
 *  gtnx_batch_ctc_beam_decode_lm */
inline void ctcBeamDecode(const Batch& ems, const float* lmDevice, float lmWeight, float insertionBonus,
                          int* tokensDevice, int64_t rowStride, int* lengthsDevice, float* scoresDevice,
                          float* amScoresDevice = nullptr, int blank = 0, int beamSize = 16, int cutoffTopN = 16,
                          int nbest = 1, const int* frames = nullptr) {
  detail::check(gtnx_batch_ctc_beam_decode_lm(ems.handle(), frames, blank, beamSize, cutoffTopN, nbest, lmDevice,
                                              lmWeight, insertionBonus, tokensDevice, rowStride, lengthsDevice,
                                              scoresDevice, amScoresDevice));
}
/** A language model held as a graph, compiled for ctcBeamDecode (gtnx_lm_graph_create has the contract): a
 *  deterministic acceptor with back-off (failure) arcs.  A snapshot of the graph's input labels and weights at
 *  construction; no autograd; accept flags and output labels are ignored.  Host work: needs no device until a decode
 *  uses it. */
class LmGraph {
 public:
  struct Info {
    int64_t numStates, numArcs;
    int startState, longestEpsilonChain;
  };
  explicit LmGraph(const Graph& g) { detail::check(gtnx_lm_graph_create(g.handle(), &h_)); }
  LmGraph(const LmGraph&) = delete;
  LmGraph& operator=(const LmGraph&) = delete;
  LmGraph(LmGraph&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  LmGraph& operator=(LmGraph&& o) noexcept {
    if (this != &o) {
      if (h_) gtnx_lm_graph_destroy(h_);
      h_ = o.h_;
      o.h_ = nullptr;
    }
    return *this;
  }
  ~LmGraph() {
    if (h_) gtnx_lm_graph_destroy(h_);
  }
  /** the walk of `label` from `state` (failure-arc semantics): false when the label is forbidden there */
  bool walk(int state, int label, float* weight, int* nextState) const {
    float w;
    int nx;
    detail::check(gtnx_lm_graph_walk(h_, state, label, &w, &nx));
    if (weight) *weight = w;
    if (nextState) *nextState = nx;
    return nx >= 0;
  }
  Info info() const {
    gtnx_lm_graph_info_t i;
    detail::check(gtnx_lm_graph_info(h_, &i));
    return Info{i.num_states, i.num_arcs, i.start_state, i.longest_epsilon_chain};
  }
  gtnx_lm_graph_t handle() const { return h_; }

 private:
  gtnx_lm_graph_t h_ = nullptr;
};
/** The same search with a compiled LM graph in the table's place: every prefix also carries its LM state, an extension
 *  adds lmWeight * (weight of the walk of (state, label)) + insertionBonus, a label the walk forbids is dropped --
 *  gtnx_batch_ctc_beam_decode_graph */
inline void ctcBeamDecode(const Batch& ems, const LmGraph& lm, float lmWeight, float insertionBonus, int* tokensDevice,
                          int64_t rowStride, int* lengthsDevice, float* scoresDevice, float* amScoresDevice = nullptr,
                          int blank = 0, int beamSize = 16, int cutoffTopN = 16, int nbest = 1,
                          const int* frames = nullptr) {
  detail::check(gtnx_batch_ctc_beam_decode_graph(ems.handle(), frames, blank, beamSize, cutoffTopN, nbest, lm.handle(),
                                                 lmWeight, insertionBonus, tokensDevice, rowStride, lengthsDevice,
                                                 scoresDevice, amScoresDevice));
}
/** Levenshtein distance (unit costs) of all B * N pairs (hyp[b, k], ref[b]) of device-resident token rows, results left
 *  on the device: hypDevice int32 B * N rows of width L, hypStride (>= L) apart, hypLengthsDevice int32 [B][N];
 *  refDevice int32 B rows of width U, refStride (>= U) apart, refLengthsDevice int32 [B] -- the lengths are device
 *  memory, clamped to the widths by the kernel, and nothing at or past a length is read; distDevice int32 [B][N];
 *  opsDevice int32 [B][N][3] = (substitutions, deletions, insertions) of the walk back that prefers diagonal, then up,
 *  then left, or null to skip it.  L <= 65536, U <= 4096.  One launch without ops; no copy back, no wait --
 *  gtnx_batch_edit_distance */
inline void editDistance(const int* hypDevice, int64_t hypStride, const int* hypLengthsDevice, const int* refDevice,
                         int64_t refStride, const int* refLengthsDevice, int B, int N, int L, int U, int* distDevice,
                         int* opsDevice = nullptr) {
  detail::check(gtnx_batch_edit_distance(hypDevice, hypStride, hypLengthsDevice, refDevice, refStride, refLengthsDevice,
                                         B, N, L, U, distDevice, opsDevice));
}
/** The exact log score of all n * N device-resident hypotheses under the slabs of a Batch::linear, results left on the
 *  device: scoresDevice[b][k] = forwardScore(ctcGraph(tokens[b][k][0 .. len), blank) o emissions_b[0 .. T_b)), len =
 *  clamp(lengthsDevice[b][k], 0, L), nothing subtracted.  tokensDevice int32 n * N rows of width L, rowStride (>= L)
 *  apart; lengthsDevice int32 [n][N] (device memory); maxLength 1 .. 4096 bounds len (longer ones score -inf, as do
 *  hypotheses that do not fit, tokens outside 0 .. C - 1 and T_b == 0); frames (host, [n]): T_b, null = the rows the
 *  batch carries.  One launch, no copy back, no wait -- gtnx_batch_ctc_score */
inline void ctcScore(const Batch& ems, const int* tokensDevice, int64_t rowStride, const int* lengthsDevice, int N, int L,
                     int maxLength, float* scoresDevice, int blank = 0, const int* frames = nullptr) {
  detail::check(gtnx_batch_ctc_score(ems.handle(), frames, blank, tokensDevice, rowStride, lengthsDevice, N, L, maxLength,
                                     scoresDevice));
}
/** gradDevice[b][t][c] = sum over k of weightsDevice[b][k] * d score[b][k] / d emissions[b][t][c] for the scores of
 *  ctcScore, every element of float32 [n][M][C] written (zeros where nothing lands, rows from T_b on included); pairs
 *  with a -inf score or a weight of exactly 0 add nothing.  Stateless (the alpha rows are recomputed into pooled
 *  scratch, sliced beyond 256 MiB) and bit-repeatable (fixed summation order, no atomics) -- gtnx_batch_ctc_score_grad */
inline void ctcScoreGrad(const Batch& ems, const int* tokensDevice, int64_t rowStride, const int* lengthsDevice, int N,
                         int L, int maxLength, const float* weightsDevice, float* gradDevice, int blank = 0,
                         const int* frames = nullptr) {
  detail::check(gtnx_batch_ctc_score_grad(ems.handle(), frames, blank, tokensDevice, rowStride, lengthsDevice, N, L,
                                          maxLength, weightsDevice, gradDevice));
}
/** The exact CTC log score of one device-resident acyclic token lattice per utterance under the slabs of a
 *  Batch::linear, results left on the device: scoresDevice[b] = log sum over the lattice's paths p of exp(w(p) +
 *  ctcScore(emissions_b[0 .. T_b), labels(p))), nothing subtracted.  arcsDevice int32 n rows of A arcs (src, dst, label),
 *  rowStride (>= 3 A) apart, dst-sorted; numArcsDevice / numNodesDevice int32 [n]; arcWeightsDevice float32 [n][A] or
 *  null; maxStates 1 .. 4096 bounds nodes + arcs (larger lattices score -inf, as do invalid ones and T_b == 0).  One
 *  launch, no copy back, no wait -- gtnx_batch_ctc_lattice_score */
inline void ctcLatticeScore(const Batch& ems, const int* arcsDevice, int64_t rowStride, const int* numArcsDevice,
                            const int* numNodesDevice, const float* arcWeightsDevice, int A, int maxStates,
                            float* scoresDevice, int blank = 0, const int* frames = nullptr) {
  detail::check(gtnx_batch_ctc_lattice_score(ems.handle(), frames, blank, arcsDevice, rowStride, numArcsDevice,
                                             numNodesDevice, arcWeightsDevice, A, maxStates, scoresDevice));
}
/** gradDevice[b][t][c] = weightsDevice[b] * d score[b] / d emissions[b][t][c], every element of float32 [n][M][C]
 *  written; arcGradDevice (or null) float32 [n][A] = weightsDevice[b] * d score[b] / d arc weight, the arcs' posteriors,
 *  zeros past numArcs.  Stateless (the alpha rows are recomputed into pooled scratch, sliced beyond 256 MiB) and
 *  bit-repeatable (fixed summation order, no atomics) -- gtnx_batch_ctc_lattice_score_grad */
inline void ctcLatticeScoreGrad(const Batch& ems, const int* arcsDevice, int64_t rowStride, const int* numArcsDevice,
                                const int* numNodesDevice, const float* arcWeightsDevice, int A, int maxStates,
                                const float* weightsDevice, float* gradDevice, float* arcGradDevice = nullptr,
                                int blank = 0, const int* frames = nullptr) {
  detail::check(gtnx_batch_ctc_lattice_score_grad(ems.handle(), frames, blank, arcsDevice, rowStride, numArcsDevice,
                                                  numNodesDevice, arcWeightsDevice, A, maxStates, weightsDevice,
                                                  gradDevice, arcGradDevice));
}
/** The best (lattice path, alignment) pair of one device-resident token lattice per utterance (ctcLatticeScore's
 *  lattices, blank, frames and maxStates) under the slabs of a Batch::linear, results left on the device: scoresDevice
 *  [n] the best w(p) + alignment score (-inf without a path), pathLenDevice [n] the arcs on the best path;
 *  pathArcsDevice / pathTokensDevice / startsDevice / endsDevice int32 n rows of width P, outStride (>= P) apart: the arc
 *  indices in path order, their labels, the first frame of each and one past its last, -1 from pathLen on and without a
 *  path (a path longer than P keeps its length and writes its first P); tokenScoresDevice (same layout, or null) the
 *  arc's emissions summed in frame order; frameArcsDevice (n rows of width M, frameStride >= M apart, or null) the arc of
 *  every frame, -1 on blank frames and from T_b on.  Float32 max-plus, of equal candidates the first in the forward's
 *  order: reproducible bit for bit.  No copy back, no wait -- gtnx_batch_ctc_lattice_align */
inline void ctcLatticeAlign(const Batch& ems, const int* arcsDevice, int64_t rowStride, const int* numArcsDevice,
                            const int* numNodesDevice, const float* arcWeightsDevice, int A, int maxStates,
                            float* scoresDevice, int* pathLenDevice, int* pathArcsDevice, int* pathTokensDevice,
                            int* startsDevice, int* endsDevice, float* tokenScoresDevice, int P, int64_t outStride,
                            int* frameArcsDevice = nullptr, int64_t frameStride = 0, int blank = 0,
                            const int* frames = nullptr) {
  detail::check(gtnx_batch_ctc_lattice_align(ems.handle(), frames, blank, arcsDevice, rowStride, numArcsDevice,
                                             numNodesDevice, arcWeightsDevice, A, maxStates, scoresDevice, pathLenDevice,
                                             pathArcsDevice, pathTokensDevice, startsDevice, endsDevice,
                                             tokenScoresDevice, P, outStride, frameArcsDevice, frameStride));
}
/** The ASG force-align term of all n * N device-resident hypotheses under the slabs of a Batch::linear, results left on
 *  the device: scoresDevice[b][k] = forwardScore(emissions_b[0 .. T_b) o (forceAlign(tokens[b][k][0 .. len)) o
 *  transitions)), len = clamp(lengthsDevice[b][k], 0, L), log semiring, nothing subtracted.  tableDevice float32
 *  [C + C * C] (device memory) in the arc order of criteria::asgTransitions: entry y = start[y], entry C + i * C + j =
 *  label j followed by label i.  tokensDevice / lengthsDevice / maxLength / frames as in ctcScore; tokens are labels
 *  only and equal neighbours are legal.  -inf: len == 0, T_b < len, len > maxLength, a token outside 0 .. C - 1, no
 *  alignment above -inf.  One launch, no copy back, no wait -- gtnx_batch_asg_score */
inline void asgScore(const Batch& ems, const float* tableDevice, const int* tokensDevice, int64_t rowStride,
                     const int* lengthsDevice, int N, int L, int maxLength, float* scoresDevice,
                     const int* frames = nullptr) {
  detail::check(gtnx_batch_asg_score(ems.handle(), frames, tableDevice, tokensDevice, rowStride, lengthsDevice, N, L,
                                     maxLength, scoresDevice));
}
/** The gradients of asgScore under the weights weightsDevice [n][N]: gradEmissionsDevice (or null) float32 [n][M][C],
 *  every element written (zeros where nothing lands, rows from T_b on included); gradTableDevice (or null) float32
 *  [C + C * C], every entry written; not both null.  Pairs with a -inf score or a weight of exactly 0 add nothing.
 *  Stateless (the alpha rows are recomputed into pooled scratch, sliced beyond 256 MiB) and bit-repeatable (fixed
 *  summation order, no atomics) -- gtnx_batch_asg_score_grad */
inline void asgScoreGrad(const Batch& ems, const float* tableDevice, const int* tokensDevice, int64_t rowStride,
                         const int* lengthsDevice, int N, int L, int maxLength, const float* weightsDevice,
                         float* gradEmissionsDevice, float* gradTableDevice, const int* frames = nullptr) {
  detail::check(gtnx_batch_asg_score_grad(ems.handle(), frames, tableDevice, tokensDevice, rowStride, lengthsDevice, N,
                                          L, maxLength, weightsDevice, gradEmissionsDevice, gradTableDevice));
}
/** The exact ASG log score of one device-resident acyclic token lattice per utterance (ctcLatticeScore's lattices) under
 *  the slabs of a Batch::linear and asgScore's table, results left on the device: scoresDevice[b] = log sum over the
 *  lattice's paths p of exp(w(p) + asgScore(emissions_b[0 .. T_b), table, labels(p))), nothing subtracted.  The states
 *  are the arcs: no blank, equal neighbours legal.  maxStates 1 .. 4096 bounds nodes + arcs (the CTC call's argument),
 *  maxEdges 1 .. 2^21 bounds the sum over the arcs of the in-degree of their src; lattices above either score -inf, as
 *  do invalid ones, T_b == 0 and a lattice without an alignment (one node included).  One launch, no copy back, no wait
 *  -- gtnx_batch_asg_lattice_score */
inline void asgLatticeScore(const Batch& ems, const float* tableDevice, const int* arcsDevice, int64_t rowStride,
                            const int* numArcsDevice, const int* numNodesDevice, const float* arcWeightsDevice, int A,
                            int maxStates, int maxEdges, float* scoresDevice, const int* frames = nullptr) {
  detail::check(gtnx_batch_asg_lattice_score(ems.handle(), frames, tableDevice, arcsDevice, rowStride, numArcsDevice,
                                             numNodesDevice, arcWeightsDevice, A, maxStates, maxEdges, scoresDevice));
}
/** The gradients of asgLatticeScore under the weights weightsDevice [n], each output nullable but not all three:
 *  gradEmissionsDevice float32 [n][M][C], gradTableDevice float32 [C + C * C], arcGradDevice float32 [n][A] (the arcs'
 *  posteriors times the weight, zeros past numArcs); every element of an output is written.  Stateless (alpha rows and
 *  one cell per edge in pooled scratch, sliced beyond 256 MiB) and bit-repeatable (fixed summation order, no atomics)
 *  -- gtnx_batch_asg_lattice_score_grad */
inline void asgLatticeScoreGrad(const Batch& ems, const float* tableDevice, const int* arcsDevice, int64_t rowStride,
                                const int* numArcsDevice, const int* numNodesDevice, const float* arcWeightsDevice, int A,
                                int maxStates, int maxEdges, const float* weightsDevice, float* gradEmissionsDevice,
                                float* gradTableDevice, float* arcGradDevice, const int* frames = nullptr) {
  detail::check(gtnx_batch_asg_lattice_score_grad(ems.handle(), frames, tableDevice, arcsDevice, rowStride,
                                                  numArcsDevice, numNodesDevice, arcWeightsDevice, A, maxStates, maxEdges,
                                                  weightsDevice, gradEmissionsDevice, gradTableDevice, arcGradDevice));
}
/** numSamples alignments of every chain of a Batch::linear drawn from the posterior of emissions o transitions (forward
 *  filtering, backward sampling; inverse CDF in label order, Philox4x32-10 keyed by `seed`), plus the merge of equal
 *  neighbours, results left on the device: tableDevice float32 [C + C * C] (start scores, then arc C + i * C + j = j ->
 *  i); tokensDevice int32 [n][numSamples][rowStride] (the merged alignment, then -1 up to the row's width M),
 *  lengthsDevice int32 [n][numSamples], logqDevice (may be null) float32 [n][numSamples] the log-probability of the
 *  drawn alignment, labelsDevice (may be null) int32 [n][numSamples][rowStride] the frame labels, logzDevice (may be
 *  null) float32 [n] the log partition function.  No alignment of finite score or T_b = 0: -1, 0, -inf, -inf.
 *  numSamples 1 .. 1024, 1 .. 1024 labels; frames (host, [n]): T_b, null = the rows the batch carries.  No copy back,
 *  no wait, rows from T_b on are never read -- gtnx_batch_asg_sample */
inline void asgSample(const Batch& ems, const float* tableDevice, int* tokensDevice, int64_t rowStride,
                      int* lengthsDevice, float* logqDevice = nullptr, int* labelsDevice = nullptr,
                      float* logzDevice = nullptr, int numSamples = 4, uint64_t seed = 0, float temperature = 1.0f,
                      const int* frames = nullptr) {
  detail::check(gtnx_batch_asg_sample(ems.handle(), frames, tableDevice, numSamples, seed, temperature, tokensDevice,
                                      rowStride, lengthsDevice, logqDevice, labelsDevice, logzDevice));
}
/** ASG prefix beam search with N-best output over a Batch::linear, results left on the device: the hypotheses are the
 *  label sequences without equal neighbours (what viterbiDecode's collapsed rows can hold), each summed over all of its
 *  alignments under emissions o transitions -- unpruned, asgScore of the tokens.  tableDevice float32 [C + C * C]
 *  (device memory) in the arc order of criteria::asgTransitions: entry c = start[c], entry C + i * C + j = label j
 *  followed by label i; an entry that is not finite forbids its bigram or first label.  tokensDevice int32
 *  [n][nbest][rowStride] (the labels of hypothesis r, then -1 up to the row's width M), lengthsDevice int32 [n][nbest],
 *  scoresDevice float32 [n][nbest]; slots without a hypothesis: -1, 0, -inf.  beamSize 1 .. 64 prefixes, the cutoffTopN
 *  (1 .. 32) best labels of a frame for stays and extensions alike, nbest <= beamSize; frames (host, [n]): T_b, null =
 *  the rows the batch carries.  Two launches, no copy back, no wait, rows from T_b on are never read --
 *  gtnx_batch_asg_beam_decode */
inline void asgBeamDecode(const Batch& ems, const float* tableDevice, int* tokensDevice, int64_t rowStride,
                          int* lengthsDevice, float* scoresDevice, int beamSize = 16, int cutoffTopN = 16, int nbest = 1,
                          const int* frames = nullptr) {
  detail::check(gtnx_batch_asg_beam_decode(ems.handle(), frames, tableDevice, beamSize, cutoffTopN, nbest, tokensDevice,
                                           rowStride, lengthsDevice, scoresDevice));
}
/** The same search with a compiled LM graph fused into the ranking: every prefix also carries L and its LM state, an
 *  extension adds lmWeight * (weight of the walk of (state, label)) + insertionBonus to L and is dropped when the walk
 *  forbids the label; candidates rank by acoustic score + L; stays, merging and the token sets stay acoustic, and
 *  tableDevice is still the criterion's own table.  scoresDevice gets acoustic + L, amScoresDevice (optional) the
 *  acoustic score alone -- unpruned, asgScore of the tokens -- gtnx_batch_asg_beam_decode_graph */
inline void asgBeamDecode(const Batch& ems, const float* tableDevice, const LmGraph& lm, float lmWeight,
                          float insertionBonus, int* tokensDevice, int64_t rowStride, int* lengthsDevice,
                          float* scoresDevice, float* amScoresDevice = nullptr, int beamSize = 16, int cutoffTopN = 16,
                          int nbest = 1, const int* frames = nullptr) {
  detail::check(gtnx_batch_asg_beam_decode_graph(ems.handle(), frames, tableDevice, beamSize, cutoffTopN, nbest,
                                                 lm.handle(), lmWeight, insertionBonus, tokensDevice, rowStride,
                                                 lengthsDevice, scoresDevice, amScoresDevice));
}
/** The best alignment of all n * N device-resident hypotheses (the form of ctcScore) under the slabs of a Batch::linear,
 *  results left on the device: scoresDevice [n][N] the Viterbi score (-inf without a path); startsDevice / endsDevice
 *  int32 n * N rows of width L, outStride (>= L) apart: the first frame of token i and one past its last, -1 for i >= len
 *  and without a path; tokenScoresDevice (same layout, or null) the token's emissions summed in frame order;
 *  frameTokensDevice (n * N rows of width M, frameStride >= M apart, or null) the token index of every frame, -1 on
 *  blank frames and from T_b on.  Float32 max-plus with the tie rule of viterbiAlign: reproducible bit for bit.  No copy
 *  back, no wait -- gtnx_batch_ctc_token_align */
inline void ctcTokenAlign(const Batch& ems, const int* tokensDevice, int64_t rowStride, const int* lengthsDevice, int N,
                          int L, int maxLength, float* scoresDevice, int* startsDevice, int* endsDevice,
                          float* tokenScoresDevice, int64_t outStride, int* frameTokensDevice = nullptr,
                          int64_t frameStride = 0, int blank = 0, const int* frames = nullptr) {
  detail::check(gtnx_batch_ctc_token_align(ems.handle(), frames, blank, tokensDevice, rowStride, lengthsDevice, N, L,
                                           maxLength, scoresDevice, startsDevice, endsDevice, tokenScoresDevice,
                                           outStride, frameTokensDevice, frameStride));
}
/** The best ASG alignment of all n * N device-resident hypotheses (the form and the table of asgScore) under the slabs
 *  of a Batch::linear, results left on the device: the outputs are those of ctcTokenAlign, frameTokensDevice never -1
 *  inside a path (ASG has no blank).  Positions i = 0 .. len - 1, a frame enters i from i or i - 1; float32 max-plus
 *  alpha + (w + e), of two equal candidates the step, as viterbiAlign's ASG launch: reproducible bit for bit.  No path
 *  where asgScore gives -inf.  No copy back, no wait -- gtnx_batch_asg_token_align */
inline void asgTokenAlign(const Batch& ems, const float* tableDevice, const int* tokensDevice, int64_t rowStride,
                          const int* lengthsDevice, int N, int L, int maxLength, float* scoresDevice, int* startsDevice,
                          int* endsDevice, float* tokenScoresDevice, int64_t outStride,
                          int* frameTokensDevice = nullptr, int64_t frameStride = 0, const int* frames = nullptr) {
  detail::check(gtnx_batch_asg_token_align(ems.handle(), frames, tableDevice, tokensDevice, rowStride, lengthsDevice, N,
                                           L, maxLength, scoresDevice, startsDevice, endsDevice, tokenScoresDevice,
                                           outStride, frameTokensDevice, frameStride));
}
inline void backward(const Batch& a, bool retainGraph = false) { detail::check(gtnx_batch_backward(a.handle(), retainGraph)); }
/** One CTC criterion step in ONE launch, no batch record and no tape: losses, emission gradients and (targetGrad) the
 *  targets' arc gradients of n utterances over a device tensor [n][T][C] -- bit for bit what ctcTargets, linear,
 *  intersect, the two forwardScore, subtract and backward compute.  ctcLossStepOk (a pure host function) says whether the
 *  batch is one the launch takes; gtn::criteria::ctcLossBatch asks it and falls back to those operations.
 *  gtnx_batch_ctc_loss_step has the contract. */
inline bool ctcLossStepOk(const int* labels, const int* lengths, int n, int T, int C, int blank, const void* emissionsDevice,
                          const void* gradDevice) {
  int ok = 0;
  detail::check(gtnx_batch_ctc_loss_step_ok(labels, lengths, n, T, C, blank, emissionsDevice, gradDevice, &ok));
  return ok != 0;
}
inline void ctcLossStep(const void* emissionsDevice, const int* labels, const int* lengths, int n, int T, int C, int blank,
                        void* lossDevice, void* gradDevice, bool targetGrad = true, void* targetGradDevice = nullptr) {
  detail::check(gtnx_batch_ctc_loss_step(emissionsDevice, labels, lengths, n, T, C, blank, lossDevice, gradDevice,
                                         targetGrad ? 1 : 0, targetGradDevice));
}
} // namespace batched

} // namespace gtn
