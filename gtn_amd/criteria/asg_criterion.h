// asg_criterion.h -- the ASG criterion of examples/asg.cpp:30-68 (golden values in
// test/criterion_test.cpp:182-306), batched over utterances that share ONE transitions graph:
//   loss_b = forwardScore(emissions_b o transitions)                       (full-connect)
//          - forwardScore(emissions_b o (forceAlign_b o transitions))      (force-align)
// On this engine the full-connect product is never built (compose keeps it symbolic and the
// dense-regime kernels of lazy.hip run it; 262 M arcs per utterance at C=512, T=1000); the
// force-align acceptors composed with the transitions are built on the device as band records (batch.h).
// Header-only.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <vector>

#include "gtn/gtn.h"

namespace gtn {
namespace criteria {

/** transitions over N labels: node 0 start, nodes 1..N accept; arcs 0 -> i+1 (label i), then
 *  j+1 -> i+1 (label i) for i, j in [0, N) in the order of examples/asg.cpp:36-47, i.e. arc
 *  N + i*N + j carries p(i | j).  Weights are left at 0. */
inline Graph asgTransitions(int N) {
  Graph g;
  g.addNode(true);
  for (int i = 1; i <= N; i++) {
    g.addNode(false, true);
    g.addArc(0, i, i - 1);
  }
  for (int i = 0; i < N; i++)
    for (int j = 0; j < N; j++) g.addArc(j + 1, i + 1, i);
  g.arcSort();  // by ilabel: compose(forceAlign, transitions) then searches a node's arcs
  return g;
}

/** all alignments of `target` (examples/asg.cpp:50-57): U+1 nodes, a step and a self-loop per label */
inline Graph asgForceAlign(const std::vector<int>& target) {
  Graph fal(false);
  fal.addNode(true, target.empty());
  for (size_t l = 1; l <= target.size(); l++) {
    fal.addNode(false, l == target.size());
    fal.addArc(l - 1, l, target[l - 1]);
    fal.addArc(l, l, target[l - 1]);
  }
  return fal;
}

/** forward + backward for a batch.  `emissions`: device [B][T][N], read in place; `transitions`: the graph of
 *  asgTransitions(N) with the caller's weights (its gradient accumulates over the batch, as in
 *  criterion_test.cpp:289-305); `lossDev`: device [B]; `gradDev`: device [B][T][N] or null.
 *  Written on batch records (gtn/batch.h): the force-alignment acceptors composed with the transitions are
 *  built on the device from the label sequences (what took 137 of 154 ms per batch of 512 through the
 *  ordinary compose), the full-connect term runs through the per-graph functions on the batch's elements.
 *  `frames` (host [B], or null): a padded batch -- utterance b has frames[b] <= T frames, its loss is that of
 *  emissions_b[:frames[b]], rows past them are never read and their gradient is 0.  With frame counts and N <= 128
 *  the full-connect term is one launch that walks every utterance's own rows (gtnx_batch_full_connect_stats); larger
 *  alphabets compose the elements, one group of launches per distinct length.  An utterance with fewer frames than
 *  labels has no alignment: its loss is +inf, its gradient rows hold the full-connect term's posteriors alone (the
 *  force-align term of a score of -inf is 0), and the transitions gradient likewise receives only that term of it. */
inline void asgLossBatch(
    const void* emissions,
    const int* labels,
    const int* lengths,
    int B,
    int T,
    int N,
    Graph& transitions,
    void* lossDev,
    void* gradDev,
    const int* frames = nullptr) {
  if (frames)  // (before anything is launched)
    for (int b = 0; b < B; ++b)
      if (frames[b] < 1 || frames[b] > T) throw std::invalid_argument("[asgLossBatch] a frame count outside 1 .. T");
  Batch ems = Batch::linear(B, T, N, emissions, gradDev != nullptr, /*borrow=*/true, frames);
  std::vector<int64_t> off(B);
  for (int b = 0; b < B; ++b) off[b] = (int64_t)b * T * N;
  Batch trans(std::vector<Graph>{transitions});
  SymbolicCompose symbolic;  // the full-connect product (262 M arcs per utterance at C4) is never built
  Batch fcc = batched::forwardScore(batched::compose(ems, trans));
  Batch fals = Batch::asgForceAlign(labels, lengths, B, transitions, N);
  Batch fal = batched::forwardScore(batched::compose(ems, fals));
  Batch losses = batched::subtract(fcc, fal);
  if (gradDev || transitions.calcGrad()) batched::backward(losses);
  losses.itemsToDevice(lossDev);
  if (gradDev) ems.gradsToDevice(gradDev, off.data());
}

inline void asgLossBatch(
    const void* emissions,
    const std::vector<std::vector<int>>& targets,
    int T,
    int N,
    Graph& transitions,
    void* lossDev,
    void* gradDev,
    const int* frames = nullptr) {
  std::vector<int> flat, len;
  for (auto& t : targets) {
    flat.insert(flat.end(), t.begin(), t.end());
    len.push_back((int)t.size());
  }
  asgLossBatch(emissions, flat.data(), len.data(), (int)targets.size(), T, N, transitions, lossDev, gradDev, frames);
}

/** The full-connect term of asgLossBatch on its own: scores[b] = forwardScore(emissions_b[:frames[b]] o transitions),
 *  the first half of the criterion, for criteria that subtract another numerator from it (asgLatticeScoreBatch's).
 *  `emissions`: device [B][T][N], read in place; `transitions`: the graph of asgTransitions(N) with the caller's weights
 *  (with calcGrad its gradient accumulates over the batch with unit seeds, as in asgLossBatch); `scoresDev`: device
 *  [B]; `gradDev`: device [B][T][N] or null, d scores[b] / d emissions_b, rows past frames[b] 0; `frames`: host [B]
 *  (1 .. T) or null.  The same launches asgLossBatch runs for this term; nothing new is compiled for it. */
inline void asgFullConnectBatch(
    const void* emissions,
    int B,
    int T,
    int N,
    Graph& transitions,
    void* scoresDev,
    void* gradDev,
    const int* frames = nullptr) {
  if (frames)  // (before anything is launched)
    for (int b = 0; b < B; ++b)
      if (frames[b] < 1 || frames[b] > T) throw std::invalid_argument("[asgFullConnectBatch] a frame count outside 1 .. T");
  Batch ems = Batch::linear(B, T, N, emissions, gradDev != nullptr, /*borrow=*/true, frames);
  std::vector<int64_t> off(B);
  for (int b = 0; b < B; ++b) off[b] = (int64_t)b * T * N;
  Batch trans(std::vector<Graph>{transitions});
  SymbolicCompose symbolic;  // the product is never built
  Batch fcc = batched::forwardScore(batched::compose(ems, trans));
  if (gradDev || transitions.calcGrad()) batched::backward(fcc);
  fcc.itemsToDevice(scoresDev);
  if (gradDev) ems.gradsToDevice(gradDev, off.data());
}

/** ASG forced alignment of a batch, results on the device: per utterance the best path of
 *  emissions_b o (forceAlign_b o transitions) (viterbiPath, shortest.cpp:190-272) as the label of every frame
 *  (`labelsDev`, device int32 [B][T]), the index of that label in the target (`tokensDev`, device int32 [B][T] or
 *  null; never -1 inside a path) and the path score (`scoresDev`, device float [B] or null).  `frames`: host [B] or
 *  null -- how many of the T rows of each utterance count; entries past them are -1, and an utterance with fewer
 *  frames than labels has score -inf and rows of -1.  `emissions`: device [B][T][N], read in place; `transitions`: the
 *  graph of asgTransitions(N) with the caller's weights.  One launch, nothing is copied back (N a multiple of 4, at
 *  most 2048; targets of at most 511 labels -- other shapes take the path-graph route, which has no tokens/frames). */
inline void asgAlignBatch(
    const void* emissions,
    const int* labels,
    const int* lengths,
    int B,
    int T,
    int N,
    Graph& transitions,
    const int* frames,
    void* labelsDev,
    void* tokensDev,
    void* scoresDev) {
  Batch ems = Batch::linear(B, T, N, emissions, /*calcGrad=*/false, /*borrow=*/true);
  Batch fals = Batch::asgForceAlign(labels, lengths, B, transitions, N);
  Batch comp = batched::compose(ems, fals);
  batched::viterbiAlign(comp, static_cast<int*>(labelsDev), T, static_cast<int*>(tokensDev),
                        static_cast<float*>(scoresDev), frames);
}

inline void asgAlignBatch(
    const void* emissions,
    const std::vector<std::vector<int>>& targets,
    int T,
    int N,
    Graph& transitions,
    const int* frames,
    void* labelsDev,
    void* tokensDev,
    void* scoresDev) {
  std::vector<int> flat, len;
  for (auto& t : targets) {
    flat.insert(flat.end(), t.begin(), t.end());
    len.push_back((int)t.size());
  }
  asgAlignBatch(emissions, flat.data(), len.data(), (int)targets.size(), T, N, transitions, frames, labelsDev, tokensDev,
                scoresDev);
}

/** ASG decode of a batch, results on the device: per utterance the best path of emissions_b o transitions
 *  (viterbiPath, shortest.cpp:190-272) as the label of every frame (`labelsDev`, device int32 [B][T]), the path score
 *  (`scoresDev`, device float [B] or null), the labels with runs of equal consecutive frames merged (`collapsedDev`,
 *  device int32 [B][T] or null) and how many of them (`lengthsDev`, device int32 [B] or null; needs collapsedDev).
 *  `frames`: host [B] or null -- how many of the T rows of each utterance count (0 .. T); entries past them are -1, and
 *  an utterance without frames has score -inf and length 0.  `emissions`: device [B][T][N], read in place, pad rows
 *  included (what they hold never changes a bit of any output); `transitions`: the graph of asgTransitions(N) with the
 *  caller's weights.  7 <= N <= 1023: one sweep of the padded batch and one launch, nothing is copied back; exact ties
 *  go to the smallest label.  Other N take the path-graph route, which has no frame counts. */
inline void asgDecodeBatch(
    const void* emissions,
    int B,
    int T,
    int N,
    Graph& transitions,
    const int* frames,
    void* labelsDev,
    void* scoresDev,
    void* collapsedDev,
    void* lengthsDev) {
  Batch ems = Batch::linear(B, T, N, emissions, /*calcGrad=*/false, /*borrow=*/true);
  batched::viterbiDecode(ems, transitions, static_cast<int*>(labelsDev), T, static_cast<float*>(scoresDev), frames,
                         static_cast<int*>(collapsedDev), static_cast<int*>(lengthsDev));
}

/** The force-align scores of B * N device-resident hypotheses under the B emission slabs, and (with weightsDev and at
 *  least one of gradEmDev / gradTableDev) their gradients under those weights: `emissions` device float32 [B][T][N_],
 *  read in place; `tableDev` device float32 [N_ + N_ * N_] in the arc order of asgTransitions (start scores, then
 *  arc N_ + i * N_ + j = j -> i); `tokensDev` device int32 [B][N][L] (dense rows); `lengthsDev` device int32 [B][N];
 *  `frames` host [B] or null; `scoresDev` device float32 [B][N] or null; `weightsDev` device float32 [B][N];
 *  `gradEmDev` device float32 [B][T][N_] or null; `gradTableDev` device float32 [N_ + N_ * N_] or null.
 *  gtnx_batch_asg_score / _grad have the contract.  Nothing is copied back. */
inline void asgScoreBatch(
    const void* emissions,
    int B,
    int T,
    int N_,
    const void* tableDev,
    const int* frames,
    const void* tokensDev,
    const void* lengthsDev,
    int N,
    int L,
    int maxLength,
    void* scoresDev,
    const void* weightsDev = nullptr,
    void* gradEmDev = nullptr,
    void* gradTableDev = nullptr) {
  const bool wantGrad = gradEmDev || gradTableDev;
  if ((weightsDev != nullptr) != wantGrad) {
    throw std::invalid_argument("asgScoreBatch: weights and a gradient come together");
  }
  if (!scoresDev && !wantGrad) {
    throw std::invalid_argument("asgScoreBatch: neither scores nor a gradient asked for");
  }
  Batch ems = Batch::linear(B, T, N_, emissions, /*calcGrad=*/false, /*borrow=*/true);
  if (scoresDev) {
    batched::asgScore(ems, static_cast<const float*>(tableDev), static_cast<const int*>(tokensDev), L,
                      static_cast<const int*>(lengthsDev), N, L, maxLength, static_cast<float*>(scoresDev), frames);
  }
  if (wantGrad) {
    batched::asgScoreGrad(ems, static_cast<const float*>(tableDev), static_cast<const int*>(tokensDev), L,
                          static_cast<const int*>(lengthsDev), N, L, maxLength, static_cast<const float*>(weightsDev),
                          static_cast<float*>(gradEmDev), static_cast<float*>(gradTableDev), frames);
  }
}

/** The exact ASG log scores of one device-resident token lattice per utterance under the B emission slabs, and (with
 *  weightsDev and at least one gradient) the gradients under those weights: `emissions` device float32 [B][T][N_], read
 *  in place; `tableDev` device float32 [N_ + N_ * N_] as for asgScoreBatch; `arcsDev` device int32 [B][A][3] (dense rows
 *  of (src, dst, label), dst-sorted); `numArcsDev` / `numNodesDev` device int32 [B]; `arcWeightsDev` device float32
 *  [B][A] or null; `frames` host [B] or null; `scoresDev` device float32 [B] or null; `weightsDev` device float32 [B];
 *  `gradEmDev` device float32 [B][T][N_] or null; `gradTableDev` device float32 [N_ + N_ * N_] or null; `arcGradDev`
 *  device float32 [B][A] or null.  gtnx_batch_asg_lattice_score / _grad have the contract.  Nothing is copied back. */
inline void asgLatticeScoreBatch(
    const void* emissions,
    int B,
    int T,
    int N_,
    const void* tableDev,
    const int* frames,
    const void* arcsDev,
    const void* numArcsDev,
    const void* numNodesDev,
    const void* arcWeightsDev,
    int A,
    int maxStates,
    int maxEdges,
    void* scoresDev,
    const void* weightsDev = nullptr,
    void* gradEmDev = nullptr,
    void* gradTableDev = nullptr,
    void* arcGradDev = nullptr) {
  const bool wantGrad = gradEmDev || gradTableDev || arcGradDev;
  if ((weightsDev != nullptr) != wantGrad) {
    throw std::invalid_argument("asgLatticeScoreBatch: weights and a gradient come together");
  }
  if (!scoresDev && !wantGrad) {
    throw std::invalid_argument("asgLatticeScoreBatch: neither scores nor a gradient asked for");
  }
  Batch ems = Batch::linear(B, T, N_, emissions, /*calcGrad=*/false, /*borrow=*/true);
  if (scoresDev) {
    batched::asgLatticeScore(ems, static_cast<const float*>(tableDev), static_cast<const int*>(arcsDev), 3 * int64_t(A),
                             static_cast<const int*>(numArcsDev), static_cast<const int*>(numNodesDev),
                             static_cast<const float*>(arcWeightsDev), A, maxStates, maxEdges,
                             static_cast<float*>(scoresDev), frames);
  }
  if (wantGrad) {
    batched::asgLatticeScoreGrad(ems, static_cast<const float*>(tableDev), static_cast<const int*>(arcsDev),
                                 3 * int64_t(A), static_cast<const int*>(numArcsDev),
                                 static_cast<const int*>(numNodesDev), static_cast<const float*>(arcWeightsDev), A,
                                 maxStates, maxEdges, static_cast<const float*>(weightsDev),
                                 static_cast<float*>(gradEmDev), static_cast<float*>(gradTableDev),
                                 static_cast<float*>(arcGradDev), frames);
  }
}

/** `numSamples` alignments per utterance drawn from the posterior of emissions o transitions, results on the device:
 *  forward filtering, backward sampling, then equal neighbours merged (gtnx_batch_asg_sample has the contract;
 *  Philox4x32-10 keyed by `seed`, so a seed repeats a run).  `emissions`: device float32 [B][T][N], read in place;
 *  `tableDev` device float32 [N + N * N] in the arc order of asgTransitions; `frames`: host [B] or null -- how many of
 *  the T rows of each utterance count (0 .. T); rows past them are never read.  `tokensDev`: device int32
 *  [B][numSamples][T], -1 from a sample's length on; `lengthsDev`: device int32 [B][numSamples]; `logqDev`: device float
 *  [B][numSamples] or null, the log-probability of the drawn alignment; `labelsDev`: device int32 [B][numSamples][T] or
 *  null, the frame labels; `logzDev`: device float [B] or null, the log partition function.  1 .. 1024 labels.  Nothing
 *  is copied back; the rows feed asgScoreBatch as they are. */
inline void asgSampleBatch(
    const void* emissions,
    int B,
    int T,
    int N,
    const void* tableDev,
    const int* frames,
    int numSamples,
    uint64_t seed,
    float temperature,
    void* tokensDev,
    void* lengthsDev,
    void* logqDev,
    void* labelsDev,
    void* logzDev) {
  Batch ems = Batch::linear(B, T, N, emissions, /*calcGrad=*/false, /*borrow=*/true);
  batched::asgSample(ems, static_cast<const float*>(tableDev), static_cast<int*>(tokensDev), T,
                     static_cast<int*>(lengthsDev), static_cast<float*>(logqDev), static_cast<int*>(labelsDev),
                     static_cast<float*>(logzDev), numSamples, seed, temperature, frames);
}

/** ASG prefix beam search of a batch, N-best results on the device: per utterance the `nbest` best label sequences
 *  without equal neighbours, each summed over all of its alignments under emissions o transitions (`tokensDev`, device
 *  int32 [B][nbest][T], -1 from each length on; `lengthsDev`, device int32 [B][nbest]; `scoresDev`, device float32
 *  [B][nbest]; slots without a hypothesis: -1, 0, -inf).  `emissions`: device float32 [B][T][N], read in place; `tableDev`
 *  device float32 [N + N * N] in the arc order of asgTransitions (start scores, then arc N + i * N + j = j -> i);
 *  `frames`: host [B] or null.  beamSize 1 .. 64, cutoffTopN 1 .. 32, nbest 1 .. beamSize.  gtnx_batch_asg_beam_decode
 *  has the contract.  Nothing is copied back; the rows feed asgScoreBatch as they are. */
inline void asgBeamDecodeBatch(
    const void* emissions,
    int B,
    int T,
    int N,
    const void* tableDev,
    const int* frames,
    int beamSize,
    int cutoffTopN,
    int nbest,
    void* tokensDev,
    void* lengthsDev,
    void* scoresDev) {
  Batch ems = Batch::linear(B, T, N, emissions, /*calcGrad=*/false, /*borrow=*/true);
  batched::asgBeamDecode(ems, static_cast<const float*>(tableDev), static_cast<int*>(tokensDev), T,
                         static_cast<int*>(lengthsDev), static_cast<float*>(scoresDev), beamSize, cutoffTopN, nbest,
                         frames);
}

/** The same search with a compiled LM graph fused into the ranking (gtnx_batch_asg_beam_decode_graph has the contract):
 *  `lmGraph` is the handle of a gtn::batched::LmGraph or of gtnx_lm_graph_create -- it is passed on as it is, the engine
 *  refuses one that is not live.  `scoresDev` gets acoustic + L, `amScoresDev` (device float32 [B][nbest], may be null)
 *  the acoustic score alone. */
inline void asgBeamDecodeBatch(
    const void* emissions,
    int B,
    int T,
    int N,
    const void* tableDev,
    const int* frames,
    int beamSize,
    int cutoffTopN,
    int nbest,
    gtnx_lm_graph_t lmGraph,
    float lmWeight,
    float insertionBonus,
    void* tokensDev,
    void* lengthsDev,
    void* scoresDev,
    void* amScoresDev) {
  Batch ems = Batch::linear(B, T, N, emissions, /*calcGrad=*/false, /*borrow=*/true);
  detail::check(gtnx_batch_asg_beam_decode_graph(ems.handle(), frames, tableDev, beamSize, cutoffTopN, nbest, lmGraph,
                                                 lmWeight, insertionBonus, static_cast<int*>(tokensDev), T,
                                                 static_cast<int*>(lengthsDev), static_cast<float*>(scoresDev),
                                                 static_cast<float*>(amScoresDev)));
}

/** The best alignment of B * N device-resident hypotheses under the B emission slabs -- when each token was spoken and
 *  how well the frames support it: `emissions` device float32 [B][T][N_], read in place; `tableDev` device float32
 *  [N_ + N_ * N_] in the arc order of asgTransitions; `tokensDev` device int32 [B][N][L] and `lengthsDev` device int32
 *  [B][N] (dense rows, what asgBeamDecodeBatch wrote when L == T); `frames` host [B] or null; `scoresDev` device float32
 *  [B][N]; `startsDev` / `endsDev` device int32 [B][N][L]; `tokenScoresDev` device float32 [B][N][L] or null;
 *  `frameTokensDev` device int32 [B][N][T] or null.  gtnx_batch_asg_token_align has the contract.  Nothing is copied
 *  back. */
inline void asgTokenAlignBatch(
    const void* emissions,
    int B,
    int T,
    int N_,
    const void* tableDev,
    const int* frames,
    const void* tokensDev,
    const void* lengthsDev,
    int N,
    int L,
    int maxLength,
    void* scoresDev,
    void* startsDev,
    void* endsDev,
    void* tokenScoresDev = nullptr,
    void* frameTokensDev = nullptr) {
  Batch ems = Batch::linear(B, T, N_, emissions, /*calcGrad=*/false, /*borrow=*/true);
  batched::asgTokenAlign(ems, static_cast<const float*>(tableDev), static_cast<const int*>(tokensDev), L,
                         static_cast<const int*>(lengthsDev), N, L, maxLength, static_cast<float*>(scoresDev),
                         static_cast<int*>(startsDev), static_cast<int*>(endsDev), static_cast<float*>(tokenScoresDev), L,
                         static_cast<int*>(frameTokensDev), T, frames);
}

} // namespace criteria
} // namespace gtn
