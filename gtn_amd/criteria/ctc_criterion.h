// ctc_criterion.h -- the CTC criterion of benchmarks/ctc.cpp:40-58,150-165 (same as
// examples/ctc.cpp:21-41 and bindings/python/examples/pytorch_loss.py) written against the
// drop-in C++ API of include/gtn, batched: host threads build the target graphs, the graph
// functions run as batch-of-graphs launches on the GPU, losses and emission gradients stay
// on the device.  Header-only; used by bench_native/ctc_step.cpp and by
// gtn_amd/criteria/criteria_capi.cpp (the PyTorch loss).
#pragma once

#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "gtn/gtn.h"

namespace gtn {
namespace criteria {

/** target acceptor: 2U+1 states, blank at even states, skip arcs between different labels */
inline Graph ctcTargetGraph(const std::vector<int>& target, int blank = 0, bool calcGrad = true) {
  // the graph of benchmarks/ctc.cpp:40-58, handed to the engine in two bulk calls (same node and
  // arc order as the reference's addNode / addArc loop)
  const int L = 2 * (int)target.size() + 1;
  std::vector<uint8_t> st(L, 0), ac(L, 0);
  std::vector<int> src, dst, lab;
  src.reserve(3 * L);
  dst.reserve(3 * L);
  lab.reserve(3 * L);
  for (int l = 0; l < L; l++) {
    const int idx = (l - 1) / 2;
    st[l] = l == 0;
    ac[l] = l == L - 1 || l + 2 == L;
    const int label = l % 2 ? target[idx] : blank;
    src.push_back(l), dst.push_back(l), lab.push_back(label);
    if (l > 0) src.push_back(l - 1), dst.push_back(l), lab.push_back(label);
    if (l % 2 && l > 1 && label != target[idx - 1]) src.push_back(l - 2), dst.push_back(l), lab.push_back(label);
  }
  Graph ctc(calcGrad);
  detail::check(gtnx_graph_add_nodes(ctc.handle(), L, st.data(), ac.data()));
  detail::check(gtnx_graph_add_arcs(ctc.handle(), (int)src.size(), src.data(), dst.data(), lab.data(), lab.data(), nullptr));
  ctc.arcSort();
  return ctc;
}

struct CtcStepTimes {
  double build = 0, linear = 0, intersect = 0, forward = 0, backward = 0;
};

/** forward + backward of  loss_b = forwardScore(emissions_b) - forwardScore(target_b ∩ emissions_b)
 *  for a batch -- benchmarks/ctc.cpp:150-165 with one Batch per call instead of parallelMap over
 *  per-utterance graphs.  `emissions`: device [B][T][C], read in place; `lossDev`: device [B];
 *  `gradDev`: device [B][T][C] (d loss / d emissions, written in place) or null.  Targets may have
 *  different lengths.  `frames` (host [B], or null): a padded batch -- utterance b has frames[b] <= T frames, the
 *  loss is that of emissions_b[:frames[b]], rows past them are never read and their gradient is 0.
 *  A batch with a gradient buffer, no `targetsOut`, full frame counts and a shape the engine's one-launch step takes
 *  (gtnx_batch_ctc_loss_step_ok) runs as that ONE launch; GTNX_CTC_STEP_FUSED=0 keeps the graph-level operations. */
inline void ctcLossBatch(
    const void* emissions,
    const int* labels,   // target sequences back to back
    const int* lengths,  // [B]
    int B,
    int T,
    int C,
    int blank,
    void* lossDev,
    void* gradDev,
    bool targetGrad = true,  // benchmarks/ctc.cpp builds its targets with calcGrad = true
    CtcStepTimes* times = nullptr,
    Batch* targetsOut = nullptr,  // the target acceptors (their gradients populated when targetGrad) handed back
    const int* frames = nullptr,
    void* targetGradDev = nullptr) {  // device float, or null: the targets' arc gradients (targetGrad), utterance b's at
                                      // the running sum of the arc counts in front of it
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  if (frames)  // (before anything is launched)
    for (int b = 0; b < B; ++b)
      if (frames[b] < 1 || frames[b] > T) throw std::invalid_argument("[ctcLossBatch] a frame count outside 1 .. T");
  // The whole step as ONE launch (gtnx_batch_ctc_loss_step: target records, both band sweeps and the loss by one
  // workgroup per utterance) when the batch is one that launch takes; everything else, and GTNX_CTC_STEP_FUSED=0 (read
  // on every call: one process can run both paths), runs the graph-level operations below.  Decided here, on the host,
  // before anything is launched; the results are the same bit for bit.
  if (gradDev && !targetsOut && B > 0) {
    bool full = true;  // (padded batches stay on the graph-level path)
    for (int b = 0; frames && b < B && full; ++b) full = frames[b] == T;
    const char* sw = std::getenv("GTNX_CTC_STEP_FUSED");
    int ok = 0;
    if (full && !(sw && sw[0] == '0' && sw[1] == 0))
      detail::check(gtnx_batch_ctc_loss_step_ok(labels, lengths, B, T, C, blank, emissions, gradDev, &ok));
    if (ok) {
      auto t0 = now();
      detail::check(gtnx_batch_ctc_loss_step(emissions, labels, lengths, B, T, C, blank, lossDev, gradDev, targetGrad ? 1 : 0,
                                             targetGrad ? targetGradDev : nullptr));
      if (times) *times = {0, 0, 0, ms(t0, now()), 0};  // (one phase carries the whole call)
      return;
    }
  }
  auto t0 = now();
  Batch ctcs = Batch::ctcTargets(labels, lengths, B, blank, targetGrad);
  auto t1 = now();
  Batch ems = Batch::linear(B, T, C, emissions, gradDev != nullptr, /*borrow=*/true, frames);
  std::vector<int64_t> off(B);
  for (int b = 0; b < B; ++b) off[b] = (int64_t)b * T * C;
  if (gradDev) ems.bindGrads(gradDev, off.data());
  auto t2 = now();
  // only forwardScore of the lattices is taken: they are never built (band.hip sweeps them)
  Batch comp = batched::intersect(ctcs, ems);
  auto t3 = now();
  // (C++ leaves the evaluation order of benchmarks/ctc.cpp:157's call arguments open; this order lets the
  //  sweep over target o emissions, which reads every emission anyway, leave forwardScore(emissions) behind)
  Batch score = batched::forwardScore(comp);
  Batch norm = batched::forwardScore(ems);
  Batch losses = batched::subtract(norm, score, lossDev);  // (written where the caller wants them: no copy below)
  auto t4 = now();
  if (gradDev) batched::backward(losses);
  auto t5 = now();
  if (times) *times = {ms(t0, t1), ms(t1, t2), ms(t2, t3), ms(t3, t4), ms(t4, t5)};
  losses.itemsToDevice(lossDev);
  if (gradDev) ems.gradsToDevice(gradDev, off.data());  // (nothing to copy when the rows were written in place)
  if (targetGradDev && targetGrad && gradDev) {
    std::vector<int64_t> goff(static_cast<size_t>(B));
    int64_t run = 0, lo = 0;
    for (int b = 0; b < B; ++b) {  // arcs of acceptor b: 2U+1 self loops, 2U steps, a skip per change of label
      const int U = lengths[b];
      goff[static_cast<size_t>(b)] = run;
      run += 4 * int64_t(U) + 1;
      for (int u = 1; u < U; ++u) run += labels[lo + u] != labels[lo + u - 1] ? 1 : 0;
      lo += U;
    }
    ctcs.gradsToDevice(targetGradDev, goff.data());
  }
  if (targetsOut) *targetsOut = std::move(ctcs);
}

inline void ctcLossBatch(
    const void* emissions,
    const std::vector<std::vector<int>>& targets,
    int T,
    int C,
    int blank,
    void* lossDev,
    void* gradDev,
    bool targetGrad = true,
    CtcStepTimes* times = nullptr) {
  std::vector<int> flat, len;
  for (auto& t : targets) {
    flat.insert(flat.end(), t.begin(), t.end());
    len.push_back((int)t.size());
  }
  ctcLossBatch(emissions, flat.data(), len.data(), (int)targets.size(), T, C, blank, lossDev, gradDev, targetGrad, times);
}

/** CTC forced alignment of a batch, results on the device: per utterance the best path of target_b ∩ emissions_b
 *  (viterbiPath, shortest.cpp:190-272) as the label of every frame (`labels`, device int32 [B][T]), the index of the
 *  frame's token in the target, -1 on blank frames (`tokens`, device int32 [B][T] or null) and the path score
 *  (`scores`, device float [B] or null).  `frames`: host [B] or null -- how many of the T rows of each utterance
 *  count; entries past them are -1.  `emissions`: device [B][T][C], read in place.  Nothing is copied back. */
inline void ctcAlignBatch(
    const void* emissions,
    const int* targets,  // target sequences back to back
    const int* lengths,  // [B]
    int B,
    int T,
    int C,
    int blank,
    const int* frames,
    void* labels,
    void* tokens,
    void* scores) {
  Batch ctcs = Batch::ctcTargets(targets, lengths, B, blank, /*calcGrad=*/false);
  Batch ems = Batch::linear(B, T, C, emissions, /*calcGrad=*/false, /*borrow=*/true);
  Batch comp = batched::intersect(ctcs, ems);
  batched::viterbiAlign(comp, static_cast<int*>(labels), T, static_cast<int*>(tokens), static_cast<float*>(scores), frames);
}

/** CTC best-path decode of a batch, results on the device: per utterance viterbiPath(emissions_b) (shortest.cpp:190-272
 *  on linearGraph(T, C)) as the label of every frame (`labelsDev`, device int32 [B][T]: the smallest label among equal
 *  maxima), the path score (`scoresDev`, device float [B] or null: the float32 sum of the row maxima in frame order),
 *  the labels with repeats merged and `blank` dropped (`collapsedDev`, device int32 [B][T] or null; blank < 0 drops
 *  nothing), the first frame of each (`startsDev`, device int32 [B][T] or null; needs collapsedDev) and how many
 *  (`lengthsDev`, device int32 [B] or null; needs collapsedDev).  `frames`: host [B] or null -- how many of the T rows of
 *  each utterance count (0 .. T); entries past them are -1, rows past them are never read, and an utterance without
 *  frames has no path.  No path (a frame with nothing above -inf, or no frames): entries -1, score -inf, length 0.
 *  `emissions`: device [B][T][C], read in place.  Two launches; nothing is copied back. */
inline void ctcDecodeBatch(
    const void* emissions,
    int B,
    int T,
    int C,
    int blank,
    const int* frames,
    void* labelsDev,
    void* scoresDev,
    void* collapsedDev,
    void* startsDev,
    void* lengthsDev) {
  Batch ems = Batch::linear(B, T, C, emissions, /*calcGrad=*/false, /*borrow=*/true);
  batched::linearDecode(ems, static_cast<int*>(labelsDev), T, static_cast<float*>(scoresDev), frames, blank,
                        static_cast<int*>(collapsedDev), static_cast<int*>(startsDev), static_cast<int*>(lengthsDev));
}

/** `numSamples` label sequences per utterance drawn from the CTC posterior, results on the device: every frame takes a
 *  label with probability exp(x / temperature) / Z over its finite entries, the alignment is collapsed
 *  (gtnx_batch_ctc_sample has the contract; Philox4x32-10 keyed by `seed`, so a seed repeats a run).  `tokensDev`: device
 *  int32 [B][numSamples][T], -1 from a sample's length on; `lengthsDev`: device int32 [B][numSamples]; `logqDev`: device
 *  float [B][numSamples] or null, the log-probability of the drawn alignment; `labelsDev`: device int32
 *  [B][numSamples][T] or null, the frame labels.  `frames`: host [B] or null -- how many of the T rows of each utterance
 *  count (0 .. T); rows past them are never read.  `emissions`: device [B][T][C], read in place.  Two launches; nothing is
 *  copied back. */
inline void ctcSampleBatch(
    const void* emissions,
    int B,
    int T,
    int C,
    int blank,
    const int* frames,
    int numSamples,
    uint64_t seed,
    float temperature,
    void* tokensDev,
    void* lengthsDev,
    void* logqDev,
    void* labelsDev) {
  Batch ems = Batch::linear(B, T, C, emissions, /*calcGrad=*/false, /*borrow=*/true);
  batched::ctcSample(ems, static_cast<int*>(tokensDev), T, static_cast<int*>(lengthsDev), static_cast<float*>(logqDev),
                     static_cast<int*>(labelsDev), blank, numSamples, seed, temperature, frames);
}

/** CTC prefix beam search of a batch with N-best output, results on the device: per utterance the `nbest` best label
 *  sequences, summed over the alignments the beam kept (gtnx_batch_ctc_beam_decode has the contract).  `tokensDev`:
 *  device int32 [B][nbest][T], -1 from a hypothesis's length on; `lengthsDev`: device int32 [B][nbest]; `scoresDev`:
 *  device float [B][nbest]; slots without a hypothesis -1, 0, -inf.  `frames`: host [B] or null -- how many of the T
 *  rows of each utterance count (0 .. T); rows past them are never read.  `emissions`: device [B][T][C], read in
 *  place.  Two launches; nothing is copied back. */
inline void ctcBeamDecodeBatch(
    const void* emissions,
    int B,
    int T,
    int C,
    int blank,
    const int* frames,
    int beamSize,
    int cutoffTopN,
    int nbest,
    void* tokensDev,
    void* lengthsDev,
    void* scoresDev) {
  Batch ems = Batch::linear(B, T, C, emissions, /*calcGrad=*/false, /*borrow=*/true);
  batched::ctcBeamDecode(ems, static_cast<int*>(tokensDev), T, static_cast<int*>(lengthsDev),
                         static_cast<float*>(scoresDev), blank, beamSize, cutoffTopN, nbest, frames);
}

/** The same search with a bigram over the labels fused into the ranking (gtnx_batch_ctc_beam_decode_lm has the
 *  contract): `lmDev` device float32 [C + C * C], the weights of asgTransitions(C) in its arc order -- what the ASG
 *  criterion learns; `lmWeight`, `insertionBonus`: the scale of a table entry and what every label adds.  `scoresDev`
 *  gets acoustic + language model, `amScoresDev` (device float [B][nbest], may be null) the acoustic total alone. */
inline void ctcBeamDecodeBatch(
    const void* emissions,
    int B,
    int T,
    int C,
    int blank,
    const int* frames,
    int beamSize,
    int cutoffTopN,
    int nbest,
    const void* lmDev,
    float lmWeight,
    float insertionBonus,
    void* tokensDev,
    void* lengthsDev,
    void* scoresDev,
    void* amScoresDev) {
  Batch ems = Batch::linear(B, T, C, emissions, /*calcGrad=*/false, /*borrow=*/true);
  batched::ctcBeamDecode(ems, static_cast<const float*>(lmDev), lmWeight, insertionBonus, static_cast<int*>(tokensDev),
                         T, static_cast<int*>(lengthsDev), static_cast<float*>(scoresDev),
                         static_cast<float*>(amScoresDev), blank, beamSize, cutoffTopN, nbest, frames);
}

/** The same search with a compiled LM graph in the table's place (gtnx_batch_ctc_beam_decode_graph has the contract):
 *  `lmGraph` is the handle of a gtn::batched::LmGraph or of gtnx_lm_graph_create -- it is passed on as it is, the engine
 *  refuses one that is not live. */
inline void ctcBeamDecodeBatch(
    const void* emissions,
    int B,
    int T,
    int C,
    int blank,
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
  Batch ems = Batch::linear(B, T, C, emissions, /*calcGrad=*/false, /*borrow=*/true);
  detail::check(gtnx_batch_ctc_beam_decode_graph(ems.handle(), frames, blank, beamSize, cutoffTopN, nbest, lmGraph,
                                                 lmWeight, insertionBonus, static_cast<int*>(tokensDev), T,
                                                 static_cast<int*>(lengthsDev), static_cast<float*>(scoresDev),
                                                 static_cast<float*>(amScoresDev)));
}

/** The exact log scores of B * N device-resident hypotheses under the B emission slabs, and (with weightsDev and gradDev)
 *  the gradient sum_k weights[b][k] * d score[b][k] / d emissions_b: `emissions` device float32 [B][T][C], read in
 *  place; `tokensDev` device int32 [B][N][L] (dense rows); `lengthsDev` device int32 [B][N]; `frames` host [B] or null;
 *  `scoresDev` device float32 [B][N] or null; `weightsDev` device float32 [B][N] and `gradDev` device float32 [B][T][C],
 *  both or neither.  gtnx_batch_ctc_score / _grad have the contract.  Nothing is copied back. */
inline void ctcScoreBatch(
    const void* emissions,
    int B,
    int T,
    int C,
    int blank,
    const int* frames,
    const void* tokensDev,
    const void* lengthsDev,
    int N,
    int L,
    int maxLength,
    void* scoresDev,
    const void* weightsDev = nullptr,
    void* gradDev = nullptr) {
  if ((weightsDev == nullptr) != (gradDev == nullptr)) {
    throw std::invalid_argument("ctcScoreBatch: weights and grad come together");
  }
  if (!scoresDev && !gradDev) {
    throw std::invalid_argument("ctcScoreBatch: neither scores nor grad asked for");
  }
  Batch ems = Batch::linear(B, T, C, emissions, /*calcGrad=*/false, /*borrow=*/true);
  if (scoresDev) {
    batched::ctcScore(ems, static_cast<const int*>(tokensDev), L, static_cast<const int*>(lengthsDev), N, L, maxLength,
                      static_cast<float*>(scoresDev), blank, frames);
  }
  if (gradDev) {
    batched::ctcScoreGrad(ems, static_cast<const int*>(tokensDev), L, static_cast<const int*>(lengthsDev), N, L,
                          maxLength, static_cast<const float*>(weightsDev), static_cast<float*>(gradDev), blank, frames);
  }
}

/** The exact CTC log scores of one device-resident token lattice per utterance under the B emission slabs, and (with
 *  weightsDev and gradDev) the gradients weights[b] * d score[b] / d (emissions_b, arc weights): `emissions` device
 *  float32 [B][T][C], read in place; `arcsDev` device int32 [B][A][3] (dense rows of (src, dst, label), dst-sorted);
 *  `numArcsDev` / `numNodesDev` device int32 [B]; `arcWeightsDev` device float32 [B][A] or null; `frames` host [B] or
 *  null; `scoresDev` device float32 [B] or null; `weightsDev` device float32 [B] and `gradDev` device float32 [B][T][C],
 *  both or neither; `arcGradDev` device float32 [B][A] or null, with gradDev only.  gtnx_batch_ctc_lattice_score / _grad
 *  have the contract.  Nothing is copied back. */
inline void ctcLatticeScoreBatch(
    const void* emissions,
    int B,
    int T,
    int C,
    int blank,
    const int* frames,
    const void* arcsDev,
    const void* numArcsDev,
    const void* numNodesDev,
    const void* arcWeightsDev,
    int A,
    int maxStates,
    void* scoresDev,
    const void* weightsDev = nullptr,
    void* gradDev = nullptr,
    void* arcGradDev = nullptr) {
  if ((weightsDev == nullptr) != (gradDev == nullptr)) {
    throw std::invalid_argument("ctcLatticeScoreBatch: weights and grad come together");
  }
  if (arcGradDev && !gradDev) {
    throw std::invalid_argument("ctcLatticeScoreBatch: the arcs' gradient comes with grad only");
  }
  if (!scoresDev && !gradDev) {
    throw std::invalid_argument("ctcLatticeScoreBatch: neither scores nor grad asked for");
  }
  Batch ems = Batch::linear(B, T, C, emissions, /*calcGrad=*/false, /*borrow=*/true);
  if (scoresDev) {
    batched::ctcLatticeScore(ems, static_cast<const int*>(arcsDev), 3 * int64_t(A), static_cast<const int*>(numArcsDev),
                             static_cast<const int*>(numNodesDev), static_cast<const float*>(arcWeightsDev), A,
                             maxStates, static_cast<float*>(scoresDev), blank, frames);
  }
  if (gradDev) {
    batched::ctcLatticeScoreGrad(ems, static_cast<const int*>(arcsDev), 3 * int64_t(A),
                                 static_cast<const int*>(numArcsDev), static_cast<const int*>(numNodesDev),
                                 static_cast<const float*>(arcWeightsDev), A, maxStates,
                                 static_cast<const float*>(weightsDev), static_cast<float*>(gradDev),
                                 static_cast<float*>(arcGradDev), blank, frames);
  }
}

/** The best (lattice path, alignment) pair of one device-resident token lattice per utterance under the B emission slabs
 *  -- which decomposition the model chose and when each of its tokens was spoken: the inputs are those of
 *  ctcLatticeScoreBatch; `scoresDev` device float32 [B]; `pathLenDev` device int32 [B]; `pathArcsDev` / `pathTokensDev` /
 *  `startsDev` / `endsDev` device int32 [B][P] (dense rows); `tokenScoresDev` device float32 [B][P] or null;
 *  `frameArcsDev` device int32 [B][T] or null.  gtnx_batch_ctc_lattice_align has the contract.  Nothing is copied
 *  back. */
inline void ctcLatticeAlignBatch(
    const void* emissions,
    int B,
    int T,
    int C,
    int blank,
    const int* frames,
    const void* arcsDev,
    const void* numArcsDev,
    const void* numNodesDev,
    const void* arcWeightsDev,
    int A,
    int maxStates,
    int P,
    void* scoresDev,
    void* pathLenDev,
    void* pathArcsDev,
    void* pathTokensDev,
    void* startsDev,
    void* endsDev,
    void* tokenScoresDev = nullptr,
    void* frameArcsDev = nullptr) {
  Batch ems = Batch::linear(B, T, C, emissions, /*calcGrad=*/false, /*borrow=*/true);
  batched::ctcLatticeAlign(ems, static_cast<const int*>(arcsDev), 3 * int64_t(A), static_cast<const int*>(numArcsDev),
                           static_cast<const int*>(numNodesDev), static_cast<const float*>(arcWeightsDev), A, maxStates,
                           static_cast<float*>(scoresDev), static_cast<int*>(pathLenDev), static_cast<int*>(pathArcsDev),
                           static_cast<int*>(pathTokensDev), static_cast<int*>(startsDev), static_cast<int*>(endsDev),
                           static_cast<float*>(tokenScoresDev), P, P, static_cast<int*>(frameArcsDev), T, blank, frames);
}

/** The best alignment of B * N device-resident hypotheses under the B emission slabs -- when each token was spoken and
 *  how well the frames support it: `emissions` device float32 [B][T][C], read in place; `tokensDev` device int32
 *  [B][N][L] and `lengthsDev` device int32 [B][N] (dense rows, what ctcBeamDecodeBatch wrote); `frames` host [B] or null;
 *  `scoresDev` device float32 [B][N]; `startsDev` / `endsDev` device int32 [B][N][L]; `tokenScoresDev` device float32
 *  [B][N][L] or null; `frameTokensDev` device int32 [B][N][T] or null.  gtnx_batch_ctc_token_align has the contract.
 *  Nothing is copied back. */
inline void ctcTokenAlignBatch(
    const void* emissions,
    int B,
    int T,
    int C,
    int blank,
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
  Batch ems = Batch::linear(B, T, C, emissions, /*calcGrad=*/false, /*borrow=*/true);
  batched::ctcTokenAlign(ems, static_cast<const int*>(tokensDev), L, static_cast<const int*>(lengthsDev), N, L,
                         maxLength, static_cast<float*>(scoresDev), static_cast<int*>(startsDev),
                         static_cast<int*>(endsDev), static_cast<float*>(tokenScoresDev), L,
                         static_cast<int*>(frameTokensDev), T, blank, frames);
}

} // namespace criteria
} // namespace gtn
