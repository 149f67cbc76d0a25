// criteria_capi.cpp -- C entry points of the batched criteria (libgtn_criteria.so), for
// callers that are not C++: gtn_amd/torch_loss.py binds gtn_ctc_loss_n with ctypes.
// Built with plain g++ against include/gtn and libgtn_amd.so.
// Every function returns 0, or -1 with the message in gtn_criteria_last_error().
#include <cstring>
#include <string>

#include <map>
#include <mutex>

#include "asg_criterion.h"
#include "ctc_criterion.h"
#include "edit_distance.h"

#define GTN_EXPORT extern "C" __attribute__((visibility("default")))

namespace {
thread_local std::string g_err;

template <class F>
int guarded(F&& body) {
  try {
    body();
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

// the transitions STRUCTURE per N is kept across calls (a trainer only changes the weights); a caller holds `mu` for as
// long as it uses the graph
struct TransitionsCache {
  std::mutex mu;
  std::map<int, gtn::Graph>* graphs = new std::map<int, gtn::Graph>();  // never destroyed: outlives the engine's teardown
};
TransitionsCache g_loss_transitions;    // (of its own: the loss's cached graph carries gradient state between calls)
TransitionsCache g_nograd_transitions;  // (gtn_asg_align_n and gtn_asg_decode_n)

gtn::Graph& transitions_for(TransitionsCache& cache, int N, bool calc_grad) {
  auto it = cache.graphs->find(N);
  if (it == cache.graphs->end()) {
    it = cache.graphs->emplace(N, gtn::criteria::asgTransitions(N)).first;
    it->second.setCalcGrad(calc_grad);
  }
  return it->second;
}
}  // namespace

GTN_EXPORT const char* gtn_criteria_last_error(void) { return g_err.c_str(); }

// emissions: DEVICE float [B][T][C]; targets: host int32, concatenated; lengths: host int32 [B];
// loss: DEVICE float [B]; grad: DEVICE float [B][T][C] or null (then no backward pass).
GTN_EXPORT int gtn_ctc_loss_n(const void* emissions, const int* targets, const int* lengths, int B, int T, int C,
                              int blank, void* loss, void* grad) {
  return guarded([&] {
    gtn::criteria::ctcLossBatch(emissions, targets, lengths, B, T, C, blank, loss, grad, /*targetGrad=*/false);
  });
}

// The same over a PADDED batch: frames: host int32 [B], utterance b's frame count (1 .. T) -- its loss is that of
// emissions[b][:frames[b]], the pad rows are never read and rows [frames[b], T) of grad are 0.
GTN_EXPORT int gtn_ctc_loss_frames_n(const void* emissions, const int* targets, const int* lengths, int B, int T, int C,
                                     int blank, const int* frames, void* loss, void* grad) {
  return guarded([&] {
    gtn::criteria::ctcLossBatch(emissions, targets, lengths, B, T, C, blank, loss, grad, /*targetGrad=*/false, nullptr,
                                nullptr, frames);
  });
}

// CTC forced alignment.  emissions: DEVICE float [B][T][C]; targets / lengths: host int32 (concatenated / [B]);
// frames: host int32 [B] or null; labels: DEVICE int32 [B][T]; tokens: DEVICE int32 [B][T] or null; scores: DEVICE
// float [B] or null.
GTN_EXPORT int gtn_ctc_align_n(const void* emissions, const int* targets, const int* lengths, int B, int T, int C,
                               int blank, const int* frames, void* labels, void* tokens, void* scores) {
  return guarded([&] {
    gtn::criteria::ctcAlignBatch(emissions, targets, lengths, B, T, C, blank, frames, labels, tokens, scores);
  });
}

// CTC best-path decode.  emissions: DEVICE float [B][T][C]; blank: the label the collapse drops (< 0: none); frames: host
// int32 [B] or null; labels: DEVICE int32 [B][T]; scores: DEVICE float [B] or null; collapsed / starts: DEVICE int32
// [B][T] or null; lengths: DEVICE int32 [B] or null (starts and lengths need collapsed).
GTN_EXPORT int gtn_ctc_decode_n(const void* emissions, int B, int T, int C, int blank, const int* frames, void* labels,
                                void* scores, void* collapsed, void* starts, void* lengths) {
  return guarded([&] {
    gtn::criteria::ctcDecodeBatch(emissions, B, T, C, blank, frames, labels, scores, collapsed, starts, lengths);
  });
}

// num_samples label sequences per utterance drawn from the CTC posterior.  emissions: DEVICE float [B][T][C]; frames:
// host int32 [B] or null; tokens: DEVICE int32 [B][num_samples][T]; lengths: DEVICE int32 [B][num_samples]; logq: DEVICE
// float [B][num_samples] or null; labels: DEVICE int32 [B][num_samples][T] or null.
GTN_EXPORT int gtn_ctc_sample_n(const void* emissions, int B, int T, int C, int blank, const int* frames,
                                int num_samples, unsigned long long seed, float temperature, void* tokens,
                                void* lengths, void* logq, void* labels) {
  return guarded([&] {
    gtn::criteria::ctcSampleBatch(emissions, B, T, C, blank, frames, num_samples, seed, temperature, tokens, lengths,
                                  logq, labels);
  });
}

// CTC prefix beam search with N-best output.  emissions: DEVICE float [B][T][C]; frames: host int32 [B] or null; tokens:
// DEVICE int32 [B][nbest][T]; lengths: DEVICE int32 [B][nbest]; scores: DEVICE float [B][nbest].
GTN_EXPORT int gtn_ctc_beam_decode_n(const void* emissions, int B, int T, int C, int blank, const int* frames,
                                     int beam_size, int cutoff_top_n, int nbest, void* tokens, void* lengths,
                                     void* scores) {
  return guarded([&] {
    gtn::criteria::ctcBeamDecodeBatch(emissions, B, T, C, blank, frames, beam_size, cutoff_top_n, nbest, tokens, lengths,
                                      scores);
  });
}

// The same with a bigram table fused into the ranking.  lm: DEVICE float [C + C * C] (the arc order of asgTransitions);
// scores: acoustic + language model; am_scores: DEVICE float [B][nbest] or null, the acoustic total alone.
GTN_EXPORT int gtn_ctc_beam_decode_lm_n(const void* emissions, int B, int T, int C, int blank, const int* frames,
                                        int beam_size, int cutoff_top_n, int nbest, const void* lm, float lm_weight,
                                        float insertion_bonus, void* tokens, void* lengths, void* scores,
                                        void* am_scores) {
  return guarded([&] {
    gtn::criteria::ctcBeamDecodeBatch(emissions, B, T, C, blank, frames, beam_size, cutoff_top_n, nbest, lm, lm_weight,
                                      insertion_bonus, tokens, lengths, scores, am_scores);
  });
}

// The same with a compiled LM graph in the table's place.  lm_graph: a handle of gtnx_lm_graph_create (libgtn_amd.so),
// passed through as a pointer: both libraries live in one process.
GTN_EXPORT int gtn_ctc_beam_decode_graph_n(const void* emissions, int B, int T, int C, int blank, const int* frames,
                                           int beam_size, int cutoff_top_n, int nbest, void* lm_graph, float lm_weight,
                                           float insertion_bonus, void* tokens, void* lengths, void* scores,
                                           void* am_scores) {
  return guarded([&] {
    gtn::criteria::ctcBeamDecodeBatch(emissions, B, T, C, blank, frames, beam_size, cutoff_top_n, nbest,
                                      static_cast<gtnx_lm_graph_t>(lm_graph), lm_weight, insertion_bonus, tokens, lengths,
                                      scores, am_scores);
  });
}

// Exact CTC log scores of B * N device-resident hypotheses.  emissions: DEVICE float32 [B][T][C]; frames: HOST int [B] or
// null; tokens: DEVICE int32 [B][N][L]; lengths: DEVICE int32 [B][N]; scores: DEVICE float32 [B][N].
GTN_EXPORT int gtn_ctc_score_n(const void* emissions, int B, int T, int C, int blank, const int* frames,
                               const void* tokens, const void* lengths, int N, int L, int max_length, void* scores) {
  return guarded([&] {
    if (!scores) throw std::invalid_argument("gtn_ctc_score_n: null scores");
    gtn::criteria::ctcScoreBatch(emissions, B, T, C, blank, frames, tokens, lengths, N, L, max_length, scores);
  });
}

// ... and their gradient: grad (DEVICE float32 [B][T][C], every element written) = sum_k weights[b][k] * d score[b][k] /
// d emissions_b for weights: DEVICE float32 [B][N].
GTN_EXPORT int gtn_ctc_score_grad_n(const void* emissions, int B, int T, int C, int blank, const int* frames,
                                    const void* tokens, const void* lengths, int N, int L, int max_length,
                                    const void* weights, void* grad) {
  return guarded([&] {
    if (!weights || !grad) throw std::invalid_argument("gtn_ctc_score_grad_n: null weights or grad");
    gtn::criteria::ctcScoreBatch(emissions, B, T, C, blank, frames, tokens, lengths, N, L, max_length, nullptr, weights,
                                 grad);
  });
}

// Exact CTC log scores of one device-resident token lattice per utterance.  emissions: DEVICE float32 [B][T][C]; frames:
// HOST int [B] or null; arcs: DEVICE int32 [B][A][3]; num_arcs / num_nodes: DEVICE int32 [B]; arc_weights: DEVICE
// float32 [B][A] or null; scores: DEVICE float32 [B].
GTN_EXPORT int gtn_ctc_lattice_score_n(const void* emissions, int B, int T, int C, int blank, const int* frames,
                                       const void* arcs, const void* num_arcs, const void* num_nodes,
                                       const void* arc_weights, int A, int max_states, void* scores) {
  return guarded([&] {
    if (!scores) throw std::invalid_argument("gtn_ctc_lattice_score_n: null scores");
    gtn::criteria::ctcLatticeScoreBatch(emissions, B, T, C, blank, frames, arcs, num_arcs, num_nodes, arc_weights, A,
                                        max_states, scores);
  });
}

// ... and their gradients for weights: DEVICE float32 [B]: grad (DEVICE float32 [B][T][C], every element written) and
// arc_grad (DEVICE float32 [B][A] or null).
GTN_EXPORT int gtn_ctc_lattice_score_grad_n(const void* emissions, int B, int T, int C, int blank, const int* frames,
                                            const void* arcs, const void* num_arcs, const void* num_nodes,
                                            const void* arc_weights, int A, int max_states, const void* weights,
                                            void* grad, void* arc_grad) {
  return guarded([&] {
    if (!weights || !grad) throw std::invalid_argument("gtn_ctc_lattice_score_grad_n: null weights or grad");
    gtn::criteria::ctcLatticeScoreBatch(emissions, B, T, C, blank, frames, arcs, num_arcs, num_nodes, arc_weights, A,
                                        max_states, nullptr, weights, grad, arc_grad);
  });
}

// The best (lattice path, alignment) pair of one device-resident token lattice per utterance: the inputs of
// gtn_ctc_lattice_score_n; scores: DEVICE float32 [B]; path_len: DEVICE int32 [B]; path_arcs / path_tokens / starts /
// ends: DEVICE int32 [B][P]; token_scores: DEVICE float32 [B][P] or null; frame_arcs: DEVICE int32 [B][T] or null.
GTN_EXPORT int gtn_ctc_lattice_align_n(const void* emissions, int B, int T, int C, int blank, const int* frames,
                                       const void* arcs, const void* num_arcs, const void* num_nodes,
                                       const void* arc_weights, int A, int max_states, int P, void* scores,
                                       void* path_len, void* path_arcs, void* path_tokens, void* starts, void* ends,
                                       void* token_scores, void* frame_arcs) {
  return guarded([&] {
    gtn::criteria::ctcLatticeAlignBatch(emissions, B, T, C, blank, frames, arcs, num_arcs, num_nodes, arc_weights, A,
                                        max_states, P, scores, path_len, path_arcs, path_tokens, starts, ends,
                                        token_scores, frame_arcs);
  });
}

// The best alignment of B * N device-resident hypotheses.  emissions: DEVICE float32 [B][T][C]; frames: HOST int [B] or
// null; tokens: DEVICE int32 [B][N][L]; lengths: DEVICE int32 [B][N]; scores: DEVICE float32 [B][N]; starts / ends: DEVICE
// int32 [B][N][L]; token_scores: DEVICE float32 [B][N][L] or null; frame_tokens: DEVICE int32 [B][N][T] or null.
GTN_EXPORT int gtn_ctc_token_align_n(const void* emissions, int B, int T, int C, int blank, const int* frames,
                                     const void* tokens, const void* lengths, int N, int L, int max_length,
                                     void* scores, void* starts, void* ends, void* token_scores, void* frame_tokens) {
  return guarded([&] {
    gtn::criteria::ctcTokenAlignBatch(emissions, B, T, C, blank, frames, tokens, lengths, N, L, max_length, scores,
                                      starts, ends, token_scores, frame_tokens);
  });
}

// Edit distance of all B * N pairs (hyp[b][k], ref[b]).  hyp: DEVICE int32 [B][N][L]; hyp_lengths: DEVICE int32 [B][N];
// ref: DEVICE int32 [B][U]; ref_lengths: DEVICE int32 [B]; dist: DEVICE int32 [B][N]; ops: DEVICE int32 [B][N][3] or
// null.
GTN_EXPORT int gtn_edit_distance_n(const void* hyp, const void* hyp_lengths, const void* ref, const void* ref_lengths,
                                   int B, int N, int L, int U, void* dist, void* ops) {
  return guarded([&] { gtn::criteria::editDistanceBatch(hyp, hyp_lengths, ref, ref_lengths, B, N, L, U, dist, ops); });
}

// gtn_ctc_loss_n as benchmarks/ctc.cpp:150-165 runs it: target graphs with calcGrad = true, and THEIR gradients too.
// target_grad: DEVICE float, utterance b's arc gradients (arc ids of benchmarks/ctc.cpp:40-58's addArc order) at
// target_grad + target_grad_offsets[b]; grad must be non-null.
GTN_EXPORT int gtn_ctc_loss_target_grads_n(const void* emissions, const int* targets, const int* lengths, int B, int T,
                                           int C, int blank, void* loss, void* grad, void* target_grad,
                                           const int64_t* target_grad_offsets) {
  return guarded([&] {
    gtn::Batch ctcs;
    gtn::criteria::ctcLossBatch(emissions, targets, lengths, B, T, C, blank, loss, grad, /*targetGrad=*/true, nullptr, &ctcs);
    if (target_grad) ctcs.gradsToDevice(target_grad, target_grad_offsets);
  });
}

// ctcLossBatch as it stands, every switch of it: frames (host int32 [B]) or null; grad may be null; target_grad != 0:
// the targets are built with calcGrad = true, and target_grad_dev (DEVICE float, or null) receives their arc gradients,
// utterance b's at the running sum of the arc counts in front of it.  Which path ran -- the one-launch step or the
// graph-level operations (GTNX_CTC_STEP_FUSED=0, or a batch the launch does not take) -- is ctcLossBatch's decision.
GTN_EXPORT int gtn_ctc_loss_step_n(const void* emissions, const int* targets, const int* lengths, int B, int T, int C,
                                   int blank, const int* frames, void* loss, void* grad, int target_grad,
                                   void* target_grad_dev) {
  return guarded([&] {
    gtn::criteria::ctcLossBatch(emissions, targets, lengths, B, T, C, blank, loss, grad, target_grad != 0, nullptr, nullptr,
                                frames, target_grad_dev);
  });
}

// ASG over a shared transitions graph.  emissions: DEVICE float [B][T][N]; targets / lengths:
// host int32 (concatenated / [B]); trans_w: DEVICE float [N + N*N] in the arc order of
// gtn::criteria::asgTransitions BEFORE its arcSort (arc i: <s> -> i; arc N + i*N + j: j -> i);
// loss: DEVICE float [B]; grad_em: DEVICE [B][T][N] or null; grad_trans: DEVICE [N + N*N] or null.
namespace {
void asg_loss_impl(const void* emissions, const int* targets, const int* lengths, int B, int T, int N, const void* trans_w,
                   const int* frames, void* loss, void* grad_em, void* grad_trans) {
  if (frames)  // (before the weights are handed to the engine: no device is asked for an invalid call)
    for (int b = 0; b < B; ++b)
      if (frames[b] < 1 || frames[b] > T) throw std::invalid_argument("[gtn_asg_loss_frames_n] a frame count outside 1 .. T");
  std::lock_guard<std::mutex> lk(g_loss_transitions.mu);
  gtn::Graph& trans = transitions_for(g_loss_transitions, N, grad_trans != nullptr);
  trans.setCalcGrad(grad_trans != nullptr);
  trans.zeroGrad();
  trans.setWeightsDevice(trans_w);  // arc ids are creation order: arcSort permutes lists, not ids
  gtn::criteria::asgLossBatch(emissions, targets, lengths, B, T, N, trans, loss, grad_em, frames);
  if (grad_trans) {
    gtnx_graph_t h = trans.handle();
    int64_t off = 0;
    gtn::detail::check(gtnx_grads_device_n(&h, 1, grad_trans, &off));
  }
}
}  // namespace

GTN_EXPORT int gtn_asg_loss_n(const void* emissions, const int* targets, const int* lengths, int B, int T, int N,
                              const void* trans_w, void* loss, void* grad_em, void* grad_trans) {
  return guarded([&] { asg_loss_impl(emissions, targets, lengths, B, T, N, trans_w, nullptr, loss, grad_em, grad_trans); });
}

// The same over a PADDED batch: frames: host int32 [B], utterance b's frame count (1 .. T) -- its loss is that of
// emissions[b][:frames[b]], the pad rows are never read and rows [frames[b], T) of grad_em are 0.
GTN_EXPORT int gtn_asg_loss_frames_n(const void* emissions, const int* targets, const int* lengths, int B, int T, int N,
                                     const void* trans_w, const int* frames, void* loss, void* grad_em,
                                     void* grad_trans) {
  return guarded([&] {
    if (!frames) throw std::invalid_argument("[gtn_asg_loss_frames_n] null frame counts");
    asg_loss_impl(emissions, targets, lengths, B, T, N, trans_w, frames, loss, grad_em, grad_trans);
  });
}

// The full-connect term of the ASG criterion alone.  emissions / trans_w as for gtn_asg_loss_n; frames: host int32 [B]
// (1 .. T) or null; scores: DEVICE float [B]; grad_em: DEVICE [B][T][N] or null; grad_trans: DEVICE [N + N*N] or null
// (summed over the batch with unit seeds).
GTN_EXPORT int gtn_asg_full_connect_n(const void* emissions, int B, int T, int N, const void* trans_w, const int* frames,
                                      void* scores, void* grad_em, void* grad_trans) {
  return guarded([&] {
    if (!scores) throw std::invalid_argument("[gtn_asg_full_connect_n] null scores");
    if (frames)  // (before the weights are handed to the engine: no device is asked for an invalid call)
      for (int b = 0; b < B; ++b)
        if (frames[b] < 1 || frames[b] > T)
          throw std::invalid_argument("[gtn_asg_full_connect_n] a frame count outside 1 .. T");
    std::lock_guard<std::mutex> lk(g_loss_transitions.mu);
    gtn::Graph& trans = transitions_for(g_loss_transitions, N, grad_trans != nullptr);
    trans.setCalcGrad(grad_trans != nullptr);
    trans.zeroGrad();
    trans.setWeightsDevice(trans_w);  // arc ids are creation order: arcSort permutes lists, not ids
    gtn::criteria::asgFullConnectBatch(emissions, B, T, N, trans, scores, grad_em, frames);
    if (grad_trans) {
      gtnx_graph_t h = trans.handle();
      int64_t off = 0;
      gtn::detail::check(gtnx_grads_device_n(&h, 1, grad_trans, &off));
    }
  });
}

// ASG forced alignment.  emissions / targets / lengths / trans_w as for gtn_asg_loss_n; frames: host int32 [B] or null;
// labels: DEVICE int32 [B][T]; tokens: DEVICE int32 [B][T] or null; scores: DEVICE float [B] or null.
GTN_EXPORT int gtn_asg_align_n(const void* emissions, const int* targets, const int* lengths, int B, int T, int N,
                               const void* trans_w, const int* frames, void* labels, void* tokens, void* scores) {
  return guarded([&] {
    std::lock_guard<std::mutex> lk(g_nograd_transitions.mu);
    gtn::Graph& trans = transitions_for(g_nograd_transitions, N, false);
    trans.setWeightsDevice(trans_w);  // arc ids are creation order: arcSort permutes lists, not ids
    gtn::criteria::asgAlignBatch(emissions, targets, lengths, B, T, N, trans, frames, labels, tokens, scores);
  });
}

// ASG decode.  emissions: DEVICE [B][T][N]; trans_w: DEVICE [N + N*N] as for gtn_asg_loss_n; frames: host int32 [B] or
// null; labels: DEVICE int32 [B][T]; scores: DEVICE float [B] or null; collapsed: DEVICE int32 [B][T] or null; lengths:
// DEVICE int32 [B] or null (needs collapsed).
GTN_EXPORT int gtn_asg_decode_n(const void* emissions, int B, int T, int N, const void* trans_w, const int* frames,
                                void* labels, void* scores, void* collapsed, void* lengths) {
  return guarded([&] {
    std::lock_guard<std::mutex> lk(g_nograd_transitions.mu);
    gtn::Graph& trans = transitions_for(g_nograd_transitions, N, false);
    trans.setWeightsDevice(trans_w);  // arc ids are creation order: arcSort permutes lists, not ids
    gtn::criteria::asgDecodeBatch(emissions, B, T, N, trans, frames, labels, scores, collapsed, lengths);
  });
}

// ASG force-align scores of B * N device-resident hypotheses.  emissions: DEVICE float32 [B][T][C]; table: DEVICE float32
// [C + C*C] as for gtn_asg_loss_n; frames: HOST int [B] or null; tokens: DEVICE int32 [B][N][L]; lengths: DEVICE int32
// [B][N]; scores: DEVICE float32 [B][N].
GTN_EXPORT int gtn_asg_score_n(const void* emissions, int B, int T, int C, const void* table, const int* frames,
                               const void* tokens, const void* lengths, int N, int L, int max_length, void* scores) {
  return guarded([&] {
    if (!scores) throw std::invalid_argument("gtn_asg_score_n: null scores");
    gtn::criteria::asgScoreBatch(emissions, B, T, C, table, frames, tokens, lengths, N, L, max_length, scores);
  });
}

// num_samples alignments per utterance drawn from the posterior of emissions o transitions, equal neighbours merged.
// emissions: DEVICE float [B][T][C]; table: DEVICE float [C + C * C]; frames: host int32 [B] or null; tokens: DEVICE
// int32 [B][num_samples][T]; lengths: DEVICE int32 [B][num_samples]; logq: DEVICE float [B][num_samples] or null; labels:
// DEVICE int32 [B][num_samples][T] or null; logz: DEVICE float [B] or null.
GTN_EXPORT int gtn_asg_sample_n(const void* emissions, int B, int T, int C, const void* table, const int* frames,
                                int num_samples, unsigned long long seed, float temperature, void* tokens,
                                void* lengths, void* logq, void* labels, void* logz) {
  return guarded([&] {
    gtn::criteria::asgSampleBatch(emissions, B, T, C, table, frames, num_samples, seed, temperature, tokens, lengths,
                                  logq, labels, logz);
  });
}

// ASG prefix beam search with N-best output.  emissions: DEVICE float32 [B][T][C]; table: DEVICE float32 [C + C*C] as for
// gtn_asg_score_n; frames: HOST int [B] or null; tokens: DEVICE int32 [B][nbest][T]; lengths: DEVICE int32 [B][nbest];
// scores: DEVICE float32 [B][nbest].  The rows are what gtn_asg_score_n and gtn_edit_distance_n read.
GTN_EXPORT int gtn_asg_beam_decode_n(const void* emissions, int B, int T, int C, const void* table, const int* frames,
                                     int beam_size, int cutoff_top_n, int nbest, void* tokens, void* lengths,
                                     void* scores) {
  return guarded([&] {
    gtn::criteria::asgBeamDecodeBatch(emissions, B, T, C, table, frames, beam_size, cutoff_top_n, nbest, tokens, lengths,
                                      scores);
  });
}

// The same with a compiled LM graph fused into the ranking.  lm_graph: a handle of gtnx_lm_graph_create (libgtn_amd.so),
// passed through as a pointer: both libraries live in one process.  am_scores: DEVICE float32 [B][nbest] or null.
GTN_EXPORT int gtn_asg_beam_decode_graph_n(const void* emissions, int B, int T, int C, const void* table,
                                           const int* frames, int beam_size, int cutoff_top_n, int nbest, void* lm_graph,
                                           float lm_weight, float insertion_bonus, void* tokens, void* lengths,
                                           void* scores, void* am_scores) {
  return guarded([&] {
    gtn::criteria::asgBeamDecodeBatch(emissions, B, T, C, table, frames, beam_size, cutoff_top_n, nbest,
                                      static_cast<gtnx_lm_graph_t>(lm_graph), lm_weight, insertion_bonus, tokens, lengths,
                                      scores, am_scores);
  });
}

// ... and their gradients under weights: DEVICE float32 [B][N]: grad_em (DEVICE float32 [B][T][C], every element
// written) and grad_table (DEVICE float32 [C + C*C], every entry written); either may be null, not both.
GTN_EXPORT int gtn_asg_score_grad_n(const void* emissions, int B, int T, int C, const void* table, const int* frames,
                                    const void* tokens, const void* lengths, int N, int L, int max_length,
                                    const void* weights, void* grad_em, void* grad_table) {
  return guarded([&] {
    if (!weights || (!grad_em && !grad_table)) throw std::invalid_argument("gtn_asg_score_grad_n: null weights or no gradient");
    gtn::criteria::asgScoreBatch(emissions, B, T, C, table, frames, tokens, lengths, N, L, max_length, nullptr, weights,
                                 grad_em, grad_table);
  });
}

// Exact ASG log scores of one device-resident token lattice per utterance.  emissions: DEVICE float32 [B][T][C]; table:
// DEVICE float32 [C + C*C] as for gtn_asg_score_n; frames: HOST int [B] or null; arcs: DEVICE int32 [B][A][3]; num_arcs /
// num_nodes: DEVICE int32 [B]; arc_weights: DEVICE float32 [B][A] or null; scores: DEVICE float32 [B].
GTN_EXPORT int gtn_asg_lattice_score_n(const void* emissions, int B, int T, int C, const void* table, const int* frames,
                                       const void* arcs, const void* num_arcs, const void* num_nodes,
                                       const void* arc_weights, int A, int max_states, int max_edges, void* scores) {
  return guarded([&] {
    if (!scores) throw std::invalid_argument("gtn_asg_lattice_score_n: null scores");
    gtn::criteria::asgLatticeScoreBatch(emissions, B, T, C, table, frames, arcs, num_arcs, num_nodes, arc_weights, A,
                                        max_states, max_edges, scores);
  });
}

// ... and their gradients under weights: DEVICE float32 [B]: grad_em (DEVICE float32 [B][T][C]), grad_table (DEVICE
// float32 [C + C*C]) and arc_grad (DEVICE float32 [B][A]), every element written; each may be null, not all three.
GTN_EXPORT int gtn_asg_lattice_score_grad_n(const void* emissions, int B, int T, int C, const void* table,
                                            const int* frames, const void* arcs, const void* num_arcs,
                                            const void* num_nodes, const void* arc_weights, int A, int max_states,
                                            int max_edges, const void* weights, void* grad_em, void* grad_table,
                                            void* arc_grad) {
  return guarded([&] {
    if (!weights || (!grad_em && !grad_table && !arc_grad))
      throw std::invalid_argument("gtn_asg_lattice_score_grad_n: null weights or no gradient");
    gtn::criteria::asgLatticeScoreBatch(emissions, B, T, C, table, frames, arcs, num_arcs, num_nodes, arc_weights, A,
                                        max_states, max_edges, nullptr, weights, grad_em, grad_table, arc_grad);
  });
}

// The best ASG alignment of B * N device-resident hypotheses.  emissions: DEVICE float32 [B][T][C]; table: DEVICE float32
// [C + C*C] as for gtn_asg_score_n; frames: HOST int [B] or null; tokens: DEVICE int32 [B][N][L]; lengths: DEVICE int32
// [B][N]; scores: DEVICE float32 [B][N]; starts / ends: DEVICE int32 [B][N][L]; token_scores: DEVICE float32 [B][N][L] or
// null; frame_tokens: DEVICE int32 [B][N][T] or null.
GTN_EXPORT int gtn_asg_token_align_n(const void* emissions, int B, int T, int C, const void* table, const int* frames,
                                     const void* tokens, const void* lengths, int N, int L, int max_length,
                                     void* scores, void* starts, void* ends, void* token_scores, void* frame_tokens) {
  return guarded([&] {
    gtn::criteria::asgTokenAlignBatch(emissions, B, T, C, table, frames, tokens, lengths, N, L, max_length, scores,
                                      starts, ends, token_scores, frame_tokens);
  });
}
