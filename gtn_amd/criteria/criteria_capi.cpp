// criteria_capi.cpp -- C entry points of the batched criteria (libgtn_criteria.so), for
// callers that are not C++: gtn_amd/torch_loss.py binds gtn_ctc_loss_n with ctypes.
// Built with plain g++ against include/gtn and libgtn_amd.so.
#include <cstring>
#include <string>

#include <map>
#include <mutex>

#include "asg_criterion.h"
#include "ctc_criterion.h"
#include "edit_distance.h"

namespace {
thread_local std::string g_err;
}

extern "C" __attribute__((visibility("default"))) const char* gtn_criteria_last_error(void) { return g_err.c_str(); }

// emissions: DEVICE float [B][T][C]; targets: host int32, concatenated; lengths: host int32 [B];
// loss: DEVICE float [B]; grad: DEVICE float [B][T][C] or null (then no backward pass).
// Returns 0, or -1 with the message in gtn_criteria_last_error().
extern "C" __attribute__((visibility("default"))) int gtn_ctc_loss_n(const void* emissions, const int* targets,
                                                                     const int* lengths, int B, int T, int C,
                                                                     int blank, void* loss, void* grad) {
  try {
    gtn::criteria::ctcLossBatch(emissions, targets, lengths, B, T, C, blank, loss, grad, /*targetGrad=*/false);
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

// The same over a PADDED batch: frames: host int32 [B], utterance b's frame count (1 .. T) -- its loss is that of
// emissions[b][:frames[b]], the pad rows are never read and rows [frames[b], T) of grad are 0.
extern "C" __attribute__((visibility("default"))) int gtn_ctc_loss_frames_n(const void* emissions, const int* targets,
                                                                            const int* lengths, int B, int T, int C,
                                                                            int blank, const int* frames, void* loss,
                                                                            void* grad) {
  try {
    gtn::criteria::ctcLossBatch(emissions, targets, lengths, B, T, C, blank, loss, grad, /*targetGrad=*/false, nullptr,
                                nullptr, frames);
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

// CTC forced alignment.  emissions: DEVICE float [B][T][C]; targets / lengths: host int32 (concatenated / [B]);
// frames: host int32 [B] or null; labels: DEVICE int32 [B][T]; tokens: DEVICE int32 [B][T] or null; scores: DEVICE
// float [B] or null.  Returns 0, or -1 with the message in gtn_criteria_last_error().
extern "C" __attribute__((visibility("default"))) int gtn_ctc_align_n(const void* emissions, const int* targets,
                                                                      const int* lengths, int B, int T, int C,
                                                                      int blank, const int* frames, void* labels,
                                                                      void* tokens, void* scores) {
  try {
    gtn::criteria::ctcAlignBatch(emissions, targets, lengths, B, T, C, blank, frames, labels, tokens, scores);
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

// CTC best-path decode.  emissions: DEVICE float [B][T][C]; blank: the label the collapse drops (< 0: none); frames: host
// int32 [B] or null; labels: DEVICE int32 [B][T]; scores: DEVICE float [B] or null; collapsed / starts: DEVICE int32
// [B][T] or null; lengths: DEVICE int32 [B] or null (starts and lengths need collapsed).  Returns 0, or -1 with the
// message in gtn_criteria_last_error().
extern "C" __attribute__((visibility("default"))) int gtn_ctc_decode_n(const void* emissions, int B, int T, int C,
                                                                       int blank, const int* frames, void* labels,
                                                                       void* scores, void* collapsed, void* starts,
                                                                       void* lengths) {
  try {
    gtn::criteria::ctcDecodeBatch(emissions, B, T, C, blank, frames, labels, scores, collapsed, starts, lengths);
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

// CTC prefix beam search with N-best output.  emissions: DEVICE float [B][T][C]; frames: host int32 [B] or null; tokens:
// DEVICE int32 [B][nbest][T]; lengths: DEVICE int32 [B][nbest]; scores: DEVICE float [B][nbest].  Returns 0, or -1 with
// the message in gtn_criteria_last_error().
extern "C" __attribute__((visibility("default"))) int gtn_ctc_beam_decode_n(const void* emissions, int B, int T, int C,
                                                                            int blank, const int* frames, int beam_size,
                                                                            int cutoff_top_n, int nbest, void* tokens,
                                                                            void* lengths, void* scores) {
  try {
    gtn::criteria::ctcBeamDecodeBatch(emissions, B, T, C, blank, frames, beam_size, cutoff_top_n, nbest, tokens, lengths,
                                      scores);
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

// Exact CTC log scores of B * N device-resident hypotheses.  emissions: DEVICE float32 [B][T][C]; frames: HOST int [B] or
// null; tokens: DEVICE int32 [B][N][L]; lengths: DEVICE int32 [B][N]; scores: DEVICE float32 [B][N].  Returns 0, or -1
// with the message in gtn_criteria_last_error().
extern "C" __attribute__((visibility("default"))) int gtn_ctc_score_n(const void* emissions, int B, int T, int C,
                                                                      int blank, const int* frames, const void* tokens,
                                                                      const void* lengths, int N, int L, int max_length,
                                                                      void* scores) {
  try {
    if (!scores) throw std::invalid_argument("gtn_ctc_score_n: null scores");
    gtn::criteria::ctcScoreBatch(emissions, B, T, C, blank, frames, tokens, lengths, N, L, max_length, scores);
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

// ... and their gradient: grad (DEVICE float32 [B][T][C], every element written) = sum_k weights[b][k] * d score[b][k] /
// d emissions_b for weights: DEVICE float32 [B][N].
extern "C" __attribute__((visibility("default"))) int gtn_ctc_score_grad_n(const void* emissions, int B, int T, int C,
                                                                           int blank, const int* frames,
                                                                           const void* tokens, const void* lengths,
                                                                           int N, int L, int max_length,
                                                                           const void* weights, void* grad) {
  try {
    if (!weights || !grad) throw std::invalid_argument("gtn_ctc_score_grad_n: null weights or grad");
    gtn::criteria::ctcScoreBatch(emissions, B, T, C, blank, frames, tokens, lengths, N, L, max_length, nullptr, weights,
                                 grad);
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

// Edit distance of all B * N pairs (hyp[b][k], ref[b]).  hyp: DEVICE int32 [B][N][L]; hyp_lengths: DEVICE int32 [B][N];
// ref: DEVICE int32 [B][U]; ref_lengths: DEVICE int32 [B]; dist: DEVICE int32 [B][N]; ops: DEVICE int32 [B][N][3] or
// null.  Returns 0, or -1 with the message in gtn_criteria_last_error().
extern "C" __attribute__((visibility("default"))) int gtn_edit_distance_n(const void* hyp, const void* hyp_lengths,
                                                                          const void* ref, const void* ref_lengths,
                                                                          int B, int N, int L, int U, void* dist,
                                                                          void* ops) {
  try {
    gtn::criteria::editDistanceBatch(hyp, hyp_lengths, ref, ref_lengths, B, N, L, U, dist, ops);
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

// The same, as benchmarks/ctc.cpp:150-165 runs it: target graphs with calcGrad = true, and THEIR gradients too.
// target_grad: DEVICE float, utterance b's arc gradients (arc ids of benchmarks/ctc.cpp:40-58's addArc order) at
// target_grad + target_grad_offsets[b]; grad must be non-null.
extern "C" __attribute__((visibility("default"))) int gtn_ctc_loss_target_grads_n(
    const void* emissions, const int* targets, const int* lengths, int B, int T, int C, int blank, void* loss,
    void* grad, void* target_grad, const int64_t* target_grad_offsets) {
  try {
    gtn::Batch ctcs;
    gtn::criteria::ctcLossBatch(emissions, targets, lengths, B, T, C, blank, loss, grad, /*targetGrad=*/true, nullptr, &ctcs);
    if (target_grad) ctcs.gradsToDevice(target_grad, target_grad_offsets);
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

// ASG over a shared transitions graph.  emissions: DEVICE float [B][T][N]; targets / lengths:
// host int32 (concatenated / [B]); trans_w: DEVICE float [N + N*N] in the arc order of
// gtn::criteria::asgTransitions BEFORE its arcSort (arc i: <s> -> i; arc N + i*N + j: j -> i);
// loss: DEVICE float [B]; grad_em: DEVICE [B][T][N] or null; grad_trans: DEVICE [N + N*N] or null.
namespace {
int asg_loss_impl(const void* emissions, const int* targets, const int* lengths, int B, int T, int N, const void* trans_w,
                  const int* frames, void* loss, void* grad_em, void* grad_trans) {
  try {
    if (frames)  // (before the weights are handed to the engine: no device is asked for an invalid call)
      for (int b = 0; b < B; ++b)
        if (frames[b] < 1 || frames[b] > T) throw std::invalid_argument("[gtn_asg_loss_frames_n] a frame count outside 1 .. T");
    // the transitions STRUCTURE is kept across calls (a trainer only changes the weights)
    static std::mutex mu;
    static auto* cache = new std::map<int, gtn::Graph>();  // never destroyed: outlives the engine's teardown
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache->find(N);
    if (it == cache->end()) it = cache->emplace(N, gtn::criteria::asgTransitions(N)).first;
    gtn::Graph& trans = it->second;
    trans.setCalcGrad(grad_trans != nullptr);
    trans.zeroGrad();
    trans.setWeightsDevice(trans_w);  // arc ids are creation order: arcSort permutes lists, not ids
    gtn::criteria::asgLossBatch(emissions, targets, lengths, B, T, N, trans, loss, grad_em, frames);
    if (grad_trans) {
      gtnx_graph_t h = trans.handle();
      int64_t off = 0;
      gtn::detail::check(gtnx_grads_device_n(&h, 1, grad_trans, &off));
    }
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}
}  // namespace

extern "C" __attribute__((visibility("default"))) int gtn_asg_loss_n(const void* emissions, const int* targets,
                                                                     const int* lengths, int B, int T, int N,
                                                                     const void* trans_w, void* loss, void* grad_em,
                                                                     void* grad_trans) {
  return asg_loss_impl(emissions, targets, lengths, B, T, N, trans_w, nullptr, loss, grad_em, grad_trans);
}

// The same over a PADDED batch: frames: host int32 [B], utterance b's frame count (1 .. T) -- its loss is that of
// emissions[b][:frames[b]], the pad rows are never read and rows [frames[b], T) of grad_em are 0.
extern "C" __attribute__((visibility("default"))) int gtn_asg_loss_frames_n(const void* emissions, const int* targets,
                                                                            const int* lengths, int B, int T, int N,
                                                                            const void* trans_w, const int* frames,
                                                                            void* loss, void* grad_em,
                                                                            void* grad_trans) {
  if (!frames) {
    g_err = "[gtn_asg_loss_frames_n] null frame counts";
    return -1;
  }
  return asg_loss_impl(emissions, targets, lengths, B, T, N, trans_w, frames, loss, grad_em, grad_trans);
}

// ASG forced alignment.  emissions / targets / lengths / trans_w as for gtn_asg_loss_n; frames: host int32 [B] or null;
// labels: DEVICE int32 [B][T]; tokens: DEVICE int32 [B][T] or null; scores: DEVICE float [B] or null.
// Returns 0, or -1 with the message in gtn_criteria_last_error().
extern "C" __attribute__((visibility("default"))) int gtn_asg_align_n(const void* emissions, const int* targets,
                                                                      const int* lengths, int B, int T, int N,
                                                                      const void* trans_w, const int* frames,
                                                                      void* labels, void* tokens, void* scores) {
  try {
    // (a structure of its own: the loss's cached graph carries gradient state between calls)
    static std::mutex mu;
    static auto* cache = new std::map<int, gtn::Graph>();  // never destroyed: outlives the engine's teardown
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache->find(N);
    if (it == cache->end()) {
      it = cache->emplace(N, gtn::criteria::asgTransitions(N)).first;
      it->second.setCalcGrad(false);
    }
    gtn::Graph& trans = it->second;
    trans.setWeightsDevice(trans_w);  // arc ids are creation order: arcSort permutes lists, not ids
    gtn::criteria::asgAlignBatch(emissions, targets, lengths, B, T, N, trans, frames, labels, tokens, scores);
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

// ASG decode.  emissions: DEVICE [B][T][N]; trans_w: DEVICE [N + N*N] as for gtn_asg_loss_n; frames: host int32 [B] or
// null; labels: DEVICE int32 [B][T]; scores: DEVICE float [B] or null; collapsed: DEVICE int32 [B][T] or null; lengths:
// DEVICE int32 [B] or null (needs collapsed).  Returns 0, or -1 with the message in gtn_criteria_last_error().
extern "C" __attribute__((visibility("default"))) int gtn_asg_decode_n(const void* emissions, int B, int T, int N,
                                                                       const void* trans_w, const int* frames,
                                                                       void* labels, void* scores, void* collapsed,
                                                                       void* lengths) {
  try {
    // (a structure of its own per N, as gtn_asg_align_n keeps: the loss's cached graph carries gradient state)
    static std::mutex mu;
    static auto* cache = new std::map<int, gtn::Graph>();  // never destroyed: outlives the engine's teardown
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache->find(N);
    if (it == cache->end()) {
      it = cache->emplace(N, gtn::criteria::asgTransitions(N)).first;
      it->second.setCalcGrad(false);
    }
    gtn::Graph& trans = it->second;
    trans.setWeightsDevice(trans_w);  // arc ids are creation order: arcSort permutes lists, not ids
    gtn::criteria::asgDecodeBatch(emissions, B, T, N, trans, frames, labels, scores, collapsed, lengths);
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}
