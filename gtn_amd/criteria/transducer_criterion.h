// transducer_criterion.h -- the transducer (RNN-T) criterion over joint logits that live on the device, written against
// the drop-in C++ API of include/gtn: one call for the scores, one for the gradient, results left on the device.
// Header-only; used by gtn_amd/criteria/criteria_capi.cpp (torch_loss.transducer_score / transducer_loss).
#pragma once

#include <stdexcept>

#include "gtn/gtn.h"

namespace gtn {
namespace criteria {

/** The transducer log scores of B utterances: `logitsDev` device float32 [B][T][U + 1][C], read in place; `targetsDev`
 *  device int32 [B][U]; `framesDev` / `targetLengthsDev` device int32 [B]; `scoresDev` device float32 [B]; `rowsDev`
 *  device float32 [B][T][U + 1][3] or null (the compact plane, kept for the gradient call).
 *  gtnx_batch_transducer_score has the contract.  Nothing is copied back. */
inline void transducerScoreBatch(
    const void* logitsDev,
    const void* targetsDev,
    const void* framesDev,
    const void* targetLengthsDev,
    int B,
    int T,
    int U,
    int C,
    int blank,
    bool normalize,
    void* scoresDev,
    void* rowsDev = nullptr) {
  if (!scoresDev) {
    throw std::invalid_argument("transducerScoreBatch: null scores");
  }
  batched::transducerScore(static_cast<const float*>(logitsDev), static_cast<const int*>(targetsDev),
                           static_cast<const int*>(framesDev), static_cast<const int*>(targetLengthsDev), B, T, U, C,
                           blank, normalize, static_cast<float*>(scoresDev), static_cast<float*>(rowsDev));
}

/** Their gradient under `weightsDev` (device float32 [B]): `gradDev` device float32 [B][T][U + 1][C], every row written;
 *  `rowsDev` the plane transducerScoreBatch left for the same inputs, or null (then it is recomputed). */
inline void transducerScoreGradBatch(
    const void* logitsDev,
    const void* targetsDev,
    const void* framesDev,
    const void* targetLengthsDev,
    int B,
    int T,
    int U,
    int C,
    int blank,
    bool normalize,
    const void* weightsDev,
    void* gradDev,
    const void* rowsDev = nullptr) {
  if (!weightsDev || !gradDev) {
    throw std::invalid_argument("transducerScoreGradBatch: null weights or gradient");
  }
  batched::transducerScoreGrad(static_cast<const float*>(logitsDev), static_cast<const int*>(targetsDev),
                               static_cast<const int*>(framesDev), static_cast<const int*>(targetLengthsDev), B, T, U, C,
                               blank, normalize, static_cast<const float*>(weightsDev), static_cast<float*>(gradDev),
                               static_cast<const float*>(rowsDev));
}

/** The token-and-duration transducer (TDT) log scores: `logitsDev` device float32 [B][T][U + 1][C + D] (C token logits,
 *  then D duration logits); `rowsDev` device float32 [B][T][U + 1][D + 4] or null; the rest as transducerScoreBatch.
 *  gtnx_batch_transducer_tdt_score has the contract.  Nothing is copied back. */
inline void transducerTdtScoreBatch(
    const void* logitsDev,
    const void* targetsDev,
    const void* framesDev,
    const void* targetLengthsDev,
    int B,
    int T,
    int U,
    int C,
    int D,
    int blank,
    float sigma,
    void* scoresDev,
    void* rowsDev = nullptr) {
  if (!scoresDev) {
    throw std::invalid_argument("transducerTdtScoreBatch: null scores");
  }
  batched::transducerTdtScore(static_cast<const float*>(logitsDev), static_cast<const int*>(targetsDev),
                              static_cast<const int*>(framesDev), static_cast<const int*>(targetLengthsDev), B, T, U, C,
                              D, blank, sigma, static_cast<float*>(scoresDev), static_cast<float*>(rowsDev));
}

/** Their gradient under `weightsDev` (device float32 [B]): `gradDev` device float32 [B][T][U + 1][C + D], every row
 *  written; `rowsDev` the plane transducerTdtScoreBatch left for the same inputs, or null (then it is recomputed). */
inline void transducerTdtScoreGradBatch(
    const void* logitsDev,
    const void* targetsDev,
    const void* framesDev,
    const void* targetLengthsDev,
    int B,
    int T,
    int U,
    int C,
    int D,
    int blank,
    float sigma,
    const void* weightsDev,
    void* gradDev,
    const void* rowsDev = nullptr) {
  if (!weightsDev || !gradDev) {
    throw std::invalid_argument("transducerTdtScoreGradBatch: null weights or gradient");
  }
  batched::transducerTdtScoreGrad(static_cast<const float*>(logitsDev), static_cast<const int*>(targetsDev),
                                  static_cast<const int*>(framesDev), static_cast<const int*>(targetLengthsDev), B, T, U,
                                  C, D, blank, sigma, static_cast<const float*>(weightsDev),
                                  static_cast<float*>(gradDev), static_cast<const float*>(rowsDev));
}

/** The same scores under an additive joint: `amDev` device float32 [B][T][C] and `lmDev` device float32 [B][U + 1][C]
 *  stand for the logits amDev[b][t][c] + lmDev[b][u][c], which are never formed; always normalised.
 *  gtnx_batch_transducer_add_score has the contract and the float32 domain.  Nothing is copied back. */
inline void transducerAddScoreBatch(
    const void* amDev,
    const void* lmDev,
    const void* targetsDev,
    const void* framesDev,
    const void* targetLengthsDev,
    int B,
    int T,
    int U,
    int C,
    int blank,
    void* scoresDev,
    void* rowsDev = nullptr) {
  if (!scoresDev) {
    throw std::invalid_argument("transducerAddScoreBatch: null scores");
  }
  batched::transducerAddScore(static_cast<const float*>(amDev), static_cast<const float*>(lmDev),
                              static_cast<const int*>(targetsDev), static_cast<const int*>(framesDev),
                              static_cast<const int*>(targetLengthsDev), B, T, U, C, blank,
                              static_cast<float*>(scoresDev), static_cast<float*>(rowsDev));
}

/** Their gradients under `weightsDev` (device float32 [B]): `gradAmDev` device float32 [B][T][C] and `gradLmDev` device
 *  float32 [B][U + 1][C], every element written; `rowsDev` the plane transducerAddScoreBatch left, or null. */
inline void transducerAddScoreGradBatch(
    const void* amDev,
    const void* lmDev,
    const void* targetsDev,
    const void* framesDev,
    const void* targetLengthsDev,
    int B,
    int T,
    int U,
    int C,
    int blank,
    const void* weightsDev,
    void* gradAmDev,
    void* gradLmDev,
    const void* rowsDev = nullptr) {
  if (!weightsDev || !gradAmDev || !gradLmDev) {
    throw std::invalid_argument("transducerAddScoreGradBatch: null weights or gradient");
  }
  batched::transducerAddScoreGrad(static_cast<const float*>(amDev), static_cast<const float*>(lmDev),
                                  static_cast<const int*>(targetsDev), static_cast<const int*>(framesDev),
                                  static_cast<const int*>(targetLengthsDev), B, T, U, C, blank,
                                  static_cast<const float*>(weightsDev), static_cast<float*>(gradAmDev),
                                  static_cast<float*>(gradLmDev), static_cast<const float*>(rowsDev));
}

/** The pruned (banded) transducer scores: `logitsDev` device float32 [B][T][S][C], the joiner's output on the S lattice
 *  columns rangesDev[b][t] .. + S - 1 of every frame (`rangesDev` device int32 [B][T]); the rest as
 *  transducerScoreBatch, `rowsDev` device float32 [B][T][S][3] or null.  gtnx_batch_transducer_pruned_score has the
 *  contract.  Nothing is copied back. */
inline void transducerPrunedScoreBatch(
    const void* logitsDev,
    const void* rangesDev,
    const void* targetsDev,
    const void* framesDev,
    const void* targetLengthsDev,
    int B,
    int T,
    int S,
    int U,
    int C,
    int blank,
    bool normalize,
    void* scoresDev,
    void* rowsDev = nullptr) {
  if (!scoresDev) {
    throw std::invalid_argument("transducerPrunedScoreBatch: null scores");
  }
  batched::transducerPrunedScore(static_cast<const float*>(logitsDev), static_cast<const int*>(rangesDev),
                                 static_cast<const int*>(targetsDev), static_cast<const int*>(framesDev),
                                 static_cast<const int*>(targetLengthsDev), B, T, S, U, C, blank, normalize,
                                 static_cast<float*>(scoresDev), static_cast<float*>(rowsDev));
}

/** Their gradient under `weightsDev` (device float32 [B]): `gradDev` device float32 [B][T][S][C], every row written;
 *  `rowsDev` the plane transducerPrunedScoreBatch left for the same inputs, or null. */
inline void transducerPrunedScoreGradBatch(
    const void* logitsDev,
    const void* rangesDev,
    const void* targetsDev,
    const void* framesDev,
    const void* targetLengthsDev,
    int B,
    int T,
    int S,
    int U,
    int C,
    int blank,
    bool normalize,
    const void* weightsDev,
    void* gradDev,
    const void* rowsDev = nullptr) {
  if (!weightsDev || !gradDev) {
    throw std::invalid_argument("transducerPrunedScoreGradBatch: null weights or gradient");
  }
  batched::transducerPrunedScoreGrad(static_cast<const float*>(logitsDev), static_cast<const int*>(rangesDev),
                                     static_cast<const int*>(targetsDev), static_cast<const int*>(framesDev),
                                     static_cast<const int*>(targetLengthsDev), B, T, S, U, C, blank, normalize,
                                     static_cast<const float*>(weightsDev), static_cast<float*>(gradDev),
                                     static_cast<const float*>(rowsDev));
}

/** transducerScoreBatch over bfloat16 / float16 logits: `logitsDev` holds 2-byte elements of `dtype` (GTNX_DTYPE_F16 /
 *  GTNX_DTYPE_BF16), read in place; scores and the rows plane stay float32.  gtnx_batch_transducer_score16 has the
 *  contract. */
inline void transducerScoreBatch16(
    const void* logitsDev,
    int dtype,
    const void* targetsDev,
    const void* framesDev,
    const void* targetLengthsDev,
    int B,
    int T,
    int U,
    int C,
    int blank,
    bool normalize,
    void* scoresDev,
    void* rowsDev = nullptr) {
  if (!scoresDev) {
    throw std::invalid_argument("transducerScoreBatch16: null scores");
  }
  batched::transducerScore16(logitsDev, dtype, static_cast<const int*>(targetsDev), static_cast<const int*>(framesDev),
                             static_cast<const int*>(targetLengthsDev), B, T, U, C, blank, normalize,
                             static_cast<float*>(scoresDev), static_cast<float*>(rowsDev));
}

/** Their gradient under `weightsDev` (device float32 [B]): `gradDev` device [B][T][U + 1][C] of the logits' dtype, every
 *  row written; `rowsDev` the plane transducerScoreBatch16 left for the same inputs, or null. */
inline void transducerScoreGradBatch16(
    const void* logitsDev,
    int dtype,
    const void* targetsDev,
    const void* framesDev,
    const void* targetLengthsDev,
    int B,
    int T,
    int U,
    int C,
    int blank,
    bool normalize,
    const void* weightsDev,
    void* gradDev,
    const void* rowsDev = nullptr) {
  if (!weightsDev || !gradDev) {
    throw std::invalid_argument("transducerScoreGradBatch16: null weights or gradient");
  }
  batched::transducerScoreGrad16(logitsDev, dtype, static_cast<const int*>(targetsDev),
                                 static_cast<const int*>(framesDev), static_cast<const int*>(targetLengthsDev), B, T, U,
                                 C, blank, normalize, static_cast<const float*>(weightsDev), gradDev,
                                 static_cast<const float*>(rowsDev));
}

/** transducerPrunedScoreBatch over bfloat16 / float16 logits [B][T][S][C] of `dtype`; the rest as
 *  transducerScoreBatch16.  gtnx_batch_transducer_pruned_score16 has the contract. */
inline void transducerPrunedScoreBatch16(
    const void* logitsDev,
    int dtype,
    const void* rangesDev,
    const void* targetsDev,
    const void* framesDev,
    const void* targetLengthsDev,
    int B,
    int T,
    int S,
    int U,
    int C,
    int blank,
    bool normalize,
    void* scoresDev,
    void* rowsDev = nullptr) {
  if (!scoresDev) {
    throw std::invalid_argument("transducerPrunedScoreBatch16: null scores");
  }
  batched::transducerPrunedScore16(logitsDev, dtype, static_cast<const int*>(rangesDev),
                                   static_cast<const int*>(targetsDev), static_cast<const int*>(framesDev),
                                   static_cast<const int*>(targetLengthsDev), B, T, S, U, C, blank, normalize,
                                   static_cast<float*>(scoresDev), static_cast<float*>(rowsDev));
}

/** Their gradient under `weightsDev`: `gradDev` device [B][T][S][C] of the logits' dtype, every row written. */
inline void transducerPrunedScoreGradBatch16(
    const void* logitsDev,
    int dtype,
    const void* rangesDev,
    const void* targetsDev,
    const void* framesDev,
    const void* targetLengthsDev,
    int B,
    int T,
    int S,
    int U,
    int C,
    int blank,
    bool normalize,
    const void* weightsDev,
    void* gradDev,
    const void* rowsDev = nullptr) {
  if (!weightsDev || !gradDev) {
    throw std::invalid_argument("transducerPrunedScoreGradBatch16: null weights or gradient");
  }
  batched::transducerPrunedScoreGrad16(logitsDev, dtype, static_cast<const int*>(rangesDev),
                                       static_cast<const int*>(targetsDev), static_cast<const int*>(framesDev),
                                       static_cast<const int*>(targetLengthsDev), B, T, S, U, C, blank, normalize,
                                       static_cast<const float*>(weightsDev), gradDev,
                                       static_cast<const float*>(rowsDev));
}

/** The node occupancies `occDev` (device float32 [B][T][U + 1]) of the full lattice whose compact plane `rowsDev`
 *  (device float32 [B][T][U + 1][3]) transducerScoreBatch or transducerAddScoreBatch left. */
inline void transducerOccupancyBatch(
    const void* rowsDev,
    const void* framesDev,
    const void* targetLengthsDev,
    int B,
    int T,
    int U,
    void* occDev) {
  batched::transducerOccupancy(static_cast<const float*>(rowsDev), static_cast<const int*>(framesDev),
                               static_cast<const int*>(targetLengthsDev), B, T, U, static_cast<float*>(occDev));
}

/** The best alignment of every transcript on its lattice (gtnx_batch_transducer_align has the contract): the inputs of
 *  transducerScoreBatch, or of transducerScoreBatch16 with `dtype` GTNX_DTYPE_F16 / GTNX_DTYPE_BF16 (0: float32);
 *  `scoresDev` device float32 [B], `tokenFramesDev` device int32 [B][U], `tokenScoresDev` device float32 [B][U] or null,
 *  `frameTokensDev` device int32 [B][T] or null, `rowsDev` the plane a score call left for the same inputs, or null.
 *  `logitsDev` null: the alignment from `rowsDev` alone (gtnx_batch_transducer_align_rows).  Nothing is copied back. */
inline void transducerAlignBatch(
    const void* logitsDev,
    int dtype,
    const void* targetsDev,
    const void* framesDev,
    const void* targetLengthsDev,
    int B,
    int T,
    int U,
    int C,
    int blank,
    bool normalize,
    const void* rowsDev,
    void* scoresDev,
    void* tokenFramesDev,
    void* tokenScoresDev = nullptr,
    void* frameTokensDev = nullptr) {
  if (!scoresDev) {
    throw std::invalid_argument("transducerAlignBatch: null scores");
  }
  const int* tg = static_cast<const int*>(targetsDev);
  const int* fr = static_cast<const int*>(framesDev);
  const int* tl = static_cast<const int*>(targetLengthsDev);
  const float* rows = static_cast<const float*>(rowsDev);
  float* sc = static_cast<float*>(scoresDev);
  int* tf = static_cast<int*>(tokenFramesDev);
  float* ts = static_cast<float*>(tokenScoresDev);
  int* ft = static_cast<int*>(frameTokensDev);
  if (!logitsDev) {
    batched::transducerAlignRows(rows, fr, tl, B, T, U, sc, tf, ts, ft);
  } else if (dtype == 0) {
    batched::transducerAlign(static_cast<const float*>(logitsDev), tg, fr, tl, B, T, U, C, blank, normalize, sc, tf, ts,
                             ft, rows);
  } else {
    batched::transducerAlign16(logitsDev, dtype, tg, fr, tl, B, T, U, C, blank, normalize, sc, tf, ts, ft, rows);
  }
}

} // namespace criteria
} // namespace gtn
