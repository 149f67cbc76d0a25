// edit_distance.h -- the Levenshtein distance of examples/edit_distance.cpp (-viterbiScore(compose(x, compose(edits,
// y)))) for a batch of token rows that live on the device, written against the drop-in C++ API of include/gtn: one
// call, results left on the device.  Header-only; used by gtn_amd/criteria/criteria_capi.cpp (torch_loss.edit_distance).
#pragma once

#include <cstdint>

#include "gtn/gtn.h"

namespace gtn {
namespace criteria {

/** Edit distance of all B * N pairs (hyp[b, k], ref[b]), unit costs, tokens compared with == only.  `hypDev`: device
 *  int32 [B][N][L] (dense rows); `hypLengthsDev`: device int32 [B][N]; `refDev`: device int32 [B][U]; `refLengthsDev`:
 *  device int32 [B] -- lengths are clamped to the widths on the device and nothing at or past a length is read, so
 *  the outputs of ctcDecodeBatch / ctcBeamDecodeBatch go in as they are.  `distDev`: device int32 [B][N]; `opsDev`:
 *  device int32 [B][N][3] = (substitutions, deletions, insertions) or null (gtnx_batch_edit_distance has the
 *  contract).  One launch without ops; nothing is copied back. */
inline void editDistanceBatch(
    const void* hypDev,
    const void* hypLengthsDev,
    const void* refDev,
    const void* refLengthsDev,
    int B,
    int N,
    int L,
    int U,
    void* distDev,
    void* opsDev = nullptr) {
  batched::editDistance(static_cast<const int*>(hypDev), L, static_cast<const int*>(hypLengthsDev),
                        static_cast<const int*>(refDev), U, static_cast<const int*>(refLengthsDev), B, N, L, U,
                        static_cast<int*>(distDev), static_cast<int*>(opsDev));
}

} // namespace criteria
} // namespace gtn
