// asg_beam.hip -- ASG prefix beam search with N-best output over a whole padded [n][M][C] batch, results left on the
// device (DESIGN section 27 holds the contract; tests/asg_beam_fp.py is the same recursion in numpy).  The hypotheses
// are the label sequences without equal neighbours, each summed over all of its alignments under emissions o
// transitions: what asg_decode(collapse=True) can emit, and what asg_score scores.
//
// Two launches.
//   rows:    the top-K stream of beam_common.h without an appended blank: (value, label) entries [n][M][topn] and their
//            counts [n][M] in scratch.
//   search:  one workgroup of 256 per utterance, sequential over the frames, in the shape of ctc_beam.hip's search.
//            The list (score, trie node, last label, parent node, length, a 64-bit hash of the prefix and one of the
//            prefix without its last label, and tr[last][last], gathered once when the prefix is created) lives in
//            LDS, twice (read / written).  Per frame:
//              1. S_t from scratch into LDS (the loads of frame t + 1 are issued at the head of frame t)
//              2. the gathers w(i, k) = table(last_i -> label_k) go out (wave v takes beams v, v + 4, ..., its lane k
//                 member k of the set; start[label_k] for the empty prefix); one thread per beam: the stay
//                 (a + tr[l][l]) + x[l] and where its last label sits in S_t; the gathers are parked in LDS before the
//                 barrier
//              3. one thread per beam j: the extension that IS beam j (a beam i of the list spells j's prefix without
//                 its last label -- same length, same hash, then the same node or the same labels along both trie
//                 chains, since a prefix that left the list and came back has a new node) is log-added into j's stay
//                 and struck from beam i's extensions (a bit of an LDS word per beam, LDS atomic-or)
//              4. one 64-bit key per candidate (stays at [0, nb), extensions at nb + i * |S_t| + k): falling score
//                 bits, kind, parent rank, label, set slot -- the contract's total order; a candidate that is dropped
//                 gets the largest key
//              5. a bitonic sort of the keys in LDS, padded with the largest key to a power of two
//              6. thread r < beam makes slot r of the new list from key r; an extension also writes trie node
//                 1 + t * beam + r = (node of its parent, label) and gathers its tr[c][c]
//            At the end thread r < nbest walks the parents of slot r and stores the tokens back to front; all threads
//            fill the rest of the rows with -1.
// Every sum is float32 in the contract's order: (a + w) + x.  A table entry that is not finite drops its candidate.
// With a compiled LM graph (lm_graph.h has the words; tests/asg_beam_graph_fp.py) the search kernel is
// its LM = kLmGraph instantiation: every prefix also carries L and its LM state (slot 0 starts with 0 in the graph's
// start state, a stay copies both, an extension takes L + inc(i, k) and next(i, k)), and candidates rank by acoustic
// score + L; the stays, step 3 and the rows stay acoustic.  The walks of (state_i, label_k) (lm_walk.h, shared with
// ctc_beam.hip) go where step 2's gathers go out, in the same lanes -- the label that is the prefix's last is never
// walked -- and inc(i, k) = lm_weight * walk + lm_bonus and next(i, k) are parked in LDS beside w(i, k).  A key then
// holds the combined total, so step 6 computes an extension's score again, by step 4's expression.
// LM = kLmNone is the code above, statement for statement: everything else sits under `if constexpr (LM != kLmNone)`.
// No global atomics; nothing depends on the order in which waves arrive (keys are distinct, every slot has one writer).
// Every store is a plain C++ store; there is no inline assembly.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "beam_common.h"
#include "kernels.h"
#include "lm_walk.h"
#include "pair_kernels.h"

namespace gtnx {
namespace {

constexpr int kMaxBeam = 64;
constexpr int kMaxSet = 32;  // topn <= 32; no blank
constexpr int kSearchBlock = 256;
constexpr int kKeySlots = 4096;  // stays + one slot per (beam, member of the set) = 2112, padded to a power of two
constexpr int kSearchWaves = kSearchBlock / 64;
constexpr int kGatherTrips = kMaxBeam / kSearchWaves;  // gathers a thread holds at most: one per beam of its wave

template <int LPR>
__global__ __launch_bounds__(kRowBlock) void asg_beam_rows_kernel(AsgBeamArgs a) {
  beam_rows_body<LPR, false>(a);
}

struct Prefixes {
  float a[kMaxBeam];     // the log-sum of the alignments that end in the last label
  float self[kMaxBeam];  // tr[last][last]
  int node[kMaxBeam], last[kMaxBeam], parent[kMaxBeam], len[kMaxBeam];
  unsigned long long hash[kMaxBeam], phash[kMaxBeam];  // of the prefix / of the prefix without its last label
};

// what the graph kernel keeps in LDS on top of the lists: L and the LM state of every prefix in both list copies, and
// inc(i, k) and next(i, k) of the frame at [i * kMaxSet + k], beside wtr
template <int LM>
struct LmLds {
  float L[2][kMaxBeam];
  int st[2][kMaxBeam];
  float inc[kMaxBeam * kMaxSet];
  int nxt[kMaxBeam * kMaxSet];
};
template <>
struct LmLds<kLmNone> {};
static_assert(kGatherTrips == kWalkTrips, "lm_walk.h: a thread holds one walk per prefix of its wave");
// A workgroup may have 64 KB of static LDS.  The large arrays of the graph instantiation -- the two lists, the keys,
// wtr and LmLds -- take 63 488 of them, and the small per-prefix and per-member arrays of the kernel about 1.5 KB
// more: whatever is added to these has to fit the 2 KB that are left.
constexpr size_t kSearchLdsLimit = 64 * 1024, kSearchLdsSmall = 2 * 1024;
static_assert(2 * sizeof(Prefixes) + sizeof(unsigned long long) * kKeySlots + sizeof(float) * kMaxBeam * kMaxSet +
                      sizeof(LmLds<kLmGraph>) + kSearchLdsSmall <= kSearchLdsLimit,
              "asg_beam_search_kernel<kLmGraph>: the static LDS would pass 64 KB");

// (a + w) + x: two sums, each rounded
__device__ __forceinline__ float step_score(float a, float w, float x) {
  const float aw = a + w;
  return aw + x;
}

template <int LM>
__global__ __launch_bounds__(kSearchBlock) void asg_beam_search_kernel(AsgBeamArgs a) {
  __shared__ Prefixes lists[2];
  __shared__ LmLds<LM> lmv;
  __shared__ unsigned long long key[kKeySlots];
  __shared__ float wtr[kMaxBeam * kMaxSet];        // w(i, k) of the frame at [i * kMaxSet + k]
  __shared__ float stay[kMaxBeam];
  __shared__ int lastk[kMaxBeam];                  // where the prefix's last label sits in S_t, or -1
  __shared__ int parnode[kMaxBeam];                // the prefix's parent node, as the list knows it after step 3
  __shared__ unsigned long long struck[kMaxBeam];  // bit k: extension k of the prefix has joined a prefix of the list
  __shared__ float sv[kMaxSet];
  __shared__ int sl[kMaxSet];
  __shared__ int s_cnt, s_nb_new;

  const int b = blockIdx.x, tid = threadIdx.x;
  const int M = a.M, W = a.beam, K = a.topn, C = a.C, nbest = a.nbest;
  int T = a.frames[b];
  T = T < 0 ? 0 : (T > M ? M : T);
  const GTNX_G gtnx_i2* ent = reinterpret_cast<const GTNX_G gtnx_i2*>(a.ent_val) + int64_t(b) * M * K;
  const GTNX_G int* ent_cnt = a.ent_cnt + int64_t(b) * M;
  GTNX_G gtnx_i2* trie = reinterpret_cast<GTNX_G gtnx_i2*>(a.trie) + int64_t(b) * (int64_t(M) * W + 1);
  const GTNX_G float* table = a.table;

  int cur = 0;
  int nb = T > 0 ? 1 : 0;  // (an utterance without frames has no hypothesis)
  if (tid == 0) {
    lists[0].a[0] = 0.0f;
    lists[0].self[0] = NEG_INF;  // (the empty prefix has no stay)
    lists[0].node[0] = 0;
    lists[0].last[0] = -1;
    lists[0].parent[0] = -1;
    lists[0].len[0] = 0;
    lists[0].hash[0] = 0ull;
    lists[0].phash[0] = 0ull;
    if constexpr (LM != kLmNone) {
      lmv.L[0][0] = 0.0f;
      lmv.st[0][0] = a.lmg_start;
    }
  }
  // the token set of the coming frame, one entry per thread, loaded a frame ahead
  gtnx_i2 nxt = entry(NEG_INF, -1);
  int nxt_cnt = 0;
  if (T > 0) {
    nxt_cnt = ent_cnt[0];
    nxt_cnt = nxt_cnt > K ? K : nxt_cnt;  // (the row kernel stores at most topn)
    if (tid < nxt_cnt) nxt = ent[tid];
  }
  for (int t = 0; t < T && nb > 0; ++t) {
    // ---- 1. S_t into LDS; the loads of S_{t+1} go out
    if (tid < kMaxSet) {  // (entries from nxt_cnt on are (-inf, -1) and are never used: only k < cnt is)
      sv[tid] = tid < nxt_cnt ? __int_as_float(nxt.x) : NEG_INF;
      sl[tid] = tid < nxt_cnt ? nxt.y : -1;
    }
    if (tid == 0) {
      s_cnt = nxt_cnt;
      s_nb_new = 0;
    }
    if (tid < kMaxBeam) struck[tid] = 0ull;
    if (t + 1 < T) {
      nxt_cnt = ent_cnt[t + 1];
      nxt_cnt = nxt_cnt > K ? K : nxt_cnt;
      if (tid < nxt_cnt) nxt = ent[int64_t(t + 1) * K + tid];
    }
    __syncthreads();
    const int cnt = s_cnt;
    const Prefixes& B = lists[cur];
    Prefixes& N = lists[cur ^ 1];
    // ---- 2. the gathers of the frame go out: lane k of wave v holds w(i, k) of the prefixes i = v, v + 4, ...  (a label
    // of S_t is below C, a last label too; the slot of the last label itself is the stay's and is not gathered)
    float wq[kGatherTrips];
    [[maybe_unused]] float incr[kGatherTrips];
    [[maybe_unused]] int nxtr[kGatherTrips];
    const int lane = tid & 63, wave = tid >> 6;
    {
      // (every LDS read first and unconditionally, so that they travel together: a slot past the list or the set
      //  holds some int, and its gather is not issued)
      const int cl = sl[lane < kMaxSet ? lane : 0];
      int lastq[kGatherTrips];
#pragma unroll
      for (int q = 0; q < kGatherTrips; ++q) lastq[q] = B.last[wave + q * kSearchWaves];
      const int c = lane < cnt ? cl : -1;
#pragma unroll
      for (int q = 0; q < kGatherTrips; ++q) {
        const int i = wave + q * kSearchWaves;
        wq[q] = 0.0f;
        if (q * kSearchWaves >= nb) continue;  // (the same in every thread: a trip without a prefix)
        if (i < nb && c >= 0) {
          const int l = lastq[q];
          if (c != l) {
            const int64_t at = l < 0 ? int64_t(c) : int64_t(C) + int64_t(c) * C + l;
            wq[q] = table[at];
          }
        }
      }
      if constexpr (LM != kLmNone) {
        // the walks of the frame, in the lanes of the gathers: (state of prefix i, label k), never the prefix's own last
        // label (a sequence with equal neighbours is no hypothesis)
        int stq[kGatherTrips];
        bool act[kGatherTrips];
#pragma unroll
        for (int q = 0; q < kGatherTrips; ++q) stq[q] = lmv.st[cur][wave + q * kSearchWaves];
#pragma unroll
        for (int q = 0; q < kGatherTrips; ++q) act[q] = wave + q * kSearchWaves < nb && c >= 0 && c != lastq[q];
#pragma unroll
        for (int q = 0; q < kGatherTrips; ++q) {
          incr[q] = 0.0f;
          nxtr[q] = 0;
        }
        const int ntrip = (nb + kSearchWaves - 1) / kSearchWaves;
        static_assert(kGatherTrips == 2 * kWalkChunk, "two passes cover every trip");
        lm_walks<0>(a.lmg, 2 * a.lmg_states, c, ntrip, stq, act, incr, nxtr);
        if (ntrip > kWalkChunk) lm_walks<kWalkChunk>(a.lmg, 2 * a.lmg_states, c, ntrip, stq, act, incr, nxtr);
      }
    }
    // the stays
    if (tid < nb) {
      const int l = B.last[tid];
      int lk = -1;
      for (int k = 0; k < cnt; ++k)
        if (sl[k] == l) lk = k;
      const float w = B.self[tid];
      float s = NEG_INF;
      if (lk >= 0 && finite_bits(w)) s = step_score(B.a[tid], w, sv[lk]);
      stay[tid] = s > NEG_INF ? s : NEG_INF;  // (NaN is dropped here)
      lastk[tid] = lk;
    }
    // (slots that are no extension -- past the set, the last label itself -- get 0: finite, and never used)
#pragma unroll
    for (int q = 0; q < kGatherTrips; ++q) {
      const int i = wave + q * kSearchWaves;
      if (q * kSearchWaves >= nb) continue;
      if (i < nb && lane < kMaxSet) wtr[i * kMaxSet + lane] = wq[q];
      if constexpr (LM != kLmNone) {
        // (the term of a slot that was not walked is that of 0: finite, and never used)
        if (i < nb && lane < kMaxSet) {
          lmv.inc[i * kMaxSet + lane] = lm_term(a.lm_weight, incr[q], a.lm_bonus);
          lmv.nxt[i * kMaxSet + lane] = nxtr[q];
        }
      }
    }
    __syncthreads();
    // ---- 3. the extension that is a prefix of the list joins it.  Prefix i is the parent of prefix j when it spells
    // j's labels without the last one.  Its node need not be the one j was created from: a prefix that left the list
    // and came back has a new node, while its child that stayed still points at the old one.  So: same length, same
    // hash (which only spares the comparison), then the same node or the same labels along both chains.
    if (tid < nb) {
      const int par = B.parent[tid], lk = lastk[tid];
      parnode[tid] = par;
      if (par >= 0) {
        int pi = -1;
        const int plen = B.len[tid] - 1;
        const unsigned long long ph = B.phash[tid];
        for (int i = 0; i < nb && pi < 0; ++i)
          if (B.len[i] == plen && B.hash[i] == ph && same_prefix(trie, B.node[i], par)) pi = i;
        if (pi >= 0) parnode[tid] = B.node[pi];  // (from now on the numbers agree: the chains are not walked again)
        if (pi >= 0 && lk >= 0) {
          // (the labels of a prefix have no equal neighbours: last(pi) is not this label, and the slot was gathered)
          const float w = wtr[pi * kMaxSet + lk];
          const float s = step_score(B.a[pi], w, sv[lk]);
          if (finite_bits(w) && s > NEG_INF) {
            stay[tid] = logadd(stay[tid], s);
            atomicOr(&struck[pi], 1ull << lk);
          }
        }
      }
    }
    __syncthreads();
    // ---- 4. the keys, padded with the largest key up to a power of two for the sort
    const int ncand = nb + nb * cnt;
    int npad = 2;
    while (npad < ncand) npad <<= 1;
    for (int idx = tid; idx < npad; idx += kSearchBlock) {
      unsigned long long kk = ~0ull;
      if (idx < nb) {
        const float total = stay[idx];
        if constexpr (LM != kLmNone) {
          if (total > NEG_INF)
            kk = (static_cast<unsigned long long>(falling_bits(total + lmv.L[cur][idx])) << 32) | (uint32_t(idx) << 25);
        } else {
          if (total > NEG_INF) kk = (static_cast<unsigned long long>(falling_bits(total)) << 32) | (uint32_t(idx) << 25);
        }
      } else if (idx < ncand) {
        const int e = idx - nb, i = e / cnt, k = e - i * cnt;
        const int c = sl[k];
        const float w = wtr[i * kMaxSet + k];
        const float s = step_score(B.a[i], w, sv[k]);
        if constexpr (LM != kLmNone) {
          const float inc = lmv.inc[i * kMaxSet + k];
          const float Li = lmv.L[cur][i];
          if (c != B.last[i] && !((struck[i] >> k) & 1ull) && finite_bits(w) && s > NEG_INF && finite_bits(inc))
            kk = (static_cast<unsigned long long>(falling_bits(s + (Li + inc))) << 32) | 0x80000000u |
                 (uint32_t(i) << 25) | (uint32_t(c) << 6) | uint32_t(k);
        } else {
          if (c != B.last[i] && !((struck[i] >> k) & 1ull) && finite_bits(w) && s > NEG_INF)
            kk = (static_cast<unsigned long long>(falling_bits(s)) << 32) | 0x80000000u | (uint32_t(i) << 25) |
                 (uint32_t(c) << 6) | uint32_t(k);  // (C <= 2^19; k < 32)
        }
      }
      key[idx] = kk;
    }
    __syncthreads();
    // ---- 5. a bitonic sort of the padded array, rising: slot r then holds the candidate of place r, and a key says all
    // there is to know about it (total, stay or extension, parent's rank, label)
    for (int k = 2; k <= npad; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < npad; i += kSearchBlock) {
          const int p = i ^ j;
          if (p > i) {
            const unsigned long long x = key[i], y = key[p];
            if ((x > y) == ((i & k) == 0)) {
              key[i] = y;
              key[p] = x;
            }
          }
        }
        __syncthreads();
      }
    // ---- 6. slot r of the new list from the key of place r; an extension also makes trie node 1 + t * beam + r
    if (tid < W && tid < npad) {
      const unsigned long long mine = key[tid];
      if (mine != ~0ull) {
        const int place = tid;
        const uint32_t lo = uint32_t(mine);
        const int i = int((lo >> 25) & 63u);
        if (!(lo & 0x80000000u)) {
          N.a[place] = stay[i];
          N.self[place] = B.self[i];
          N.node[place] = B.node[i];
          N.last[place] = B.last[i];
          N.parent[place] = parnode[i];
          N.len[place] = B.len[i];
          N.hash[place] = B.hash[i];
          N.phash[place] = B.phash[i];
          if constexpr (LM != kLmNone) {
            lmv.L[cur ^ 1][place] = lmv.L[cur][i];
            lmv.st[cur ^ 1][place] = lmv.st[cur][i];
          }
        } else {
          const int c = int((lo >> 6) & 0x7ffffu);
          const int nd = 1 + t * W + place;  // (M * beam < 2^31)
          if constexpr (LM != kLmNone) {
            // the key holds the combined total: the acoustic score again, by step 4's expression (the same bits; +0
            // for -0, as the key's bits give it), and L and the state of the new prefix
            const int k = int(lo & 63u);
            N.a[place] = step_score(B.a[i], wtr[i * kMaxSet + k], sv[k]) + 0.0f;
            lmv.L[cur ^ 1][place] = lmv.L[cur][i] + lmv.inc[i * kMaxSet + k];
            lmv.st[cur ^ 1][place] = lmv.nxt[i * kMaxSet + k];
          } else {
            N.a[place] = from_falling_bits(uint32_t(mine >> 32));  // (the key's bits are the score's)
          }
          N.self[place] = table[int64_t(C) + int64_t(c) * C + c];
          N.node[place] = nd;
          N.last[place] = c;
          N.parent[place] = B.node[i];
          N.len[place] = B.len[i] + 1;
          N.hash[place] = grow_hash(B.hash[i], c);
          N.phash[place] = B.hash[i];
          gtnx_i2 made;
          made.x = B.node[i];
          made.y = c;
          trie[nd] = made;
        }
        atomicMax(&s_nb_new, place + 1);  // (LDS; places are taken from 0 up, the maximum is the count)
      }
    }
    __syncthreads();
    nb = s_nb_new;
    cur ^= 1;
    __syncthreads();  // (s_nb_new is reset at the head of the next frame)
  }
  // ---- the first nbest of the final list
  __syncthreads();  // (the trie nodes of this workgroup's last frames are visible to its own threads)
  const Prefixes& F = lists[cur];
  for (int r = 0; r < nbest; ++r) {
    const int len = r < nb ? F.len[r] : 0;
    GTNX_G int* row = a.tokens + (int64_t(b) * nbest + r) * a.row_stride;
    for (int i = len + tid; i < M; i += kSearchBlock) row[i] = -1;
  }
  if (tid < nbest) {
    const int r = tid;
    GTNX_G int* row = a.tokens + (int64_t(b) * nbest + r) * a.row_stride;
    int len = 0;
    float score = NEG_INF;
    [[maybe_unused]] float am = NEG_INF;
    if (r < nb) {
      len = F.len[r];  // (a prefix grows by at most one label per frame: len <= T <= M)
      score = F.a[r];
      if constexpr (LM != kLmNone) {
        am = score;
        score = am + lmv.L[cur][r];
      }
      int nd = F.node[r], lab = F.last[r], par = F.parent[r];
      for (int k = len - 1; k >= 0 && nd > 0; --k) {
        row[k] = lab;
        nd = par;
        if (nd > 0) {
          const gtnx_i2 e = trie[nd];
          par = e.x;
          lab = e.y;
        }
      }
    }
    a.lengths[int64_t(b) * nbest + r] = len;
    a.scores[int64_t(b) * nbest + r] = score;
    if constexpr (LM != kLmNone)
      if (a.am_scores) a.am_scores[int64_t(b) * nbest + r] = am;
  }
}

template <int LPR>
void launch_rows(const AsgBeamArgs& a, hipStream_t st) {
  for_row_slices(a, LPR, a.topn, [&](const AsgBeamArgs& s, dim3 grid) {
    hipLaunchKernelGGL(asg_beam_rows_kernel<LPR>, grid, dim3(kRowBlock), 0, st, s);
  });
}

}  // namespace

void launch_asg_beam(const AsgBeamArgs& a, int which, hipStream_t st) {
  if (a.n <= 0) return;
  if (which == 0) {
    if (a.M <= 0) return;
    // lanes per row: every lane of a group gets at least one 16-byte load where the row has that many
    if (a.C <= 32) launch_rows<8>(a, st);
    else if (a.C <= 64) launch_rows<16>(a, st);
    else if (a.C <= 128) launch_rows<32>(a, st);
    else launch_rows<64>(a, st);
    return;
  }
  if (a.lmg)
    hipLaunchKernelGGL(asg_beam_search_kernel<kLmGraph>, dim3(static_cast<unsigned>(a.n)), dim3(kSearchBlock), 0, st, a);
  else
    hipLaunchKernelGGL(asg_beam_search_kernel<kLmNone>, dim3(static_cast<unsigned>(a.n)), dim3(kSearchBlock), 0, st, a);
}

}  // namespace gtnx
