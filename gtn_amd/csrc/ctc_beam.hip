// ctc_beam.hip -- CTC prefix beam search with N-best output over a whole padded [n][M][C] batch, results left on the
// device (DESIGN section 20 holds the contract; tests/ctc_beam_fp.py is the same recursion in numpy).
//
// Two launches.
//   rows:    beam_common.h's body with the blank appended (asg_beam.hip runs the same body without one): the stream of
//            linear_decode.hip (a group of LPR lanes owns one row: scalar head up to the next 16-byte
//            boundary, 16-byte loads, scalar tail; grid = (blocks of frames, utterance); rows from frames[b] on are
//            never addressed) with a top-K selection on it.  Round r takes the first entry, in the order (value
//            descending, label ascending), that comes after the entry of round r - 1: per lane `v > m` in rising label
//            order among the entries still allowed, across lanes the larger value and of equal values the smaller
//            label.  NaN fails every comparison and -inf never exceeds the start value, so neither is chosen; a round
//            that finds nothing ends the row.  The row is read again in every round (from the vector L1 after the
//            first), which keeps any number of labels in one code path.  Then `blank` is appended if no round took it
//            and its entry is above -inf.  Lane 0 of the group stores one 8-byte (value, label) entry per round and the
//            count.
//   search:  one workgroup of 256 per utterance, sequential over the frames.  The list (pb, pnb, trie node, last label,
//            parent node, length, a 64-bit hash of the prefix and one of the prefix without its last label) lives in
//            LDS, twice (read / written).  Per frame:
//              1. S_t from scratch into LDS (the loads of frame t + 1 are issued at the head of frame t)
//              2. one thread per beam: tot, the stay scores, where its last label sits in S_t
//              3. one thread per beam j: the extension that IS beam j (a beam i of the list spells j's prefix without
//                 its last label -- same length, same hash, then the same node or the same labels along both trie
//                 chains, since a prefix that left the list and came back has a new node -- and label(node_j) is in
//                 S_t) is added into pnb'_j and struck from beam i's extensions (a bit of an LDS word per beam, LDS
//                 atomic-or: the bits are independent)
//              4. one 64-bit key per candidate (stays at [0, nb), extensions at nb + i * |S_t| + k): total descending,
//                 then stay before extension, parent rank, label -- the contract's total order; a candidate that is
//                 dropped gets the largest key
//              5. a bitonic sort of the keys in LDS, padded with the largest key to a power of two: slot r then holds
//                 the candidate of place r, and a key says all there is to know about it
//              6. thread r < beam makes slot r of the new list from key r; an extension also writes trie node
//                 1 + t * beam + r = (node of its parent, label)
//            At the end thread r < nbest walks the parents of slot r and stores the tokens back to front; all threads
//            fill the rest of the rows with -1.
// With a bigram table (tests/ctc_beam_lm_fp.py) the search kernel is its LM = kLmTable instantiation:
// every beam also carries L, the table's score of its prefix, candidates rank by acoustic total + L, and pb / pnb stay
// acoustic.  The gathers inc(i, k) = lm_weight * w(last_i -> label_k) + lm_bonus go out after step 1, when S_t and the
// last labels are known (wave v takes beams v, v + 4, ..., its lane k member k of the set), fly during step 2 and are
// parked in LDS before its barrier; step 4 reads them from there.  A key then holds the combined total, so step 6
// computes an extension's score again, by step 4's expression; for that the key keeps the member's place in the set in
// its lowest 6 bits, below a label of 19 bits (the engine refuses more labels with a table: it would not fit a device).
// LM = kLmNone is the code above, statement for statement: everything else sits under `if constexpr (LM != kLmNone)`.
// With a compiled LM graph (lm_graph.h has the words; tests/ctc_beam_graph_fp.py) it is the third
// instantiation, LM = kLmGraph: everything the table has, and every beam also carries its LM state (slot 0 starts at the
// graph's start state, a stay copies it, an extension takes next(i, k)).  Where the table is gathered the thread walks
// (state_i, label_k) instead (lm_walk.h, shared with asg_beam.hip) -- all its walks together, one probe of each per
// round, so that the dependent loads of up to 8 walks overlap -- and parks next(i, k) beside inc(i, k).  Every loop of
// the walk has a compile-time bound, and a walk that exhausts one forbids its extension.
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
constexpr int kMaxSet = 33;     // topn <= 32, plus the blank
constexpr int kSearchBlock = 256;
constexpr int kMaxCand = kMaxBeam + kMaxBeam * kMaxSet;  // stays + one slot per (beam, member of the set)
constexpr int kKeySlots = 4096;                          // the next power of two: the sort pads up to one

// the rows: the shared top-K stream with the blank appended (beam_common.h)
template <int LPR>
__global__ __launch_bounds__(kRowBlock) void ctc_beam_rows_kernel(CtcBeamArgs a) {
  beam_rows_body<LPR, true>(a);
}

struct Beams {
  float pb[kMaxBeam], pnb[kMaxBeam];
  int node[kMaxBeam], last[kMaxBeam], parent[kMaxBeam], len[kMaxBeam];
  unsigned long long hash[kMaxBeam], phash[kMaxBeam];  // of the prefix / of the prefix without its last label
};

// what the LM kernels keep in LDS on top of the lists: L of every beam in both list copies, and inc(i, k) of the
// frame at [i * kMaxSet + k]; with a graph also the LM state of every beam and next(i, k)
template <int LM>
struct LmLds {
  float L[2][kMaxBeam];
  float inc[kMaxBeam * kMaxSet];
};
template <>
struct LmLds<kLmNone> {};
template <>
struct LmLds<kLmGraph> {
  float L[2][kMaxBeam];
  float inc[kMaxBeam * kMaxSet];
  int st[2][kMaxBeam];
  int nxt[kMaxBeam * kMaxSet];
};
constexpr int kSearchWaves = kSearchBlock / 64;
constexpr int kIncTrips = kMaxBeam / kSearchWaves;  // gathers a thread holds at most: one per beam of its wave

static_assert(kIncTrips == kWalkTrips, "lm_walk.h: a thread holds one walk per beam of its wave");

template <int LM>
__global__ __launch_bounds__(kSearchBlock) void ctc_beam_search_kernel(CtcBeamArgs a) {
  __shared__ Beams beams[2];
  __shared__ LmLds<LM> lmv;
  __shared__ unsigned long long key[kKeySlots];
  __shared__ float tot[kMaxBeam], spb[kMaxBeam], spnb[kMaxBeam];
  __shared__ int lastk[kMaxBeam];                  // where the beam's last label sits in S_t, or -1
  __shared__ int parnode[kMaxBeam];                // the beam's parent node, as the list knows it after step 3
  __shared__ unsigned long long struck[kMaxBeam];  // bit k: extension k of the beam has joined a beam of the list
  __shared__ float sv[kMaxSet];
  __shared__ int sl[kMaxSet];
  __shared__ int s_cnt, s_blank_k, s_nb_new;

  const int b = blockIdx.x, tid = threadIdx.x;
  const int M = a.M, W = a.beam, K1 = a.topn + 1, blank = a.blank, nbest = a.nbest;
  int T = a.frames[b];
  T = T < 0 ? 0 : (T > M ? M : T);
  const GTNX_G gtnx_i2* ent = reinterpret_cast<const GTNX_G gtnx_i2*>(a.ent_val) + int64_t(b) * M * K1;
  const GTNX_G int* ent_cnt = a.ent_cnt + int64_t(b) * M;
  GTNX_G gtnx_i2* trie = reinterpret_cast<GTNX_G gtnx_i2*>(a.trie) + int64_t(b) * (int64_t(M) * W + 1);

  int cur = 0;
  int nb = T > 0 ? 1 : 0;  // (an utterance without frames has no hypothesis)
  if (tid == 0) {
    beams[0].pb[0] = 0.0f;
    beams[0].pnb[0] = NEG_INF;
    beams[0].node[0] = 0;
    beams[0].last[0] = -1;
    beams[0].parent[0] = -1;
    beams[0].len[0] = 0;
    beams[0].hash[0] = 0ull;
    beams[0].phash[0] = 0ull;
    if constexpr (LM != kLmNone) lmv.L[0][0] = 0.0f;
    if constexpr (LM == kLmGraph) lmv.st[0][0] = a.lmg_start;
  }
  // the token set of the coming frame, one entry per thread, loaded a frame ahead
  gtnx_i2 nxt = entry(NEG_INF, -1);
  int nxt_cnt = 0;
  if (T > 0) {
    nxt_cnt = ent_cnt[0];
    nxt_cnt = nxt_cnt > K1 ? K1 : nxt_cnt;  // (the row kernel stores at most topn + 1)
    if (tid < nxt_cnt) nxt = ent[tid];
  }
  for (int t = 0; t < T && nb > 0; ++t) {
    // ---- 1. S_t into LDS; the loads of S_{t+1} go out
    if (tid < kMaxSet) {  // (entries from nxt_cnt on are (-inf, -1) and are never read: only k < cnt is)
      sv[tid] = tid < nxt_cnt ? __int_as_float(nxt.x) : NEG_INF;
      sl[tid] = tid < nxt_cnt ? nxt.y : -1;
    }
    if (tid == 0) {
      s_cnt = nxt_cnt;
      s_blank_k = -1;
      s_nb_new = 0;
    }
    if (tid < kMaxBeam) struck[tid] = 0ull;
    __syncthreads();
    const int cnt = s_cnt;
    if (tid < cnt && sl[tid] == blank) s_blank_k = tid;  // (labels of a set are distinct: one writer)
    if (t + 1 < T) {
      nxt_cnt = ent_cnt[t + 1];
      nxt_cnt = nxt_cnt > K1 ? K1 : nxt_cnt;
      if (tid < nxt_cnt) nxt = ent[int64_t(t + 1) * K1 + tid];
    }
    __syncthreads();
    const Beams& B = beams[cur];
    Beams& N = beams[cur ^ 1];
    const int bk = s_blank_k;
    // the gathers of the frame go out: lane k of wave v holds inc(i, k) of the beams i = v, v + 4, ...  (the blank is
    // no extension: its row and column are never read; a label of S_t is below C, a last label too)
    [[maybe_unused]] float incr[kIncTrips];
    [[maybe_unused]] int nxtr[kIncTrips];
    if constexpr (LM == kLmGraph) {
      // the walks of the frame, where the table's gathers are: the same lanes serve the same (beam, member)
      const int lane = tid & 63, wave = tid >> 6;
      const int cl = sl[lane < kMaxSet ? lane : 0];
      int stq[kIncTrips];
      bool act[kIncTrips];
#pragma unroll
      for (int q = 0; q < kIncTrips; ++q) stq[q] = lmv.st[cur][wave + q * kSearchWaves];
      const int c = (lane < cnt && lane != bk) ? cl : -1;
#pragma unroll
      for (int q = 0; q < kIncTrips; ++q) act[q] = wave + q * kSearchWaves < nb && c >= 0;
#pragma unroll
      for (int q = 0; q < kIncTrips; ++q) {
        incr[q] = 0.0f;
        nxtr[q] = 0;
      }
      const int ntrip = (nb + kSearchWaves - 1) / kSearchWaves;
      static_assert(kIncTrips == 2 * kWalkChunk, "two passes cover every trip");
      lm_walks<0>(a.lmg, 2 * a.lmg_states, c, ntrip, stq, act, incr, nxtr);
      if (ntrip > kWalkChunk) lm_walks<kWalkChunk>(a.lmg, 2 * a.lmg_states, c, ntrip, stq, act, incr, nxtr);
    }
    if constexpr (LM == kLmTable) {
      // (every LDS read first and unconditionally, so that they travel together: a slot past the list or the set
      //  holds some int, and its gather is not issued)
      const int lane = tid & 63, wave = tid >> 6;
      const int cl = sl[lane < kMaxSet ? lane : 0];
      int lastq[kIncTrips];
#pragma unroll
      for (int q = 0; q < kIncTrips; ++q) lastq[q] = B.last[wave + q * kSearchWaves];
      const int c = (lane < cnt && lane != bk) ? cl : -1;
#pragma unroll
      for (int q = 0; q < kIncTrips; ++q) {
        const int i = wave + q * kSearchWaves;
        incr[q] = 0.0f;
        if (q * kSearchWaves >= nb) continue;  // (the same in every thread: a trip without a beam)
        if (i < nb && c >= 0) {
          const int l = lastq[q];
          const int64_t at = l < 0 ? int64_t(c) : int64_t(a.C) + int64_t(c) * a.C + l;
          incr[q] = a.lm[at];
        }
      }
    }
    // ---- 2. the stays
    if (tid < nb) {
      const float pb = B.pb[tid], pnb = B.pnb[tid];
      const float tt = logadd(pb, pnb);
      const int l = B.last[tid];
      int lk = -1;
      for (int k = 0; k < cnt; ++k)
        if (sl[k] == l) lk = k;
      tot[tid] = tt;
      spb[tid] = bk >= 0 ? tt + sv[bk] : NEG_INF;
      spnb[tid] = (lk >= 0 && pnb > NEG_INF) ? pnb + sv[lk] : NEG_INF;
      lastk[tid] = lk;
    }
    if constexpr (LM != kLmNone) {
      // (slots that are no extension -- past the set, the blank -- get the term of 0: finite, and never used)
      const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
      for (int q = 0; q < kIncTrips; ++q) {
        const int i = wave + q * kSearchWaves;
        if (q * kSearchWaves >= nb) continue;
        if (i < nb && lane < kMaxSet) lmv.inc[i * kMaxSet + lane] = lm_term(a.lm_weight, incr[q], a.lm_bonus);
        if constexpr (LM == kLmGraph)
          if (i < nb && lane < kMaxSet) lmv.nxt[i * kMaxSet + lane] = nxtr[q];
      }
    }
    __syncthreads();
    // ---- 3. the extension that is a beam of the list joins it.  Beam i is the parent of beam j when it spells
    // j's prefix without its last label.  Its node need not be the one j was created from: a prefix that left the
    // list and came back has a new node, while its child that stayed still points at the old one.  So: same length,
    // same hash (which only spares the comparison), then the same node or the same labels along both chains.
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
          const float base = B.last[pi] == B.last[tid] ? B.pb[pi] : tot[pi];
          if (base > NEG_INF) {
            spnb[tid] = logadd(spnb[tid], base + sv[lk]);
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
        const float total = logadd(spb[idx], spnb[idx]);
        if constexpr (LM != kLmNone) {
          if (total > NEG_INF)
            kk = (static_cast<unsigned long long>(falling_bits(total + lmv.L[cur][idx])) << 32) | (uint32_t(idx) << 25);
        } else {
          if (total > NEG_INF) kk = (static_cast<unsigned long long>(falling_bits(total)) << 32) | (uint32_t(idx) << 25);
        }
      } else if (idx < ncand) {
        const int e = idx - nb, i = e / cnt, k = e - i * cnt;
        const int c = sl[k];
        const float base = c == B.last[i] ? B.pb[i] : tot[i];
        const float s = base + sv[k];
        if constexpr (LM != kLmNone) {
          const float inc = lmv.inc[i * kMaxSet + k];  // (the blank's slot is finite, and the test on k drops it)
          const float Li = lmv.L[cur][i];
          if (k != bk && !((struck[i] >> k) & 1ull) && base > NEG_INF && s > NEG_INF && finite_bits(inc))
            kk = (static_cast<unsigned long long>(falling_bits(s + (Li + inc))) << 32) | 0x80000000u |
                 (uint32_t(i) << 25) | (uint32_t(c) << 6) | uint32_t(k);  // (C <= 2^19 with a table; k <= 32)
        } else {
          if (k != bk && !((struck[i] >> k) & 1ull) && base > NEG_INF && s > NEG_INF)
            kk = (static_cast<unsigned long long>(falling_bits(s)) << 32) | 0x80000000u | (uint32_t(i) << 25) |
                 uint32_t(c);
        }
      }
      key[idx] = kk;
    }
    __syncthreads();
    // ---- 5. the first `beam` keys, in order.  A key says all there is to know about its candidate (total, stay or
    // extension, parent's rank, label), so it does not matter where it ends up.
    // a bitonic sort of the padded array, rising: slot r then holds the candidate of place r.  (Ranking by counting
    // the keys below one's own was built first and measured: its N^2 / 256 LDS reads per thread made a frame cost 25 us
    // at 272 candidates and 629 us at 2 112 -- DESIGN section 20.)
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
          N.pb[place] = spb[i];
          N.pnb[place] = spnb[i];
          N.node[place] = B.node[i];
          N.last[place] = B.last[i];
          N.parent[place] = parnode[i];
          N.len[place] = B.len[i];
          N.hash[place] = B.hash[i];
          N.phash[place] = B.phash[i];
          if constexpr (LM != kLmNone) lmv.L[cur ^ 1][place] = lmv.L[cur][i];
          if constexpr (LM == kLmGraph) lmv.st[cur ^ 1][place] = lmv.st[cur][i];
        } else {
          const int c = LM ? int((lo >> 6) & 0x7ffffu) : int(lo & 0x1ffffffu);
          const int nd = 1 + t * W + place;  // (M * beam < 2^31)
          N.pb[place] = NEG_INF;
          if constexpr (LM != kLmNone) {
            // the key holds the combined total: the acoustic score again, by step 4's expression (the same bits; +0
            // for -0, as the key's bits give it), and L of the new prefix, by step 4's too
            const int k = int(lo & 63u);
            const float s = (c == B.last[i] ? B.pb[i] : tot[i]) + sv[k];
            N.pnb[place] = s + 0.0f;
            lmv.L[cur ^ 1][place] = lmv.L[cur][i] + lmv.inc[i * kMaxSet + k];
            if constexpr (LM == kLmGraph) lmv.st[cur ^ 1][place] = lmv.nxt[i * kMaxSet + k];
          } else {
            N.pnb[place] = from_falling_bits(uint32_t(mine >> 32));
          }
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
  const Beams& F = beams[cur];
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
      score = logadd(F.pb[r], F.pnb[r]);
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
void launch_rows(const CtcBeamArgs& a, hipStream_t st) {
  for_row_slices(a, LPR, a.topn + 1, [&](const CtcBeamArgs& s, dim3 grid) {
    hipLaunchKernelGGL(ctc_beam_rows_kernel<LPR>, grid, dim3(kRowBlock), 0, st, s);
  });
}

}  // namespace

void launch_ctc_beam(const CtcBeamArgs& a, int which, hipStream_t st) {
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
    hipLaunchKernelGGL(ctc_beam_search_kernel<kLmGraph>, dim3(static_cast<unsigned>(a.n)), dim3(kSearchBlock), 0, st, a);
  else if (a.lm)
    hipLaunchKernelGGL(ctc_beam_search_kernel<kLmTable>, dim3(static_cast<unsigned>(a.n)), dim3(kSearchBlock), 0, st, a);
  else
    hipLaunchKernelGGL(ctc_beam_search_kernel<kLmNone>, dim3(static_cast<unsigned>(a.n)), dim3(kSearchBlock), 0, st, a);
}

}  // namespace gtnx
