// edit_distance.hip -- batched Levenshtein distance of device-resident token rows, results left on the device (DESIGN
// section 21 holds the contract; tests/edit_distance_fp.py has the same recurrence and the same walk in plain Python).
//
// One launch, one wave of 64 per pair (hyp[b, k], ref[b]); the 64-bit word of Myers' bit-vector recurrence in Hyyro's
// block form IS the wave: lane l of block blk stands for reference row 64 * blk + l, and the match mask of a hypothesis
// token is Eq = __ballot(row < len_ref && ref_token == token) -- any int32 is a token, there are no per-symbol tables.
//
//   forward: the reference is staged in LDS once.  The blocks are taken one after the other (block-major), so a block's
//            (Pv, Mv) are two wave-uniform 64-bit values that never leave registers.  The hypothesis comes in chunks of
//            64 tokens, lane k holding token 64 * c + k (one coalesced load per chunk and block), handed out by
//            readlane.  The horizontal carry between block blk - 1 and blk of column j is one of {-1, 0, +1}: a chunk's
//            64 carries are two 64-bit masks (plus, minus) in LDS, written by block blk - 1 and read by block blk; into
//            block 0 the carry is +1 everywhere (D[0][j] = j).  The distance is followed along row len_ref in the last
//            block: + the bit of Ph, - the bit of Mh at row (len_ref - 1) % 64.
//   walk:    (only with `ops`) the forward pass keeps (Pv, Mv) of every (column, block) in scratch, 16 bytes each,
//            stored by lane blk -- the lane that reads them back, so the walk reads only what the same lane has
//            stored and no ordering between lanes is relied upon.  Column 0 is the constant (all ones, 0).  Lane l holds
//            its block's words of the current column j and of column j - 1 in registers; they are loaded once per
//            column.  D[i][j] is carried along (every move but a match lowers it by one).  Per step
//              D[i-1][j-1] = j - 1 + sum over the lanes of popcount(Pv & low) - popcount(Mv & low)   (column j - 1)
//            decides the diagonal, bit (i - 1) of the current column's Pv decides up, and left is what remains: the
//            contract's order of the moves.
// Lengths are device memory: they are clamped to 0 .. L / 0 .. U here, and nothing at or past a clamped length is read.
// Every store is a plain C++ store; there is no inline assembly and no atomic.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace gtnx {
namespace {

typedef unsigned long long u64;
// (kernels.h: gtnx_ul2 is the 16 bytes (Pv, Mv) of one block of one column)

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ u64 uni64(u64 v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(v));
  const unsigned hi = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(v >> 32));
  return (static_cast<u64>(hi) << 32) | lo;
}

// the sum of `v` over lanes 0 .. nlanes - 1 (the other lanes hold 0), the same value in every lane
__device__ __forceinline__ int wave_sum(int v, int nlanes) {
  if (nlanes <= 8) {
    int s = 0;
    for (int l = 0; l < nlanes; ++l) s += __builtin_amdgcn_readlane(v, l);
    return s;
  }
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

template <bool OPS>
__global__ __launch_bounds__(64) void edit_distance_kernel(EditDistanceArgs a) {
  extern __shared__ u64 s_mem[];
  const int chunks_w = (a.L + 63) >> 6;                      // chunks of the row's width
  u64* s_car = s_mem;                                        // [chunks_w][2]: carries out of the block just done
  int* s_ref = reinterpret_cast<int*>(s_mem + 2 * chunks_w);  // [64 * nbU]

  const int lane = static_cast<int>(threadIdx.x);
  const int64_t p = a.pair0 + static_cast<int64_t>(blockIdx.x);
  const int64_t b = p / a.N;
  const GTNX_G int* hyp = a.hyp + p * a.hyp_stride;
  const GTNX_G int* ref = a.ref + b * a.ref_stride;
  const int m = uni(min(max(a.ref_len[b], 0), a.U));  // rows
  const int n = uni(min(max(a.hyp_len[p], 0), a.L));  // columns
  const int nb = (m + 63) >> 6;
  const int chunks = (n + 63) >> 6;

  for (int i = lane; i < m; i += 64) s_ref[i] = ref[i];
  __syncthreads();

  GTNX_G gtnx_ul2* col = nullptr;  // [L][nbU], this pair's
  if (OPS) col = a.scratch + static_cast<int64_t>(blockIdx.x) * a.L * a.nbU;

  int score = nb == 0 ? n : m;
  const int lastbit = (m - 1) & 63;
  for (int blk = 0; blk < nb; ++blk) {
    const int row = blk * 64 + lane;
    const bool valid = row < m;
    const int rtok = valid ? s_ref[row] : 0;
    const bool last = blk == nb - 1;
    u64 Pv = ~0ull, Mv = 0;
    for (int c = 0; c < chunks; ++c) {
      const int j0 = c * 64;
      const int cnt = min(64, n - j0);
      const int htok = lane < cnt ? hyp[j0 + lane] : 0;
      u64 hp = ~0ull, hm = 0;
      if (blk > 0) {
        hp = uni64(s_car[2 * c]);
        hm = uni64(s_car[2 * c + 1]);
      }
      u64 op = 0, om = 0;
      for (int k = 0; k < cnt; ++k) {
        const int tok = __builtin_amdgcn_readlane(htok, k);
        u64 Eq = __ballot(valid && rtok == tok);
        const u64 hpos = (hp >> k) & 1, hneg = (hm >> k) & 1;
        const u64 Xv = Eq | Mv;
        Eq |= hneg;
        const u64 Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
        u64 Ph = Mv | ~(Xh | Pv);
        u64 Mh = Pv & Xh;
        if (last) score += static_cast<int>((Ph >> lastbit) & 1) - static_cast<int>((Mh >> lastbit) & 1);
        op |= (Ph >> 63) << k;
        om |= (Mh >> 63) << k;
        Ph = (Ph << 1) | hpos;
        Mh = (Mh << 1) | hneg;
        Pv = Mh | ~(Xv | Ph);
        Mv = Ph & Xv;
        if (OPS && lane == blk) {
          gtnx_ul2 w;
          w.x = Pv;
          w.y = Mv;
          col[static_cast<int64_t>(j0 + k) * a.nbU + blk] = w;
        }
      }
      if (!last && lane == 0) {
        s_car[2 * c] = op;
        s_car[2 * c + 1] = om;
      }
    }
    __syncthreads();
  }
  if (lane == 0) a.dist[p] = score;

  if (OPS) {
    int i = m, j = n, d = score;
    int subs = 0, dels = 0, ins = 0;
    // this lane's block of column j (c*) and of column j - 1 (q*); column 0 is (all ones, 0)
    u64 cPv = ~0ull, qPv = ~0ull, qMv = 0;  // (of column j only Pv is asked: the up move)
    int htok = 0;
    if (j > 0 && lane < nb) {
      const gtnx_ul2 w = col[static_cast<int64_t>(j - 1) * a.nbU + lane];
      cPv = w.x;
    }
    if (j > 1 && lane < nb) {
      const gtnx_ul2 w = col[static_cast<int64_t>(j - 2) * a.nbU + lane];
      qPv = w.x;
      qMv = w.y;
    }
    if (j > 0) htok = hyp[j - 1];
    while (i > 0 && j > 0) {
      const int rtok = s_ref[i - 1];
      const int rows = min(max(i - 1 - 64 * lane, 0), 64);  // rows of this lane's block among the first i - 1
      const u64 low = rows == 64 ? ~0ull : ((1ull << rows) - 1);
      const int part = __popcll(qPv & low) - __popcll(qMv & low);
      const int dd = j - 1 + wave_sum(part, (i - 1 + 63) >> 6);  // D[i-1][j-1]
      const int cost = rtok != htok;
      bool shift;
      if (dd + cost == d) {
        subs += cost;
        d = dd;
        --i;
        --j;
        shift = true;
      } else {
        const int r = i - 1;
        const bool up = __ballot(lane == (r >> 6) && ((cPv >> (r & 63)) & 1)) != 0;
        --d;
        if (up) {
          ++dels;
          --i;
          shift = false;
        } else {
          ++ins;
          --j;
          shift = true;
        }
      }
      if (shift) {
        cPv = qPv;
        qPv = ~0ull;
        qMv = 0;
        if (j > 0) {
          htok = hyp[j - 1];
          if (j > 1 && lane < nb) {
            const gtnx_ul2 w = col[static_cast<int64_t>(j - 2) * a.nbU + lane];
            qPv = w.x;
            qMv = w.y;
          }
        }
      }
    }
    dels += i;
    ins += j;
    if (lane == 0) {
      a.ops[p * 3 + 0] = subs;
      a.ops[p * 3 + 1] = dels;
      a.ops[p * 3 + 2] = ins;
    }
  }
}

// the carries of a row's width of columns, then the reference at its width: 32 KB at the largest L and U
size_t lds_bytes(int L, int U) {
  return 16 * static_cast<size_t>((L + 63) / 64) + 256 * static_cast<size_t>((U + 63) / 64);
}

}  // namespace

void launch_edit_distance(const EditDistanceArgs& a, hipStream_t st) {
  if (a.count <= 0) return;
  const size_t lds = lds_bytes(a.L, a.U);
  const dim3 grid(static_cast<unsigned>(a.count)), block(64);
  if (a.ops) hipLaunchKernelGGL(edit_distance_kernel<true>, grid, block, lds, st, a);
  else hipLaunchKernelGGL(edit_distance_kernel<false>, grid, block, lds, st, a);
}

}  // namespace gtnx
