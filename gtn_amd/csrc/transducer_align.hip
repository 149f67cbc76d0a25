// transducer_align.hip -- the best alignment of a known transcript on the transducer lattice: the max-plus half of
// transducer.hip's criterion over the same compact plane (lp_blank, lp_label, lse) per node, whichever rows kernel left
// it (DESIGN section 46 holds the contract; tests/transducer_align_fp.py has the recurrence and the walk in numpy).
//
//   v[0,0] = 0;  v[t,u] = max(v[t-1,u] + lp_blank[t-1,u], v[t,u-1] + lp_label[t,u-1]);  of equal candidates the blank
//   arc wins;  score = v[T_b-1, U_b] + lp_blank[T_b-1, U_b].
//
// One wave per utterance, one launch:
//   sweep:  transducer_sweep_kernel's skew.  Lane l owns the K = 1, 2, 4, 8, 16 columns l K .. l K + K - 1 in registers,
//           advances row t = s - l at step s, takes the left neighbour's carry through the DPP wave shift and has loaded
//           the next row's compact values before it computes the current one.  A node is a compare, a select and two
//           adds.  The K decisions of a lane and row (bit k set: node (t, l K + k) is entered by its label arc) are one
//           word of 8 (K <= 8) or 16 bits at plane[t][l]: one bit per node, no alpha plane.  The plane lives in LDS while
//           T rows of it fit 60 KiB (960 rows, 480 for K == 16), else in the caller's scratch.
//   walk:   from (T_b - 1, U_b) to (0, 0), wave-uniform: the word of (t, lane) is read from LDS once per row and lane, a
//           label step writes its frame into an LDS table of U entries and nothing goes to global memory.  With the plane
//           in scratch the wave first copies a window of rows into LDS with 16-byte loads and refills it when the walk
//           leaves it below.  The wave's own stores are made visible to its loads by the workgroup barrier.
//   out:    all lanes store token_frames and gather token_scores from the compact plane, and take frame_tokens[t] as the
//           number of tokens emitted at frames <= t by a binary search of the LDS table; the -1 / -inf tails and the
//           outputs of an utterance without a path come from the same loops, so every element is stored exactly once.
// Every store is a plain C++ store; there are no atomics and no inline assembly.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "kernels.h"

namespace gtnx {
namespace {

constexpr float NEG_INF = -__builtin_inff();
constexpr float POS_INF = __builtin_inff();
constexpr int kPlaneLds = 60 << 10;  // the LDS budget of the bit plane (or of its window); the frame table has 4 KiB

template <int K>
struct WordOf {
  typedef uint8_t type;
};
template <>
struct WordOf<16> {
  typedef uint16_t type;
};
typedef unsigned int u4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
// a value of a plane the caller may have filled: NaN and +inf close the arc
__device__ __forceinline__ float arc(float v) { return v < POS_INF ? v : NEG_INF; }
// lane l's value of lane l - 1 (lane 0: `edge`); every lane of the wave takes part
__device__ __forceinline__ float from_lower_lane(float v, float edge) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x138, 0xf, 0xf, false));
}

template <int K, bool SCRATCH>
__global__ __launch_bounds__(64) void transducer_align_kernel(TransducerAlignArgs a) {
  typedef typename WordOf<K>::type Word;
  constexpr int kWinRows = kPlaneLds / (64 * int(sizeof(Word)));
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // (the bit plane's rows 0 .. T - 1, or a window of kWinRows of them; then the frame of every token)
  Word* win = reinterpret_cast<Word*>(smem);
  int* tf = reinterpret_cast<int*>(smem + size_t(SCRATCH ? kWinRows : a.T) * 64 * sizeof(Word));

  const int lane = static_cast<int>(threadIdx.x);
  const int lb = static_cast<int>(blockIdx.x), b = a.utt0 + lb;
  const int Tb = uni(a.frames[b]), Ub = uni(a.tlen[b]);
  const int U1 = a.U1, U = U1 - 1;
  const GTNX_G float* rows = a.rows + static_cast<int64_t>(lb) * a.T * U1 * 3;
  GTNX_G Word* plane = SCRATCH ? reinterpret_cast<GTNX_G Word*>(a.plane) + static_cast<int64_t>(lb) * a.T * 64 : nullptr;
  const bool valid = Tb >= 1 && Tb <= a.T && Ub >= 0 && Ub < U1;

  float score = NEG_INF;
  if (valid) {
    const int u0 = lane * K;
    const int lmax = Ub / K, kend = Ub - lmax * K;  // the lane and the register that own column U_b
    const int steps = Tb + lmax;
    const bool mine = lane <= lmax;

    float keep[K];       // v[t-1, u] + lp_blank[t-1, u] of the row done last
    float nb[K], nl[K];  // the compact values of the row to do next
#pragma unroll
    for (int k = 0; k < K; ++k) keep[k] = NEG_INF;
    if (lane == 0) keep[0] = 0.0f;  // (the start enters node (0, 0))

    // (t outside 0 .. T_b - 1 and u > U_b load nothing: -inf)
    auto load = [&](int t, float* pb, float* pl) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        pb[k] = NEG_INF;
        pl[k] = NEG_INF;
        if (t >= 0 && t < Tb && u0 + k <= Ub) {
          const GTNX_G float* p = rows + (static_cast<int64_t>(t) * U1 + u0 + k) * 3;
          pb[k] = arc(p[0]);
          pl[k] = arc(p[1]);
        }
      }
    };

    float carry = NEG_INF;
    load(-lane, nb, nl);
    for (int s = 0; s < steps; ++s) {
      const int t = s - lane;
      float cb[K], cl[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        cb[k] = nb[k];
        cl[k] = nl[k];
      }
      load(t + 1, nb, nl);
      float left = from_lower_lane(carry, NEG_INF);
      if (mine && t >= 0 && t < Tb) {
        unsigned word = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const bool label = left > keep[k];  // (equal: the blank arc; -inf never beats a finite candidate)
          const float v = label ? left : keep[k];
          word |= (label ? 1u : 0u) << k;
          keep[k] = v + cb[k];
          left = v + cl[k];
        }
        carry = left;
        if (SCRATCH) plane[static_cast<int64_t>(t) * 64 + lane] = static_cast<Word>(word);
        else win[t * 64 + lane] = static_cast<Word>(word);
      }
    }
    float sc = NEG_INF;
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (k == kend) sc = keep[k];
    score = __shfl(sc, lmax, 64);
  }
  if (lane == 0) a.scores[b] = score;
  const bool path = score > NEG_INF;  // (the same in every lane)

  if (path) {
    __syncthreads();  // the sweep's words, LDS or global, are visible to every lane
    int t = Tb - 1, u = Ub;
    int ln = u / K, k = u - ln * K;
    int lo = SCRATCH ? Tb : 0;  // the window holds rows lo .. lo + kWinRows - 1
    bool need = true;
    unsigned w = 0;
    while (t > 0 || u > 0) {
      if (SCRATCH && t < lo) {
        __syncthreads();
        lo = t + 1 > kWinRows ? t + 1 - kWinRows : 0;
        const int n16 = (t - lo + 1) * 4 * int(sizeof(Word));  // 16-byte pieces of rows lo .. t
        const GTNX_G u4* src = reinterpret_cast<const GTNX_G u4*>(plane + static_cast<int64_t>(lo) * 64);
        for (int i = lane; i < n16; i += 64) reinterpret_cast<u4*>(win)[i] = src[i];
        __syncthreads();
      }
      if (need) {
        w = win[(t - lo) * 64 + ln];
        need = false;
      }
      const bool label = t == 0 || (u > 0 && ((w >> k) & 1u));
      if (label) {
        --u;
        if (lane == 0) tf[u] = t;
        if (k == 0) {
          k = K - 1;
          --ln;
          need = true;
        } else {
          --k;
        }
      } else {
        --t;
        need = true;
      }
    }
    __syncthreads();  // lane 0's table is visible to every lane
  }

  // ---- outputs: every element exactly once ----
  const int nlive = path ? Ub : 0;
  GTNX_G int* otf = a.token_frames + static_cast<int64_t>(b) * U;
  GTNX_G float* ots = a.token_scores ? a.token_scores + static_cast<int64_t>(b) * U : nullptr;
  for (int u = lane; u < U; u += 64) {
    const int f = u < nlive ? tf[u] : -1;
    otf[u] = f;
    if (ots) ots[u] = f >= 0 ? arc(rows[(static_cast<int64_t>(f) * U1 + u) * 3 + 1]) : NEG_INF;
  }
  if (a.frame_tokens) {
    GTNX_G int* oft = a.frame_tokens + static_cast<int64_t>(b) * a.T;
    for (int t = lane; t < a.T; t += 64) {
      int c = -1;
      if (path && t < Tb) {  // the number of tokens emitted at frames <= t
        int l = 0, h = nlive;
        while (l < h) {
          const int mid = (l + h) >> 1;
          if (tf[mid] <= t) l = mid + 1;
          else h = mid;
        }
        c = l;
      }
      oft[t] = c;
    }
  }
}

template <int K>
constexpr int lds_rows() {
  return kPlaneLds / (64 * int(sizeof(typename WordOf<K>::type)));
}

template <int K>
void align_launch(const TransducerAlignArgs& a, hipStream_t st) {
  const size_t table = sizeof(int) * size_t(kTransducerMaxU1);
  if (a.plane) {
    hipLaunchKernelGGL((transducer_align_kernel<K, true>), dim3(unsigned(a.count)), dim3(64), size_t(kPlaneLds) + table,
                       st, a);
  } else {
    const size_t lds = size_t(a.T) * 64 * sizeof(typename WordOf<K>::type) + table;
    hipLaunchKernelGGL((transducer_align_kernel<K, false>), dim3(unsigned(a.count)), dim3(64), lds, st, a);
  }
}

inline int k_of(int U1) {
  const int k = (U1 + 63) / 64;
  return k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : 16;
}

}  // namespace

size_t transducer_align_plane_bytes(int T, int U1) {
  const bool wide = k_of(U1) == 16;
  if (T <= (wide ? lds_rows<16>() : lds_rows<8>())) return 0;
  return size_t(T) * 64 * (wide ? 2 : 1);
}

void launch_transducer_align(const TransducerAlignArgs& a, hipStream_t st) {
  if (a.count <= 0) return;
  switch (k_of(a.U1)) {
    case 1: align_launch<1>(a, st); break;
    case 2: align_launch<2>(a, st); break;
    case 4: align_launch<4>(a, st); break;
    case 8: align_launch<8>(a, st); break;
    default: align_launch<16>(a, st); break;
  }
  HIP_CHECK(hipGetLastError());
}

}  // namespace gtnx
