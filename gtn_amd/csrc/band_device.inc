// band_device.inc -- what the band sweeps share, included inside the anonymous namespace of every translation unit that
// instantiates them (band.hip: the sweep kernels; ctc_step.hip: the one-launch CTC step): constants, wave-level
// helpers, the staging of HBM chunks and the LDS layout.  Not a translation unit of its own.
constexpr float NEGF = -1.0e30f;   // log-domain zero
constexpr float DEADF = -1.0e29f;  // anything below is "no path"
constexpr float LOG2E = 1.44269504088896340736f;
constexpr double LN2 = 0.693147180559945309417;
constexpr int BW = 256;  // lanes of one role: 4 sweeper waves + 4 helper waves per workgroup
constexpr int WG = 512;
constexpr int WGB = 768;  // the backward sweep: 4 sweeper + 4 staging + 4 draining waves
constexpr int NBE = 5;   // blocks in the emission / alpha rings: one landing, four in use (lead .. last wave)
constexpr int NBG = 7;   // blocks the backward sweep keeps: one landing, four in use, one being summed, one draining
constexpr int NBGE = 8;  // ... of emissions: they land a tick before the rest of their chunk
#ifndef GTNX_BWD_SPLIT
#define GTNX_BWD_SPLIT 0  // (1: measured slower, see band_backward_kernel)
#endif
#ifndef GTNX_FWD_COPY_DEPTH
#define GTNX_FWD_COPY_DEPTH 2
#endif
#ifndef GTNX_FWD_COPY_ROTATE
#define GTNX_FWD_COPY_ROTATE 1
#endif
#ifndef GTNX_FWD_DEPTH
#define GTNX_FWD_DEPTH 2
#endif

#ifdef GTNX_BAND_TIMING
// diagnostic build (tools/ubench/band_bench.hip): cycles per phase of a tick, wave 0 of workgroup 0
#define GTNX_TM(slot)                 \
  do {                                \
    const long long now_ = clock64(); \
    tm_acc[slot] += now_ - tm_last;   \
    tm_last = now_;                   \
  } while (0)
#define GTNX_TM_INIT(base)                       \
  const int tm_base = base;                      \
  long long tm_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}; \
  long long tm_n = 0;                            \
  long long tm_last = clock64()
#define GTNX_TM_TICK() tm_n += 1
#define GTNX_TM_DUMP()                                                      \
  do {                                                                      \
    if (blockIdx.x == 0 && (threadIdx.x & 63) == 0) {                       \
      for (int i_ = 0; i_ < 7; ++i_) g_band_timing[tm_base + (threadIdx.x >> 6) * 7 + i_] += tm_acc[i_]; \
      if (threadIdx.x == 0) g_band_timing[tm_base + 127] += tm_n;           \
    }                                                                       \
  } while (0)
#else
#define GTNX_TM(slot) do { } while (0)
#define GTNX_TM_INIT(base) do { } while (0)
#define GTNX_TM_TICK() do { } while (0)
#define GTNX_TM_DUMP() do { } while (0)
#endif

__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
#ifdef GTNX_EXP_FAKE_MATH  // (tools/ubench experiment, wrong results: what the sweeps cost with full-rate stand-ins for the transcendentals)
__device__ __forceinline__ float ex2(float x) { return __builtin_fmaf(x, 0.001f, 1.0f); }
__device__ __forceinline__ float lg2(float x) { return __builtin_fmaf(x, 0.001f, -0.001f); }
#else
__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float lg2(float x) { return __builtin_amdgcn_logf(x); }
#endif

// A value that came from a global load and is first used inside the main loop would make the
// compiler put its `s_waitcnt vmcnt` THERE -- where it also waits for every global store issued
// since (stores count in vmcnt on gfx9): one store round trip per gradient row.  settle() is a
// use in front of the loop; uniform() does the same and moves a wave-uniform value to an SGPR.
__device__ __forceinline__ void settle(float& x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void settle(int& x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ float uniform(float x) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}
__device__ __forceinline__ double uniform(double x) {
  const long long b = __double_as_longlong(x);
  const unsigned lo = __builtin_amdgcn_readfirstlane(unsigned(b)), hi = __builtin_amdgcn_readfirstlane(unsigned(b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// lane i <- lane i-1 (lane 0 takes `fill`) / lane i <- lane i+1 (lane 63 takes `fill`)
__device__ __forceinline__ float wave_shr1(float x, float fill) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(x), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_shl1(float x, float fill) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(x), 0x130, 0xf, 0xf, false));
}
// wave64 reductions: six DPP ops (a lane without a source keeps its value), total in lane 63
#define GTNX_DPP6(op)                                                         \
  "s_nop 1\n\t" op " %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"     \
  "s_nop 1\n\t" op " %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"     \
  "s_nop 1\n\t" op " %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"     \
  "s_nop 1\n\t" op " %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"     \
  "s_nop 1\n\t" op " %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"  \
  "s_nop 1\n\t" op " %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"  \
  "s_nop 1"
__device__ __forceinline__ float wave_max(float x) {  // uniform result
  asm volatile(GTNX_DPP6("v_max_f32_dpp") : "+v"(x));
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
}
__device__ __forceinline__ float wave_sum63(float x) {  // lane 63 holds the total
  asm volatile(GTNX_DPP6("v_add_f32_dpp") : "+v"(x));
  return x;
}
__device__ __forceinline__ float wave_sum(float x) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wave_sum63(x)), 63));
}
// two wave64 sums at once (the two chains fill each other's DPP wait states); totals in lane 63
#define GTNX_DPP2(ctl)                                                  \
  "v_add_f32_dpp %0, %0, %0 " ctl "\n\tv_add_f32_dpp %1, %1, %1 " ctl "\n\ts_nop 0\n\t"
__device__ __forceinline__ void wave_sum63x2(float& a, float& b) {
  asm volatile("s_nop 1\n\t"
               GTNX_DPP2("row_shr:1 row_mask:0xf bank_mask:0xf")
               GTNX_DPP2("row_shr:2 row_mask:0xf bank_mask:0xf")
               GTNX_DPP2("row_shr:4 row_mask:0xf bank_mask:0xf")
               GTNX_DPP2("row_shr:8 row_mask:0xf bank_mask:0xf")
               GTNX_DPP2("row_bcast:15 row_mask:0xa bank_mask:0xf")
               GTNX_DPP2("row_bcast:31 row_mask:0xc bank_mask:0xf")
               : "+v"(a), "+v"(b));
}
// the same inside every aligned group of 16 lanes (one DPP row): totals in lanes 15, 31, 47, 63
__device__ __forceinline__ void row_sum15x2(float& a, float& b) {
  asm volatile("s_nop 1\n\t"
               GTNX_DPP2("row_shr:1 row_mask:0xf bank_mask:0xf")
               GTNX_DPP2("row_shr:2 row_mask:0xf bank_mask:0xf")
               GTNX_DPP2("row_shr:4 row_mask:0xf bank_mask:0xf")
               GTNX_DPP2("row_shr:8 row_mask:0xf bank_mask:0xf")
               : "+v"(a), "+v"(b));
}
// all-reduce inside every aligned group of 16 lanes (one DPP row) by rotations
#define GTNX_ROR4(op)                                                        \
  "s_nop 1\n\t" op " %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"    \
  "s_nop 1\n\t" op " %0, %0, %0 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"    \
  "s_nop 1\n\t" op " %0, %0, %0 row_ror:2 row_mask:0xf bank_mask:0xf\n\t"    \
  "s_nop 1\n\t" op " %0, %0, %0 row_ror:1 row_mask:0xf bank_mask:0xf\n\t"    \
  "s_nop 1"
__device__ __forceinline__ float row16_max(float x) {
  asm volatile(GTNX_ROR4("v_max_f32_dpp") : "+v"(x));
  return x;
}
__device__ __forceinline__ float row16_sum(float x) {
  asm volatile(GTNX_ROR4("v_add_f32_dpp") : "+v"(x));
  return x;
}
// log2(2^x0 + 2^x1 + 2^x2): the largest term is exactly 1, so two v_exp_f32 and one v_log_f32
__device__ __forceinline__ float lse3(float x0, float x1, float x2) {
  const float mx = fmaxf(fmaxf(x0, x1), x2);
  const float md = __builtin_amdgcn_fmed3f(x0, x1, x2);
  const float mn = fminf(fminf(x0, x1), x2);
  return mx + lg2(1.0f + ex2(md - mx) + ex2(mn - mx));
}

// what a lane knows about its NPL nodes
template <int NPL>
struct NodeRegs {
  int lab[NPL];      // matched label (0 when the node has no in-arc; its weights are NEGF then)
  float wi[3][NPL];  // in-arc from n-k, log2 units (NEGF: no such arc)
  float wo[3][NPL];  // out-arc to n+k
  int ao[3][NPL];    // arc ids of the out-arcs (-1: none)
  bool has_in[NPL];
  bool start[NPL], accept[NPL];
};
template <int NPL, bool WANT_OUT>
__device__ __forceinline__ void load_nodes(const BandPair& P, int m0, NodeRegs<NPL>& g) {
  const GTNX_G gtnx_i4* nodes = reinterpret_cast<const GTNX_G gtnx_i4*>(P.nodes);
#pragma unroll
  for (int j = 0; j < NPL; ++j) {
    const int m = m0 + j;
    g.lab[j] = 0;
    g.start[j] = g.accept[j] = g.has_in[j] = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      g.wi[k][j] = g.wo[k][j] = NEGF;
      g.ao[k][j] = -1;
    }
    if (m < P.N) {
      const gtnx_i4 q = nodes[m];  // {label, arc from m, arc from m-1, arc from m-2}
      g.lab[j] = q.x >= 0 ? q.x : 0;
      const uint8_t f = P.nflags[m];
      g.start[j] = (f & NF_START) != 0;
      g.accept[j] = (f & NF_ACCEPT) != 0;
      const int a[3] = {q.y, q.z, q.w};
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (a[k] >= 0) {
          g.has_in[j] = true;
          g.wi[k][j] = P.w ? fmaxf(P.w[a[k]] * LOG2E, NEGF) : 0.0f;
        }
    }
    if (WANT_OUT) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (m + k < P.N) {
          const gtnx_i4 q = nodes[m + k];
          const int a = k == 0 ? q.y : (k == 1 ? q.z : q.w);
          if (a >= 0) {
            g.ao[k][j] = a;
            g.wo[k][j] = P.w ? fmaxf(P.w[a] * LOG2E, NEGF) : 0.0f;
          }
        }
      }
    }
  }
}

// emissions land in log2 units with -inf clamped to the finite log-zero
__device__ __forceinline__ float em2(float x) { return fmaxf(x * LOG2E, NEGF); }

// rows of a chunk are contiguous in HBM: element e (0 .. rows * W) -> row e / W; W <= 4096, e <= 4096
__device__ __forceinline__ int row_of(int e, int W, float invW) {
  int r = int(float(e) * invW);
  if (r * W > e) --r;
  if ((r + 1) * W <= e) ++r;
  return r;
}

// A chunk of `rows` contiguous HBM rows of W floats each, staged through NS floats per lane of
// a group of LN lanes: issue() starts the loads, each() hands them back with their coordinates.
template <int NS, int LN = BW>
struct Stage {
  float v[NS];
  // loads are unconditional per lane (lanes past the end re-read the last element): a load under
  // a lane mask would have to be merged with its default, i.e. waited for, right where it is
  // issued.  Whole rounds past the end are skipped (uniform).  VEC is a compile-time choice: with
  // both forms in one kernel the second would wait for the first (they write the same registers)
  template <bool VEC>
  __device__ __forceinline__ void issue(const GTNX_G float* src, int cnt, int tid) {
    if (cnt <= 0) return;  // uniform
    // Both modes fetch the chunk -- K rows, contiguous in HBM -- with 16-byte loads (global_load_dwordx4 needs
    // dword alignment only).  VEC: rows are a multiple of 4 floats and the source is 16-byte aligned, so a load
    // never straddles two rows and lands with one 16-byte LDS store at a precomputed offset.  !VEC (any
    // alphabet, any alignment): the same loads, landed element by element with the row found per element.
    // (C = 255 used to take one 4-byte load per element: 2.6x the backward sweep's time at C = 256.)
    // (cnt >= 4: the band path takes alphabets of at least 4 labels -- band_min_labels())
#pragma unroll
    for (int i = 0; i < NS / 4; ++i) {
      if (i > 0 && 4 * i * LN >= cnt) break;  // uniform
      const int e = min(4 * (i * LN + tid), cnt - 4);
      // (e >= 0: a 32-bit BYTE offset beside the uniform base -- no 64-bit lane arithmetic, no register pair per slot)
      const gtnx_f4 q = *reinterpret_cast<const GTNX_G gtnx_f4*>(reinterpret_cast<const GTNX_G char*>(src) + unsigned(4 * e));
      v[4 * i] = q.x;
      v[4 * i + 1] = q.y;
      v[4 * i + 2] = q.z;
      v[4 * i + 3] = q.w;
    }
  }
  // VEC mode: where slot i of a FULL chunk of K rows lands in a ring block whose rows are `stride`
  // floats apart and in reverse order (chunk row r -> block row K-1-r), computed once: a chunk of
  // fewer rows sits (K - rows) block rows lower
  // (reverse = false: the forward sweep's ring, chunk row r -> block row r)
  int off[NS / 4];
  __device__ __forceinline__ void init_offsets(int W, int stride, int K, int tid, bool reverse = true) {
    const float invW = 1.0f / float(W);
#pragma unroll
    for (int i = 0; i < NS / 4; ++i) {
      const int e = 4 * (i * LN + tid);
      const int r = row_of(min(e, 4096), W, invW);
      off[i] = (reverse ? K - 1 - r : r) * stride + (e - r * W);
    }
  }
  // f(i, ring offset, values) for the slots of a chunk of `rows` rows of W floats
  template <class F>
  __device__ __forceinline__ void each_vec(int cnt, int shift, int tid, F&& f) const {
#pragma unroll
    for (int i = 0; i < NS / 4; ++i) {
      if (i > 0 && 4 * i * LN >= cnt) break;  // uniform
      if (4 * (i * LN + tid) < cnt) f(i, off[i] - shift, gtnx_f4{v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]});
    }
  }
  // a use of every staging register: all of this wave's loads are waited for HERE, and the
  // compiler knows that none is pending when the next issue() reuses the registers
  __device__ __forceinline__ void settle_all() {
#pragma unroll
    for (int i = 0; i < NS; ++i) asm volatile("" : "+v"(v[i]));
  }
  // VEC: f(i, e, r, c, q) per 16-byte slot -- slot index, element, chunk row, column, the four values.
  // !VEC: f(i, e, r, c, {x, 0, 0, 0}) per ELEMENT (a slot may straddle rows; the last slot of a chunk whose size
  // is not a multiple of 4 was fetched from cnt - 4 and lands there: the overlap rewrites the same values)
  template <bool VEC, class F>
  __device__ __forceinline__ void each(int cnt, int W, int tid, F&& f) const {
    const float invW = 1.0f / float(W);
    if constexpr (VEC) {
#pragma unroll
      for (int i = 0; i < NS / 4; ++i) {
        if (i > 0 && 4 * i * LN >= cnt) break;  // uniform
        const int e = 4 * (i * LN + tid);
        if (e < cnt) {
          const int r = row_of(e, W, invW);
          f(i, e, r, e - r * W, gtnx_f4{v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]});
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < NS / 4; ++i) {
        if (i > 0 && 4 * i * LN >= cnt) break;  // uniform
        if (4 * (i * LN + tid) < cnt) {
          const int e = min(4 * (i * LN + tid), cnt - 4);
          const int r0 = row_of(e, W, invW), c0 = e - r0 * W;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            // (W >= 4: an element is in row r0 or the next one.  No loop in here: anything the compiler cannot
            //  unroll turns v[] into a runtime-indexed array in scratch memory)
            int r = r0, col = c0 + k;
            if (col >= W) {
              col -= W;
              ++r;
            }
            f(i, e + k, r, col, gtnx_f4{v[4 * i + k], 0.0f, 0.0f, 0.0f});
          }
        }
      }
    }
  }
};

// LDS layout shared by host (size) and device (carving); all counts in floats
struct BandLds {
  int CS;  // ring row stride of emission rows
  int o_ering, o_aring, o_oring, o_snode, o_misc, total;
};
__host__ __device__ inline BandLds band_lds(int C, int K, int NSmax, bool backward) {
  BandLds L;
  L.CS = C + 4;
  int o = 0;
  L.o_ering = o;  // the backward sweep keeps a block's emissions until its gradient rows are out
  o += (backward ? NBGE : NBE) * K * L.CS;
  o = (o + 3) & ~3;
  L.o_aring = o;  // alpha rows
  o += backward ? NBE * K * NSmax : 0;
  o = (o + 3) & ~3;
  L.o_oring = o;  // node posteriors (>= 2C ints: the prologue sorts labels here)
  o += backward ? max(NBG * K * NSmax, 2 * C) : 0;
  o = (o + 3) & ~3;
  L.o_snode = o;  // nodes sorted by (label, node)
  o += backward ? 512 : 0;
  // doubles: offr[5][16], red[16], find[4], aofr[NBE][K][4] | floats: bndr[5][4K][2], fin[8], lsep[2][16][8][2] / lser[NBG][K]
  // (region 0 of offr / bndr is constant: what the first wave of the pipeline reads as its neighbour)
  L.o_misc = o;
  o += 160 + 32 + 8 + 2 * NBE * K * 4 + 40 * K + 8 + 512;
  L.total = o;
  return L;
}
struct BandMisc {
  double *offr, *red, *find, *aofr;
  float *bndr, *fin, *lsep;
};
template <int K>
__device__ __forceinline__ BandMisc band_misc(float* lds, const BandLds& L) {
  BandMisc m;
  m.offr = reinterpret_cast<double*>(lds + L.o_misc);
  m.red = m.offr + 80;
  m.find = m.red + 16;
  m.aofr = m.find + 4;
  m.bndr = lds + L.o_misc + 200 + 2 * NBE * K * 4;
  m.fin = m.bndr + 40 * K;
  m.lsep = m.fin + 8;
  return m;
}

// shift of a wave's running row by its maximum; the reduction is independent of the next
// steps' chain, so the scheduler may interleave it with them
__device__ __forceinline__ float wave_max_of(const float* v, int n) {
  float mx = v[0];
  for (int j = 1; j < n; ++j) mx = fmaxf(mx, v[j]);
  return wave_max(mx);
}

// ==========================================================================================
// CTC target acceptors built where they are used: the graph of benchmarks/ctc.cpp:40-58 /
// examples/ctc.cpp:21-41 (2U+1 nodes, blank at even nodes, self-loop + arc from the previous
// node everywhere, a skip arc between different labels; arc ids in the reference's addArc
// order) as the band records the sweeps read -- one workgroup per label sequence, nothing but
// the labels crosses PCIe.  Lists sorted by (label, node) as band_info() makes them on the host.
// ==========================================================================================
// (the records of ONE sequence by one workgroup of at least 260 lanes: ctc_targets_kernel below, and the head of the
//  one-launch CTC step, ctc_step.hip.  tl, tk: 260 ints of LDS each, 16-byte aligned)
__device__ __forceinline__ void ctc_target_records(const CtcTargetArgs& a, int blank, int* tl, int* tk) {
  // tl, tk: the label sequence and its skip flags (label i differs from label i - 1), padded to whole 16-byte reads
  const int N = a.N, U = (N - 1) >> 1, m = threadIdx.x;
  if (m < 260) {
    const int v = m < U ? a.labels[m] : 0x7fffffff;  // (padding: above every real label, no skip arc)
    tl[m] = v;
    tk[m] = (m > 0 && m < U && v != a.labels[m - 1]) ? 1 : 0;
  }
  __syncthreads();
  if (m >= N) return;
  const bool odd = (m & 1) != 0;
  const int my = odd ? tl[(m - 1) >> 1] : blank;
  const int skip = odd ? tk[(m - 1) >> 1] : 0;
  // Rank among the (label, node) pairs and first arc id.  Node 2i + 1 carries label i, every even node the blank:
  // the nodes in front of (my, m) are the label nodes with a smaller label (or mine, earlier) -- one pass over the
  // U labels, four per LDS read, where rounds 2-5 compared against all N nodes -- plus a closed form for the blanks.
  // The arcs in front of node m: one self loop per node, one step arc per node but the first, the skips counted
  // in the same pass.
  const int mi = (m - 1) >> 1;  // (odd m: my own label index; even m: labels 0 .. m/2 - 1 lie in front of me)
  const int before = odd ? mi : (m >> 1);  // label indices < before belong to nodes in front of m
  int rank = 0, skips = 0;
  for (int o = 0; o < U; o += 4) {
    const gtnx_i4 l4 = *reinterpret_cast<const gtnx_i4*>(tl + o), k4 = *reinterpret_cast<const gtnx_i4*>(tk + o);
    const int lo[4] = {l4.x, l4.y, l4.z, l4.w}, ko[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool front = o + k < before;
      rank += (lo[k] < my || (lo[k] == my && front)) ? 1 : 0;
      skips += front ? ko[k] : 0;
    }
  }
  // the blank nodes (even, U + 1 of them): all in front of a larger label, the earlier ones in front of an equal one
  rank += blank < my ? U + 1 : (blank == my ? (m + 1) >> 1 : 0);
  const int base = (m > 0 ? 2 * m - 1 : 0) + skips;
  GTNX_G BandNode* nd = const_cast<GTNX_G BandNode*>(a.nodes);
  nd[m].lab = my;
  nd[m].aid[0] = base;
  nd[m].aid[1] = m > 0 ? base + 1 : -1;
  nd[m].aid[2] = skip ? base + 2 : -1;
  a.nflags[m] = uint8_t((m == 0 ? NF_START : 0) | (m + 2 >= N ? NF_ACCEPT : 0));
  a.snode[rank] = m;
  a.slab[rank] = my;
  if (m == N - 1 && a.n_arcs) a.n_arcs[0] = base + 1 + (m > 0 ? 1 : 0) + skip;
}
