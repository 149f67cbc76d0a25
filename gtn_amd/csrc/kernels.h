// kernels.h -- device-side views (PODs laid out in HBM) and the launch entry
// points of the HIP kernels.  Everything here is plain data + free functions so
// the host runtime (graph.cpp / ops.cpp) never sees kernel internals.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

// kernel attributes (hipFuncSetAttribute: the dynamic LDS limit) belong to a (function, DEVICE) pair: a launcher sets
// them the first time it runs on each device, not once per process (runtime.h: one context per device)
#include <atomic>
#include <cstdint>
// `if (auto first = gtnx_first_on_device(done)) { ...hipFuncSetAttribute... }`: the device's bit is published when
// `first` goes out of scope, i.e. AFTER the attribute calls -- a second thread launching on the same device meanwhile
// (the side-stream thread) sees it clear and sets the attributes itself (twice is harmless) instead of launching
// under the default limit
struct gtnx_first_on_device {
  std::atomic<uint64_t>& done;
  uint64_t bit;
  bool first;
  explicit gtnx_first_on_device(std::atomic<uint64_t>& d) : done(d) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    bit = uint64_t(1) << (dev & 63);
    first = !(done.load(std::memory_order_acquire) & bit);
  }
  gtnx_first_on_device(const gtnx_first_on_device&) = delete;
  ~gtnx_first_on_device() {
    if (first) done.fetch_or(bit, std::memory_order_acq_rel);
  }
  explicit operator bool() const { return first; }
};

namespace gtnx {

// Pointers inside the argument structs are loaded from memory, so the compiler
// would treat them as generic ("flat") addresses: flat_load/flat_store, which
// are slower and -- worse -- tick lgkmcnt as well as vmcnt, so an LDS-only
// barrier (s_waitcnt lgkmcnt(0); s_barrier) would still wait for every HBM
// access in flight.  In device code the members are therefore typed as GLOBAL
// (address space 1) pointers; the host sees ordinary pointers of the same size.
#if defined(__HIP_DEVICE_COMPILE__)
#define GTNX_G __attribute__((address_space(1)))
#else
#define GTNX_G
#endif

// 16-byte adjacency record as a builtin vector (loadable from any address space)
typedef int gtnx_i4 __attribute__((ext_vector_type(4)));
typedef float gtnx_f4 __attribute__((ext_vector_type(4)));

enum : int { KIND_EXPLICIT = 0, KIND_LINEAR = 1 };
enum : int { NF_START = 1, NF_ACCEPT = 2, NF_ORPHAN = 4 /* unqueued accept node: score 0.0 */ };

// ---------------------------------------------------------------------------
// Structure-of-arrays view of one graph in HBM (replaces gtn/graph.h:58-73's
// AoS Arc + per-node std::vector<int> in/out).  Arc arrays are in arc-id (API)
// order.  Adjacency is CSR over arc ids: out_list[out_off[n] .. out_off[n+1])
// is Graph::out(n) in the reference's list order, likewise in_*.
// KIND_LINEAR (gtn/creations.cpp:20-33) stores nothing but (M, C): arc a is
// (a / C) -> (a / C + 1) with label a % C; only the weight tensor is material.
// ---------------------------------------------------------------------------
struct DGraph {
  int kind;
  int N, A;
  int M, C;
  int n_start, n_accept;
  int flags;  // bit0 ilabelSorted, bit1 olabelSorted, bit2 GF_EPS_FREE (no epsilon label on any arc), bit3 GF_ACCEPTOR
  const GTNX_G int* src;
  const GTNX_G int* dst;
  const GTNX_G int* il;
  const GTNX_G int* ol;
  const GTNX_G uint8_t* nflags;
  const GTNX_G int* start_list;
  const GTNX_G int* accept_list;
  const GTNX_G int* out_off;
  const GTNX_G int* out_list;  // nullptr => identity (arcs already grouped by src in id order)
  const GTNX_G int* in_off;
  const GTNX_G int* in_list;
  // packed adjacency records in list order: {ilabel, olabel, dst (out) / src (in), arc id};
  // present for host-built graphs, nullptr for device-built ones
  const GTNX_G gtnx_i4* out_rec;
  const GTNX_G gtnx_i4* in_rec;
  const GTNX_G float* w;  // weights, arc-id order (filled per op; not part of the structure)
};

// ---------------------------------------------------------------------------
// Level schedule of a DAG for shortest distance, in *position space*: nodes
// renumbered by their place in the reference's Kahn FIFO order
// (gtn/functions/shortest.cpp:96-145), grouped into dependency levels.
//   rows   : row_off[p] .. row_off[p+1] index in_srcpos/in_arc  (in-arcs of p)
//   in_w   : optional weights permuted into row order (compose emits it)
//   out_*  : the transposed rows for the backward sweep
// Device-built layered products have position == node id and out_arc == nullptr
// (arc k is the k-th out entry).
// ---------------------------------------------------------------------------
struct DSched {
  int P;  // scheduled nodes
  int L;  // levels
  int n_accept;
  int flags;  // bit0: tie-break by arc id (rows unordered); bit1: out rows are identity
  const GTNX_G int* level_off;  // [L+1]
  const GTNX_G int* row_off;    // [P+1]
  const GTNX_G int* in_srcpos;  // [Ain]
  const GTNX_G int* in_arc;     // [Ain] arc ids
  const GTNX_G int* in_rank;    // [Ain] push rank for viterbiPath ties (nullptr => arc id)
  const GTNX_G float* in_w;     // [Ain] or nullptr
  const GTNX_G uint8_t* pflags; // [P] NF_START | NF_ACCEPT by position
  const GTNX_G int* acc_pos;    // [n_accept] position of accept()[k]
  const GTNX_G int* out_off;    // [P+1]
  const GTNX_G int* out_dstpos; // [Aout]
  const GTNX_G int* out_arc;    // [Aout] or nullptr (identity)
};
enum : int { SCHED_TIE_BY_ARC = 1, SCHED_OUT_IDENTITY = 2 };

// the same schedule built on the device from the graph's CSR arrays (levelize.hip); positions inside a level
// are in node-id order (no queue replay: not for viterbiPath's tie-break)
struct LevelizeOut {
  int* level_off;    // [N + 2]
  int* row_off;      // [N + 1]
  int* in_srcpos;    // [A]
  int* in_arc;       // [A]
  uint8_t* pflags;   // [N]
  int* acc_pos;      // [n_accept]
  int* out_off;      // [N + 1]
  int* out_dstpos;   // [A]
  int* out_arc;      // [A]
};
enum : int { LV_P = 0, LV_L, LV_N_IN, LV_N_OUT, LV_ERROR, LV_MAX_WIDTH, LV_MAX_LEVEL_ARCS, LV_MAX_REACH, LV_INFO_INTS };
size_t levelize_scratch_bytes(int N, int A);
void device_levelize(const DGraph& g, const LevelizeOut& out, void* scratch, int* info_host /* LV_INFO_INTS */, hipStream_t st);

// per-graph result of the forward sweep (kept for the backward sweep)
struct SdResult {
  float score;      // shortest.cpp:159
  float max_final;  // maxScoresCache.back()
  int argmax_final; // position of the arg-max accept node (tropical), -1 if none
  int pad;
};

// one shortest-distance problem
struct SdArgs {
  DSched s;
  const GTNX_G float* w;   // arc-id order weights
  GTNX_G float* scores;    // [P]
  GTNX_G int* argmax;      // [P] tropical only (arc id, -1 = the start node's virtual 0)
  GTNX_G SdResult* result; // [1]
  GTNX_G float* out_score; // [1] the scalar graph's weight
  // backward
  const GTNX_G float* delta;  // [1] upstream gradient of the scalar
  GTNX_G float* node_grad;    // [P]
  GTNX_G float* arc_grad;     // [A] arc-id order
  int chunk_levels;           // narrow kernels: levels per LDS chunk (host: caps / widest level)
  // narrow kernels: when set, P / L / accept count are read from the producing compose's
  // result block on the device (the host may not know them yet -- graph.h DeferredSizes)
  const GTNX_G struct ComposeOut* dyn_out;
  const GTNX_G int* dyn_counts;
  // fused compose-gradient scatter (narrow backward only; see sd_narrow_fuse_caps):
  // arc k of the lattice came from arc gi_fixed[k] of the explicit compose input and
  // arc gi_chain[k] of the linear chain, whose arcs of level l lie in [l*C, (l+1)*C)
  const GTNX_G int* gi_fixed;
  const GTNX_G int* gi_chain;
  GTNX_G float* grad_fixed;   // [fixed_A] zero-filled by the host; may be null
  GTNX_G float* grad_chain;   // [T*C]     zero-filled by the host; may be null
  int chain_C, fixed_A, chain_A;
  int chain_accumulate;  // grad_chain already holds a gradient: rows are added to, not stored
};

enum : int { SD_LOG = 0, SD_TROPICAL = 1, SD_PATH = 2 };

// narrow != 0 (2: every graph carries row-ordered weights in_w) selects the LDS-ring kernel for deep, narrow lattices (every graph
// of the batch must satisfy: level arcs <= sd_narrow_tmp_cap(), per-level reach
// <= sd_narrow_ring()); only the log semiring has it so far.
int sd_narrow_ring();
int sd_narrow_tmp_cap();
int sd_narrow_node_cap();
void launch_sd_forward(const SdArgs* d_args, int n, int mode, int narrow,
                       int avg_in_degree_x16, hipStream_t st);
// deep, thin DAGs in the log semiring (thousands of levels of one or two nodes): one wave per graph, scores /
// node gradients in LDS, rows staged a chunk ahead (shortest.hip).  Every graph needs P <= sd_deep_node_cap().
int sd_deep_node_cap();
void launch_sd_forward_deep(const SdArgs* d_args, int n, int maxP, hipStream_t st);
void launch_sd_backward_deep(const SdArgs* d_args, int n, int maxP, hipStream_t st);
int sd_narrow_ring_backward();
// narrow != 0: LDS-ring kernel (log semiring, identity out rows, eligibility as forward
// with reach <= sd_narrow_ring_backward())
// narrow == 2: as 1, plus the fused gradient scatter into the compose inputs (every
// graph must satisfy fixed_A <= cap_fixed and chunk_levels * chain_C <= cap_chain)
// fuse_lds_bytes (narrow == 2): dynamic LDS of the chain window, max over the batch of
// chunk_levels * chain_C * 4
void launch_sd_backward(const SdArgs* d_args, int n, int mode, int narrow, int avg_out_degree_x16, hipStream_t st,
                        int fuse_lds_bytes = 0);
void sd_narrow_fuse_caps(int* cap_fixed, int* cap_chain);
// diagnostics: launches per kernel cell (direction / family / mode / lanes per node) since the process started, counted
// on the host by the four launch functions above (gtn_amd.h: gtnx_debug_shortest_routes)
int sd_route_cells();
const char* sd_route_name(int cell);  // "" outside [0, sd_route_cells())
int64_t sd_route_launches(int cell);

// viterbiPath pointer chase (shortest.cpp:239-245): writes path arc ids first-arc-first
struct PathArgs {
  DSched s;
  DGraph g;
  const GTNX_G int* argmax;       // back-pointers by position (arc id / -1)
  const GTNX_G SdResult* result;
  GTNX_G int* path_arcs;          // [cap]
  GTNX_G int* path_il;            // [cap]
  GTNX_G int* path_ol;            // [cap]
  GTNX_G float* path_w;           // [cap]
  GTNX_G int* path_len;           // [4]: length, has_node, exact tie on the path, -
  int cap;
  // exact-tie check of the visited nodes (path_tie_kernel): node scores by position, weights by arc id
  const GTNX_G float* scores;
  const GTNX_G float* w;
  GTNX_G int* path_pos;           // [cap] position of the node each path arc enters
  GTNX_G int* pred;               // [P] scratch: position of the node each position's best in-arc leaves (-1: none)
  GTNX_G int* tmp;                // [cap] scratch: the visited positions, last first
};
void launch_path_chase(const PathArgs* d_args, int n, int max_cap, int max_P, hipStream_t st);

// ---------------------------------------------------------------------------
// linear-chain emissions graphs: forwardScore / viterbiScore and their grads
// are row reductions over the [M][C] weight tensor (no graph traversal).
// ---------------------------------------------------------------------------
struct LinArgs {
  const GTNX_G float* w;   // [M][C]
  int M, C;
  GTNX_G float* out_score; // [1]
  GTNX_G float* partial;   // [splits]
  const GTNX_G float* delta;
  GTNX_G float* grad;      // [M][C]
  int accumulate;          // backward: grad += (the graph already holds a gradient) instead of grad =
};
// vec_rows != 0 (log semiring only): every member has C % 4 == 0, C <= 1024 and 16-byte
// aligned weight / gradient rows -- rows are reduced out of registers (linear_rows_kernel)
void launch_linear_forward(const LinArgs* d_args, int n, int tropical, int vec_rows, hipStream_t st);
void launch_linear_backward(const LinArgs* d_args, int n, int tropical, int vec_rows, hipStream_t st);

// ---------------------------------------------------------------------------
// composition (gtn/functions/compose.cpp:377-522)
// ---------------------------------------------------------------------------
enum : int { MATCH_UNSORTED = 0, MATCH_SINGLY_G1 = 1, MATCH_SINGLY_G2 = 2, MATCH_DOUBLY = 3 };

struct ComposeOut {
  int N, A, L;
  int layered;   // every arc goes from BFS level k to k+1
  int overflow;  // capacity exceeded (host bound was wrong) -- never expected
  int max_width;       // widest BFS level (nodes)
  int max_level_arcs;  // most arcs emitted by one level
  int csr_built;       // in_off / in_list / in_src / in_w were built inside compose_kernel
  int rep_levels;      // BFS levels emitted by stationary-level replication (not expanded one by one)
  int skipped;         // src / il / ol / in_list were NOT written (ComposeArgs::skip honoured); see compose_fill
  int t_b, t_f, t_rep; // 100 MHz ticks spent in phase B / phase F (total) / replication (diagnostics)
  // compose_wide.hip: the hole its plan kernel left for the replication kernel -- levels wr_L + 1 .. wr_L + wr_K
  // are level wr_L (frontier ids wr_lo .. wr_lo + wr_W, arcs wr_na .. wr_na + wr_Aw) moved in time
  int wr_L, wr_K, wr_lo, wr_W, wr_na, wr_Aw;
};

constexpr int GF_EPS_FREE = 4;
constexpr int GF_ACCEPTOR = 8;  // ilabel == olabel on every arc (known at upload; products of acceptors inherit it)

struct ComposeArgs {
  DGraph g1, g2;
  int matcher;
  int lds_state;  // co-reachability / discovered bitmaps live in LDS
  // FAST variant only: leave out the arrays that are derivable from the others (src from
  // out_off; il / ol from gradInfo and the inputs' labels; in_list by re-scattering the
  // in-rows) -- 16 of the 40 bytes a composed arc costs.  launch_compose_fill() writes
  // them when somebody needs them (inspection, another compose, viterbi, generic kernels).
  int skip;
  // FAST variant, chain product with an epsilon-free partner: > 0 selects the time-windowed
  // bitmap layout with this many time slices (compose.hip); 0 = classic pair-indexed bitmaps
  int chain_bits;
  // FAST variant, chain products: != 0 leaves the stationary levels to launch_compose_replicate(), which must
  // follow on the same stream (ComposeOut::wr_* is the hand-over)
  int rep_grid;
  int Ncap, Acap;
  GTNX_G int* state;     // [N1*N2] pair -> INT_MIN unreachable / R / claim / node id
  GTNX_G int* queue;     // [N1*N2] backward-BFS queue of pair ids
  // outputs (SoA, arc-id order)
  GTNX_G int* src;
  GTNX_G int* dst;
  GTNX_G int* il;
  GTNX_G int* ol;
  GTNX_G float* w;
  GTNX_G int* gi1;       // gradInfo.first  (compose.cpp:443-446)
  GTNX_G int* gi2;       // gradInfo.second
  GTNX_G uint8_t* nflags;
  GTNX_G int* pair_of;   // [Ncap] composed node -> pair id
  GTNX_G int* out_off;   // [Ncap+1]
  GTNX_G int* level_off; // [Ncap+2]
  // in-CSR (filled by the transpose kernels)
  GTNX_G int* in_off;    // [Ncap+1]
  GTNX_G int* in_cursor; // [Ncap]
  GTNX_G int* in_list;   // [Acap]
  GTNX_G int* in_src;    // [Acap]
  GTNX_G float* in_w;    // [Acap]
  GTNX_G int* start_list;  // [Ncap]
  GTNX_G int* accept_list; // [Ncap]
  GTNX_G int* counts;      // [2] n_start, n_accept
  GTNX_G ComposeOut* out;
  // compose_pairs_kernel only: the lists it binary-searches, sorted on the matched label -- g1's out / in
  // records by olabel, g2's by ilabel (the graph's own records when it is sorted on that label, else a stable
  // sorted view made by launch_sorted_view); null for a side the matcher never searches
  int trim_fwd_first;  // compose_pairs_kernel: mark the pairs reached from the start pairs first (see the kernel)
  const GTNX_G gtnx_i4* s1_out;
  const GTNX_G gtnx_i4* s1_in;
  const GTNX_G gtnx_i4* s2_out;
  const GTNX_G gtnx_i4* s2_in;
};
// dyn_lds_bytes: 2 bitmaps of N1*N2 bits for the largest pair table of the batch
// when every graph has lds_state set, else 0
int compose_max_bitmap_bytes();
// bytes of the chain layout for a partner with `No` nodes and `slices` time slices
size_t compose_chain_bitmap_bytes(int No, int slices);
// all n problems share (matcher, g1 is linear, g2 is linear)
// fast != 0: the compact LDS-only variant (needs dyn_lds_bytes > 0); pairs it cannot
// handle come back with ComposeOut::overflow == 2 and must be re-run with fast = 0
// cache1 != 0 (fast only): g1's adjacency is cached in LDS; dyn_lds_bytes then
// covers the bitmaps plus compose_g1_cache_bytes() of the largest g1
size_t compose_g1_cache_bytes(int N1, int A1);
int compose_lds_budget(int wide);
// wide != 0 (fast chain products only): 512-lane workgroups, partners of up to 512 nodes
void launch_compose(const ComposeArgs* d_args, int n, int matcher, int lin1, int lin2, int dyn_lds_bytes,
                    int fast, int cache1, int wide, hipStream_t st);
// compose_wide.hip: chain products (exactly one side KIND_LINEAR, chain length >= 1) with an epsilon-free partner
// of at most compose_wide_node_cap() nodes whose arcs match in the partner's list order (see the file's header);
// any out-degree.  All n pairs share `lin2` (the chain is the second graph).  Leaves ComposeOut::csr_built = 0:
// launch_compose_transpose() follows.
// the stationary levels a FAST chain-product launch left out (ComposeArgs::rep_grid): arcs, in-rows, node
// arrays of levels wr_L + 1 .. wr_L + wr_K from level wr_L, with as many workgroups as the output deserves
void launch_compose_replicate(const ComposeArgs* d_args, int n, int lin2, int max_acap, hipStream_t st);
int compose_wide_node_cap();
void launch_compose_wide(const ComposeArgs* d_args, int n, int lin2, int max_acap, hipStream_t st);
// compose_wide.hip, general products (both graphs explicit, any degrees, epsilons allowed): a wave per frontier
// pair.  `state` must arrive filled with INT_MIN; s1_* / s2_* set for the side(s) `matcher` searches (UNSORTED
// searches g2 through its sorted view).  Leaves csr_built = 0.
void launch_compose_pairs(const ComposeArgs* d_args, int n, int matcher, hipStream_t st);
void launch_sorted_view(const DGraph& g, int key_olabel, void* out_view /* [A] 16-byte records */, void* in_view, hipStream_t st);
struct ComposeFillArgs {
  int N, A;
  const GTNX_G int* out_off;
  const GTNX_G int* dst;
  const GTNX_G float* w;
  const GTNX_G int* gi1;
  const GTNX_G int* gi2;
  const GTNX_G int* lab1;  // ilabels of input 1 (null: linear chain with C1 labels per step)
  const GTNX_G int* lab2;  // olabels of input 2
  int C1, C2;
  GTNX_G int* src;
  GTNX_G int* il;
  GTNX_G int* ol;
  GTNX_G int* in_cursor;   // [N] scratch, preset to in_off
  GTNX_G int* in_list;
  GTNX_G int* in_src;
  GTNX_G float* in_w;
};
void launch_compose_fill(const ComposeFillArgs& a, hipStream_t st);
size_t compose_transpose_scratch_bytes(int n, int maxNcap);
void launch_compose_transpose(const ComposeArgs* d_args, int n, int maxAcap, int maxNcap, void* scratch,
                              hipStream_t st);

// out_rec / in_rec (16 B * A each) for a device-built explicit graph
void launch_build_records(const DGraph& g, void* out_rec, void* in_rec, hipStream_t st);

struct ComposeGradArgs {
  const GTNX_G float* delta; // [A] grads of the composed arcs
  const GTNX_G int* gi1;
  const GTNX_G int* gi2;
  int A;
  int A1, A2;
  GTNX_G float* grad1; // nullptr when input 0 has calcGrad = false
  GTNX_G float* grad2;
};
void launch_compose_grad(const ComposeGradArgs* d_args, int n, int maxA, hipStream_t st);

// ---------------------------------------------------------------------------
// lazy chain products (lazy.hip): shortest distance / path / gradients over
// chain (T x C emissions) o G without building the product
// ---------------------------------------------------------------------------
struct LazyGroup {          // utterances that share one explicit graph G
  DGraph g;                 // G: CSR + packed records + weights
  int chain_first;          // compose(chain, G): match on G's ilabel; else on its olabel
  int T, C, N, nb;          // chain length / labels per step, |G| nodes, utterances
  int Npad, Cpad;           // LDS row strides (odd: 16 utterance rows hit 16 banks)
  // G's rows repacked for the time-step kernels: {other node, matched label or -1,
  // weight bits, arc id} in in-row / out-row order -- one 16-byte load per arc
  const gtnx_i4* lrec_in;
  const gtnx_i4* lrec_out;
  const float* const* em;   // [nb] chain weights, T*C each
  const float* em_base;     // ... or, when the chains are slices of one tensor at a constant stride (floats),
  int64_t em_stride;        //     em[b] == em_base + b * em_stride (null / 0: use the table)
  float* alpha;             // [T+1][nb][N]
  float* beta;              // [T+1][nb][N] (gradients only)
  int* bp;                  // [T+1][nb][N] back-pointers (arc of G), tropical only
  float* score;             // [nb]
  int* best;                // [nb] best accept node of G (-1: no path), tropical only
  const float* const* delta;  // [nb] upstream gradient of each score
  float* const* grad_em;      // [nb] chain gradient buffers (T*C) or null entries
  float* grad_fixed;          // [A] gradient of G's arcs (zero-filled) or null
  // dense regime (log semiring; every node's in-arcs share one matched label and G is
  // nearly complete): the recursion is a product with E = exp(w - cmax) in the
  // probability domain -- see lazy.hip "dense regime"
  const float* E;             // [N][N] row = source, col = destination (0: no arc)
  const float* cmax;          // [N] largest in-arc weight per destination (-inf: none)
  const int* nlab;            // [N] matched label of the node's in-arcs (-1: none)
  int lab_unique;             // no two nodes share a matched label (gradient rows need no atomics)
  int tie_by_node;            // maxplus_path_kernel: of equal maxima the one from the smallest SOURCE NODE (viterbiPath of
                              // a transitions graph whose layers the reference's queue visits in node order); 0: the
                              // first one in in-row order (the reference's in-list order: viterbiScore's gradient)
  float* amax;                // [T+1][nb] row max of alpha[t]   (written by the forward steps)
  float* bmax;                // [T][nb]   row max of em + beta[t+1] + cmax (backward steps)
  float* amaxp;               // [T+1][nb][ntp] the same, one partial per column tile (matrix-core form: reduced into
  float* bmaxp;               //                amax / bmax once a pass is through, launch_lazy_mfma_rowmax)
  int ntp;                    // partials per row: column tiles rounded up to 4
  float* R;                   // [N][N] sum over (t, utterance) of the arc posteriors / exp(w)
  // gradients: per (t, utterance) normaliser log sum_n exp(alpha[t+1][n] + beta[t+1][n]).  It
  // equals the total score exactly in exact arithmetic; in float32 the two sweeps drift apart
  // by a few ulps of |score| over T steps, and normalising each time step by its own sum keeps
  // every step's posterior mass at 1 (the standard alpha-beta remedy).  Null: use `score`.
  const float* zt;
  // matrix-core form of the dense regime (lazy.hip: lazy_mfma_*)
  float* xt[2];               // [Kpad / 4][nbpad][4] the contraction input, exponentiated, in operand layout (two planes)
  const float* Ep;            // [Kpad / 4][Npad2][4] E zero-padded
  const float* ETp;           // [Kpad / 4][Npad2][4] its transpose
  int Kpad, Npad2, nbpad;     // N rounded up to operand batches / to 32; nb rounded up to 32 (max-plus form: to 64)
  int rot;                    // leading nodes without a matched in-arc: the planes index nodes rotated by this many
  int rel;                    // alpha / beta / amax / bmax / zt are stored RELATIVE to per-row references (matrix-core form,
                              // lazy.hip "dense regime on the matrix cores"): alpha[t] against RA[t] = sum of amax[0 .. t-1]
  // max-plus form of the dense regime (tropical semiring; maxplus.hip): xt holds alpha itself
  const float* mp_Wq;         // [dblock][Kpad / 2][16][2] largest weight per (source, destination column), -inf: no arc
  const int* mp_colidx;       // [N] node -> destination column, -1 for nodes without a matched in-arc
  const int* mp_colnode;      // [mp_ncol] column -> node
  const int* mp_dead;         // [mp_ndead] the nodes without a matched in-arc
  int mp_ncol, mp_ndead;
};
size_t lazy_step_lds_bytes(const LazyGroup& g);
int lazy_tile_nodes();
int lazy_tile_batch();
void launch_lazy_pack(const LazyGroup& g, gtnx_i4* lrec_in, gtnx_i4* lrec_out, hipStream_t st);
void launch_lazy_init(const LazyGroup& g, int which, hipStream_t st);
void launch_lazy_step(const LazyGroup& g, int t, int mode, int backward, hipStream_t st);
void launch_lazy_final(const LazyGroup& g, int mode, hipStream_t st);
void launch_lazy_path(const LazyGroup& g, int* path_arc, int* path_il, int* path_ol, float* path_w, int* path_len,
                      hipStream_t st);
// node_label != null: every node's in-arcs share one matched label (no arc loop)
void launch_lazy_local_z(const LazyGroup& g, float* zt, hipStream_t st);  // [T][nb]
void launch_lazy_chain_grad(const LazyGroup& g, const int* node_label, hipStream_t st);
// local z + chain gradient in one pass (shared in-arc labels, N <= 1024): writes zt like launch_lazy_local_z
bool lazy_z_chain_grad_ok(const LazyGroup& g);
void launch_lazy_z_chain_grad(const LazyGroup& g, const int* node_label, float* zt, hipStream_t st);
void launch_lazy_fixed_grad(const LazyGroup& g, int max_in_deg, hipStream_t st);
struct LazyPathGrad {
  const float* delta;   // [len] (stride 1) or one scalar (stride 0)
  int delta_stride;
  const int* path_arc;  // [len] arcs of G, first-arc-first
  const int* il;
  const int* ol;
  int len, C, chain_first;
  float* grad_chain;    // [T*C] or null
  float* grad_fixed;    // [A] or null
};
void launch_lazy_path_grad(const LazyPathGrad& a, hipStream_t st);
// one workgroup per (chain, small G) pair: lazy_pair.hip
struct LazyPair {
  DGraph g;                    // G with packed records and weights
  const GTNX_G float* em;      // [T][C] chain weights
  GTNX_G float* alpha;         // [T+1][N]
  GTNX_G float* score;         // [1]
  const GTNX_G float* delta;   // [1] upstream gradient of the score   (backward)
  GTNX_G float* grad_em;       // [T][C] written completely, or null   (backward)
  GTNX_G float* grad_fixed;    // [A] zero-filled by the host, or null (backward)
  int T, C, chain_first, pad;
};
int lazy_pair_max_nodes();
int lazy_pair_max_degree();
int lazy_pair_block(int max_nodes);   // lanes per workgroup for a batch whose largest G has max_nodes
int lazy_pair_max_labels(int block);
// all pairs of one launch share C; cus: compute units of the device (workgroups are spread evenly)
void launch_lazy_pair_forward(const LazyPair* d_pairs, int n, int block, int C, int cus, hipStream_t st);
void launch_lazy_pair_backward(const LazyPair* d_pairs, int n, int block, int C, int cus, hipStream_t st);
// one workgroup per (chain, BANDED G) pair: band.hip.  G's arcs go from n to n, n+1 or n+2,
// at most one per (n, step), and all in-arcs of a node carry one matched label.
struct BandNode {
  int lab;     // matched label of the node's in-arcs (-1: no in-arc)
  int aid[3];  // arc id of the in-arc from n, n-1, n-2 (-1: none)
};
struct BandPair {
  const GTNX_G BandNode* nodes;    // [N]
  const GTNX_G uint8_t* nflags;    // [N] NF_START | NF_ACCEPT
  const GTNX_G int* snode;         // [n_lab] nodes with an in-arc, sorted by (label, node)
  const GTNX_G int* slab;          // [n_lab] their labels
  const GTNX_G float* w;           // G's weights, arc-id order; null: all zero
  const GTNX_G float* em;          // [T][C] chain weights
  GTNX_G float* em_copy;           // forward only, or null: every emission the sweep stages is also stored here (the
                                   // copy a region owes its emission graphs, region.cpp PendingCopy: one pass
                                   // over the caller's tensor instead of two)
  GTNX_G float* alpha;             // [T+1][NS] log2 units, shifted rows
  GTNX_G double* aoff;             // [0]: the score in log2 units; [1 + (r >> lgrn) * 4 + w]: shift of alpha row r, wave w
  GTNX_G float* score;             // [1]
  GTNX_G float* norm;              // [1] forwardScore of the chain itself, or null
  GTNX_G float* rowlse;            // [T] log2-sum-exp2 of every emission row, or null
  const GTNX_G float* delta;       // [1] upstream gradient of the score         (backward)
  const GTNX_G float* delta_norm;  // [1] upstream gradient of norm, or null     (backward)
  GTNX_G float* grad_em;           // [T][C] written completely, or null         (backward)
  GTNX_G float* grad_fixed;        // [A] zero-filled by the host, or null       (backward)
  int N, T, C, NS;
  int hot;                         // label shared by >= 8 nodes of G (CTC: blank), or -1
  int lgrn;                        // log2 of the rows per shift period of the forward launch
  int n_lab;
  int bidx;                        // the pair's index in its batch record (BandPatch)
  int64_t goff;                    // offset of G's arc gradients inside the batch's gradient block (BandPatch)
};
// A backward launch over the table the FORWARD launch left on the device: what differs between the two launches of a
// batch record -- where the upstream gradients are read and the gradients written -- travels by value with the launch,
// as bases the kernel offsets by the pair's index (one table upload, a 5 us launch of its own, less per step).
struct BandPatch {
  int on;                          // 0: the table is complete (every launch but a batch record's backward)
  int M;                           // rows of a chain (stride of rowlse)
  const GTNX_G float* delta;       // [n]
  const GTNX_G float* delta_norm;  // [n] or null
  GTNX_G float* rowlse;            // [n][M] or null
  GTNX_G float* grad_em;           // [n][A] or null
  GTNX_G float* grad_fixed;        // + goff, or null
  int64_t A;                       // arcs of a chain (stride of grad_em)
};
// viterbiScore / viterbiPath of chain o (banded G): one workgroup per pair (band.hip)
struct BandDecode {
  const GTNX_G BandNode* nodes;  // [N]
  const GTNX_G uint8_t* nflags;  // [N]
  const GTNX_G float* w;         // G's weights (natural log), arc-id order; null: all zero
  const GTNX_G float* em;        // [T][C]
  GTNX_G uint8_t* bp;            // which in-arc won (0: from n, 1: n-1, 2: n-2; 3: none): [T][NS] bytes, or 2 bits per
                                 // (time, node) packed per lane (band_viterbi_wave_kernel); T * NS + 512 bytes either way
  GTNX_G int* pnode;             // [T + 1] nodes of the best path
  GTNX_G int* path_arc;          // [T] arcs of G along it, first-arc-first
  GTNX_G int* path_lab;          // [T] matched labels
  GTNX_G float* path_w;          // [T] weights of the product's arcs
  GTNX_G int* path_len;          // [1] T, or -1 when no accepting path exists
  GTNX_G float* score;           // [1]
  GTNX_G int* tie;               // [1] an exact tie between finite candidates was seen
  // ranked launches only (exact ties of CTC-shaped targets decided without the lattice, ops_band.cpp tie_ranks):
  // of two equal candidates the one whose SOURCE node has the smaller rank_in wins, of two equal accept nodes the
  // one with the smaller rank_acc
  const GTNX_G int* rank_in;     // [N]
  const GTNX_G int* rank_acc;    // [N]
  int N, T, C, NS;
  int stage_floats, pad;         // LDS staging area of the launch (floats)
};
// ranked != 0: band_viterbi_wave_kernel's RANKED variant (needs the shapes the wave kernel takes: vec, C <= 2048)
void launch_band_viterbi(const BandDecode* d_pairs, int n, int stage_floats, int max_nodes, int max_labels, int vec,
                         hipStream_t st, int ranked = 0);
bool band_viterbi_wave_ok(int max_nodes, int max_labels, int vec);
// Forced alignment of chain o (CTC target acceptor), one wave per utterance (align.hip): the tropical recursion of
// band_viterbi_wave_kernel<NPL, RANKED = true> over the first T of the utterance's T_full emission rows, ties decided
// by the closed-form node ranks of ops_band.cpp (tie_ranks: blank below every label; p = leading strict ascents of the
// label sequence), and the frame labels / token indices written from the pointer chase straight into the caller's rows.
struct AlignArgs {
  const GTNX_G BandNode* nodes;  // [N] the target's band records (batch_ctc_targets)
  const GTNX_G uint8_t* nflags;  // [N]
  const GTNX_G float* em;        // [T_full][C], 16-byte aligned, C % 4 == 0
  GTNX_G unsigned* bp;           // back-pointer words: ceil(T * NPL / 16) rows of 64
  GTNX_G int* labels;            // [T_full] label of every frame, -1 from T on (and everywhere without a path)
  GTNX_G int* tokens;            // [T_full] index into the label sequence, -1 on blank frames; or null
  GTNX_G float* score;           // [1] or null
  int N, T, T_full, C;
  int p, pad;
};
int align_npl(int max_nodes);  // nodes per lane of a launch (1, 2, 4, 8)
// max_nodes <= 512, C <= 2048 and a multiple of 4, every em 16-byte aligned: band_align_ok
bool band_align_ok(int max_nodes, int max_labels, int vec);
void launch_band_align(const AlignArgs* d_args, int n, int max_nodes, hipStream_t st);
// Forced alignment of chain o (force-alignment acceptor o ASG transitions), one wave per utterance (asg_align.hip):
// the tropical recursion over the U + 1 nodes of batch_asg_force_align's band records -- two candidates per node, the
// self-loop (aid[0]) and the step from node n - 1 (aid[1]), weights from the batch's gathered `w` -- over the first T of
// the utterance's T_full emission rows; of two equal candidates the step wins (the reference's queue order); the frame
// labels / token indices (node - 1, never -1 inside a path) written from the pointer chase into the caller's rows.
struct AsgAlignArgs {
  const GTNX_G BandNode* nodes;  // [N = U + 1] the target's band records (batch_asg_force_align)
  const GTNX_G uint8_t* nflags;  // [N]
  const GTNX_G float* w;         // [2U] arc weights, arc-id order (BandNode.aid indexes it)
  const GTNX_G float* em;        // [T_full][C], 16-byte aligned, C % 4 == 0
  GTNX_G unsigned* bp;           // back-pointer words, 1 bit per (time, node): ceil(T * NPL / 32) rows of 64
  GTNX_G int* labels;            // [T_full] label of every frame, -1 from T on (and everywhere without a path)
  GTNX_G int* tokens;            // [T_full] index into the label sequence; or null
  GTNX_G float* score;           // [1] or null
  int N, T, T_full, C;
};
int asg_align_npl(int max_nodes);  // nodes per lane of a launch (1, 2, 4, 8)
int asg_align_max_labels();        // 2048
// max_nodes <= 512, C <= 2048 and a multiple of 4, every em 16-byte aligned: asg_align_ok
bool asg_align_ok(int max_nodes, int max_labels, int vec);
size_t asg_align_plane_bytes(int T, int npl);  // one utterance's back-pointer plane, sized by the LAUNCH's npl
void launch_asg_align(const AsgAlignArgs* d_args, int n, int max_nodes, hipStream_t st);
// ---------------------------------------------------------------------------
// rational.hip: clone / concat / closure / union_ (functions.cpp:66-223) built on the device
// ---------------------------------------------------------------------------
struct RationalSeg {      // one input graph's place in the output
  DGraph g;               // its device view, weights included (implicit chains: as ensure_device_batch fills it in)
  int node_off, arc_off;  // where its nodes / arcs start
  int conn_off;           // where the epsilon connectors INTO it (concat) / around it (closure) start
  int keep_start, keep_accept;
  int pad;
};
struct RationalOut {
  int N, A;
  GTNX_G int* src;
  GTNX_G int* dst;
  GTNX_G int* il;
  GTNX_G int* ol;
  GTNX_G float* w;
  GTNX_G uint8_t* nflags;
  GTNX_G int* start_list;
  GTNX_G int* accept_list;
  GTNX_G int* out_off;
  GTNX_G int* out_list;
  GTNX_G int* in_off;
  GTNX_G int* in_list;
};
size_t rational_csr_temp_bytes(int N, int A);
// projection: 0 none, 1 input, 2 output (functions.h Projection); closure != 0: node 0 is the new start / accept node
void launch_rational_build(const RationalSeg* d_segs, int nseg, int max_A, int max_N, int max_conn, const RationalOut& out,
                           int projection, int closure, void* temp, hipStream_t st);
void launch_rational_adjacency(const RationalOut& out, void* temp, hipStream_t st);
// remove (functions.cpp:253-318): kept nodes = start nodes and nodes with an in-arc that does not carry the removed
// label pair; per kept node the reference's breadth-first walk over the removed arcs (queue order, out-list order),
// one lane per kept node, in batches of `rows` nodes that share the stamp / queue scratch
struct RemoveArgs {
  DGraph g;                 // explicit, adjacency resident
  int ilabel, olabel;
  const GTNX_G int* new_id;  // [N] kept node -> its id in the result (exclusive scan of the keep flags)
  const GTNX_G int* roots;   // [K] result node -> node of g
  int K, root0, rows;
  GTNX_G int* stamp;         // [rows][N], zero before the first batch
  GTNX_G int* queue;         // [rows][N]
  GTNX_G int* arc_cnt;       // [K] (count pass)
  const GTNX_G int* arc_off; // [K + 1] (emit pass)
  RationalOut out;
};
void launch_remove_keep(const DGraph& g, int ilabel, int olabel, int* keep, hipStream_t st);
void launch_remove_roots(const int* keep, const int* new_id, int N, int* roots, hipStream_t st);
void launch_remove_walk(const RemoveArgs& a, bool emit, hipStream_t st);
size_t scan_temp_bytes(int n);
void launch_exclusive_scan(const int* in, int* out, int n, void* temp, size_t temp_bytes, hipStream_t st);
// the binary graph format's arc table ({src, dst, ilabel, olabel} x A, 16-byte aligned), weights and node flags, all
// on the device, into a structure's arrays + adjacency (the device side of gtnx_graph_load_buffer)
void launch_rational_load(const void* rows, const float* w, const uint8_t* flags, const RationalOut& out, void* temp,
                          hipStream_t st);
// one CTC target acceptor per label sequence, written as band records on the device (band.hip)
struct CtcTargetArgs {
  const GTNX_G int* labels;   // [U]
  GTNX_G BandNode* nodes;     // [N = 2U + 1]
  GTNX_G uint8_t* nflags;     // [N]
  GTNX_G int* snode;          // [N]
  GTNX_G int* slab;           // [N]
  GTNX_G int* n_arcs;         // [1] or null
  int N, pad;
};
void launch_ctc_targets(const CtcTargetArgs* d_args, int n, int blank, hipStream_t st);
// One CTC criterion step of a batch in ONE launch (ctc_step.hip): workgroup b builds utterance b's target records, runs
// both band sweeps and writes loss_b in between.  Travels BY VALUE with the launch: every per-utterance address is a
// base + b * a stride sized by the batch's largest target, so no table is uploaded.
struct CtcStepDesc {
  const GTNX_G int* stage;    // PINNED HOST memory, read in place: [n] entries {label offset, U, rows, arc-gradient offset}
  const GTNX_G int* labels;   // PINNED HOST memory: the label sequences back to back
  const GTNX_G float* em;     // [n][T][C]
  GTNX_G float* grad;         // [n][T][C], every row written
  GTNX_G float* loss;         // [n]
  GTNX_G float* tgrad;        // the targets' arc gradients, utterance b's at its entry's offset; null: not wanted
  GTNX_G char* rec;           // band records: per utterance nodes | flags (+ o_flags) | snode (+ o_snode) | slab (+ o_slab)
  GTNX_G float* alpha;        // [n] planes of [T + 1][NS_b] floats
  GTNX_G double* aoff;        // [n] x (4 T + 16) doubles: score and row shifts (BandPair::aoff)
  GTNX_G float* rowlse;       // [n][T]
  GTNX_G float* score;        // [n]
  GTNX_G float* norm;         // [n]
  int64_t em_stride, rec_stride, alpha_stride, aoff_stride;  // in elements of the array (rec: bytes)
  int o_flags, o_snode, o_slab;
  int T, C, blank, lgrn;
};
int band_block_rows(int C, int max_NS, bool backward);
bool ctc_step_cell(int C, int max_NS);  // is there an instantiated cell for rows of C labels and targets of max_NS (row stride) nodes?
void launch_ctc_step(const CtcStepDesc& d, int n, int max_NS, bool gradg, hipStream_t st);
// one force-alignment acceptor o transitions per label sequence (examples/asg.cpp:50-68), as band records
struct AsgFalArgs {
  const GTNX_G int* labels;      // [U]
  const GTNX_G float* trans_w;   // weights of the transitions graph, asgTransitions arc layout
  GTNX_G BandNode* nodes;        // [U + 1]
  GTNX_G uint8_t* nflags;        // [U + 1]
  GTNX_G int* snode;             // [U]
  GTNX_G int* slab;              // [U]
  GTNX_G float* w;               // [2U] arc weights (gathered)
  GTNX_G int* arc_map;           // [2U] transitions arc of every arc
  int U, pad;
};
void launch_asg_fal_targets(const AsgFalArgs* d_args, int n, int n_labels, hipStream_t st);
void launch_asg_fal_scatter(const float* g, const int* maps, const int64_t* tab /* 3 per sequence */, int n_seq, int64_t longest,
                            float* trans_grad, hipStream_t st);
int band_max_nodes();
int band_max_labels();
int band_min_labels();
int band_npl(int max_nodes);               // nodes per lane: 1 or 2
int band_row_stride(int N, int npl);       // NS
int band_forward_lgrn(int C);
// all pairs of one launch share C and npl; unit: self-loop + previous-node arc at every node, all weights 0;
// vec: C % 4 == 0 and every pair's emissions are 16-byte aligned (16-byte staging loads)
// `one` (HOST memory; a launch of one pair for which band_one_ok holds): the record travels as the kernel's own argument
// and d_pairs is not read
bool band_one_ok(int npl, int C, int max_NS, bool vec, bool backward);
void launch_band_forward(const BandPair* d_pairs, int n, int npl, int C, int max_NS, bool unit, bool vec, hipStream_t st,
                         const BandPair* one = nullptr);
// patch (optional; not with `one`): d_pairs is the table a FORWARD launch used -- see BandPatch
void launch_band_backward(const BandPair* d_pairs, int n, int npl, int C, int max_NS, bool unit, bool gradg, bool vec,
                          hipStream_t st, const BandPair* one = nullptr, const BandPatch* patch = nullptr);
// dense regime
void launch_lazy_dense_prep(const LazyGroup& g, float* E, float* cmax, hipStream_t st);  // nlab must be set
// backward: vin / vout = the two halves of a [2][nb][N] scratch (vin null on the first step)
void launch_lazy_dense_step(const LazyGroup& g, int t, int backward, hipStream_t st, const float* vin = nullptr,
                            float* vout = nullptr);
void launch_lazy_dense_fixed_grad(const LazyGroup& g, hipStream_t st);                   // R zero-filled
size_t maxplus_w_floats(const LazyGroup& g);                                   // mp_ncol / Kpad set
void launch_maxplus_prep(const LazyGroup& g, hipStream_t st);                  // mp_Wq, both input planes
void launch_maxplus_step(const LazyGroup& g, int t, hipStream_t st);           // alpha[t] -> alpha[t+1]
void launch_maxplus_path(const LazyGroup& g, int* path_arc, int* path_il, int* path_ol, float* path_w, int* path_len,
                         hipStream_t st);
// asg_decode.hip: the decode of every utterance of a max-plus group at its own length, results on the device -- one
// wave per utterance walks back from row d_frames[b] (device, [nb], 0 .. g.T) of the alpha planes the sweeps above
// filled for t = 0 .. g.T: labels[b * row_stride + t] the label of frame t (-1 from d_frames[b] to g.T), scores[b] the
// best accept score of that row (or null), collapsed[b * row_stride + ..] the labels with runs merged, -1 up to g.T
// (or null), lengths[b] how many (or null).  Ties: first accept node in accept_list order, smallest source node.
// No accepting path: entries -1, score -inf, length 0.  Nothing past row d_frames[b] is read.
void launch_asg_decode(const LazyGroup& g, const int* d_frames, int* labels, int64_t row_stride, float* scores,
                       int* collapsed, int* lengths, hipStream_t st);
void launch_lazy_mfma_prep(const LazyGroup& g, hipStream_t st);                // Ep / ETp from E
void launch_lazy_mfma_init(const LazyGroup& g, int which, hipStream_t st);     // keys, first input (0 forward, 1 backward)
void launch_lazy_mfma_step(const LazyGroup& g, int t, int backward, hipStream_t st);
// the whole pass (steps 0 .. T-1, or T-1 .. 0) as ONE cooperative launch: workgroups of a row tile hand their
// step's output to each other through agent-scope stores / loads and a counter; false when not applicable
size_t lazy_mfma_chain_sync_ints(const LazyGroup& g);
bool launch_lazy_mfma_chain(const LazyGroup& g, int backward, int* zeroed_sync, int cus, hipStream_t st);
void launch_lazy_mfma_keys(float* keys, int64_t n, hipStream_t st);            // order-preserving integer keys -> floats
void launch_lazy_mfma_rowmax(const LazyGroup& g, int which, hipStream_t st);   // amaxp -> amax (0) / bmaxp -> bmax (1)
void launch_lazy_mfma_score(const LazyGroup& g, hipStream_t st);               // score (relative, lazy_final) += sum of amax, float64
// R zero-filled.  partials: scratch of lazy_mfma_fixed_grad_scratch_bytes(g) bytes or null (then the blocks meet in R by atomics)
size_t lazy_mfma_fixed_grad_scratch_bytes(const LazyGroup& g);
void launch_lazy_mfma_fixed_grad(const LazyGroup& g, void* pair_consts /* 16 B x T x nb */, hipStream_t st, void* partials = nullptr,
                                 size_t partials_bytes = 0);

// ---------------------------------------------------------------------------
// small elementwise helpers
// ---------------------------------------------------------------------------
void launch_fill_i32(int* p, int v, size_t n, hipStream_t st);
void launch_fill_f32(float* p, float v, size_t n, hipStream_t st);
void launch_scalar_seed(float* root, float* g0, float s0, int acc0, float* g1, float s1, int acc1, size_t n, hipStream_t st);
// out[i] = sa * a[i] + sb * b[i]  over n scalars held at arbitrary addresses
struct ScalarArgs {
  const GTNX_G float* a;
  const GTNX_G float* b; // may be nullptr
  GTNX_G float* out;
  GTNX_G float* mirror;  // pinned host memory that gets the value too, or nullptr (runtime.h: mirror_slot)
};
void launch_scalar_combine(const ScalarArgs* d_args, int n, float sa, float sb, hipStream_t st);
void launch_copy_small(void* dst, const void* src, size_t bytes, hipStream_t st);  // src: device or pinned host memory
void launch_scalar_combine_one(const ScalarArgs& a, float sa, float sb, hipStream_t st);  // the record as a kernel argument
// o0[i] = s0 * d[i], o1[i] = s1 * d[i] (o1 may be null); seed != null: d is 1 and is written to *seed
struct ScalarFanArgs {
  const GTNX_G float* d;
  GTNX_G float* seed;
  GTNX_G float* o0;
  GTNX_G float* o1;
};
void launch_scalar_fan(const ScalarFanArgs* d_args, int n, float s0, float s1, hipStream_t st);
void launch_scalar_fan_one(const ScalarFanArgs& a, float s0, float s1, hipStream_t st);
// dst[i] += src[i] for a batch of vectors (atomic when dst's may repeat)
struct AxpyArgs {
  GTNX_G float* dst;
  const GTNX_G float* src;
  int64_t n;
  float scale;
};
void launch_axpy_batch(const AxpyArgs* d_args, int n, int64_t maxn, int atomic, hipStream_t st);
// dst[0 .. bytes) = src[0 .. bytes) for a batch of segments (16-byte accesses where both ends allow it)
struct CopySeg {
  void* dst;
  const void* src;
  int64_t bytes;  // a multiple of 4
};
void launch_copy_segments(const CopySeg* d_segs, int n, int64_t max_bytes, hipStream_t st);
// gather n scalars at arbitrary addresses into a dense array
void launch_gather_scalars(const float* const* d_ptrs, float* out, int n, hipStream_t st);
// out[i] = (accumulate ? out[i] : 0) + sa * a[i] + sb * b[i]  (b may be null) -- dense vectors of a batch record
void launch_vec_axpby(float* out, const float* a, const float* b, size_t n, float sa, float sb, int accumulate, hipStream_t st);
// viterbiPath grad: grad[arcs[a]] += delta[a]
struct ScatterArgs {
  const GTNX_G int* idx;
  const GTNX_G float* delta;
  GTNX_G float* grad;
  int n;
};
void launch_scatter_add(const ScatterArgs* d_args, int n, int maxn, hipStream_t st);
// zeros for the pad rows of a ragged [n][M][C] tensor (padfill.hip): element b's floats [rows[b] * C, M * C) at
// base + (offs ? offs[b] : b * stride); prefix[b] = sum over b' < b of (M - rows[b']) * C, prefix[n] the total
struct PadFillArgs {
  GTNX_G float* base;
  const GTNX_G int64_t* offs;    // [n] float offsets of the elements, or nullptr: b * stride
  const GTNX_G int* rows;        // [n]
  const GTNX_G int64_t* prefix;  // [n + 1]
  int64_t stride;
  int n, C;
};
void launch_pad_fill(const PadFillArgs& a, int64_t total_floats, hipStream_t st);
// asg_full.hip: forwardScore(linearGraph(T_b, N) o asgTransitions(N)) of every utterance of a padded [n][M][N] tensor at
// its own length and the gradient of those scores, one workgroup per utterance, one launch each way.  w: the transitions
// weights in arc-id order (w[0 .. N) the start scores, w[N + i * N + j] the score of j -> i).  Forward: score[b]; with
// la / L / zd set it also stores what the backward launch re-reads (la [n][M][N]: alpha_t[i] minus the step's running
// scale, L [n][M]: that scale, zd [n]: the score in float64).  Backward (seed delta[b]): rows < rows[b] of grad_em
// (or null) are OVERWRITTEN with delta * gamma, and partial (or null) [n][N + N * N] receives every utterance's
// share of the transitions gradient, arc-id order; launch_asg_full_reduce adds the shares in utterance order (no
// atomics).  Rows >= rows[b] of em, la and grad_em are never addressed.  A score of -inf: zeros.  1 <= N <=
// asg_full_max_labels().
struct AsgFullArgs {
  const GTNX_G float* em;     // [n][M][N]
  const GTNX_G int* rows;     // [n], 1 .. M, or nullptr: M
  const GTNX_G float* w;      // [N + N * N]
  GTNX_G float* score;        // [n]
  GTNX_G float* la;           // [n][M][N] or nullptr (forward only: nothing kept for a gradient)
  GTNX_G double* L;           // [n][M]
  GTNX_G double* zd;          // [n]
  const GTNX_G float* delta;  // [n] (backward)
  GTNX_G float* grad_em;      // [n][M][N] or nullptr
  GTNX_G float* partial;      // [n][N + N * N] or nullptr
  int n, M, N;
};
int asg_full_max_labels();  // 128
void launch_asg_full_forward(const AsgFullArgs& a, hipStream_t st);
void launch_asg_full_backward(const AsgFullArgs& a, hipStream_t st);
void launch_asg_full_reduce(const float* partial, int n, int N, float* out, hipStream_t st);
// linear_decode.hip: viterbiPath of every chain of an [n][M][C] tensor at its own length frames[b] (device, 0 .. M),
// then the CTC collapse, results on the device.  labels[b * row_stride + t] = the first label holding the maximum of
// row t (-1 from frames[b] to M); scores[b] (or null) = ((0 + m_0) + m_1) + ... in frame order; collapsed[b *
// row_stride + k] (or null) the labels with repeats merged and `blank` dropped (blank < 0: nothing dropped), starts
// likewise (or null; needs collapsed) the first frame of each, both -1 from lengths[b] (or null) to M.  A row without
// an entry above -inf, or frames[b] = 0: no path -- every entry of every row -1, score -inf, length 0.  rowmax: [n][M] floats of
// scratch.  Nothing from row frames[b] on is read.  Two launches: which = 0 the rows (label and maximum of every
// row), which = 1 one wave per utterance (score, collapse, the -1 entries).
struct LinearDecodeArgs {
  const GTNX_G float* em;
  const GTNX_G int* frames;  // [n]
  GTNX_G int* labels;
  GTNX_G float* rowmax;      // [n][M]
  GTNX_G float* scores;
  GTNX_G int* collapsed;
  GTNX_G int* starts;
  GTNX_G int* lengths;
  int64_t row_stride;
  int n, M, C, blank;
};
void launch_linear_decode(const LinearDecodeArgs& a, int which, hipStream_t st);
// ctc_sample.hip: N alignments of every chain of an [n][M][C] tensor drawn from its frame posteriors at its own length
// frames[b] (device, 0 .. M), then the CTC collapse, results on the device (the contract: DESIGN section 32).  Frame t
// of sample k of utterance b0 + b takes label c with probability exp(x[c] / temperature) / Z over the finite entries,
// by inverse CDF in label order against u = (2 * (word >> 9) + 1) * 2^-24, word = output (k & 3) of Philox4x32-10 with
// key (seed_lo, seed_hi) and counter (t, b0 + b, k >> 2, 0).  which = 0: the rows -- labels[(b * N + k) * label_stride
// + t] and terms[(b * N + k) * M + t] = x[c] / temperature - log Z; a row without a finite entry: label -1.
// which = 1: one wave per (b, k) -- logq[b * N + k] (or null) = the terms added in frame order from 0, tokens[(b * N +
// k) * row_stride + i] the labels with repeats merged and `blank` dropped (blank < 0: nothing dropped), -1 from
// lengths[b * N + k] to M, the labels -1 from frames[b] to M when fill_labels is set (they are the caller's).  A label
// of -1 below frames[b], or frames[b] = 0: no path -- -1 rows, length 0, logq -inf.  Nothing from row frames[b] on is
// read.  N 1 .. 1024, temperature finite and > 0 (the engine has refused the rest).
constexpr int kCtcSampleMaxN = 1024;
struct CtcSampleArgs {
  const GTNX_G float* em;
  const GTNX_G int* frames;  // [n]
  GTNX_G int* labels;        // [n][N][label_stride]: the caller's rows, or scratch with label_stride = M
  GTNX_G float* terms;       // [n][N][M] of scratch
  GTNX_G int* tokens;
  GTNX_G int* lengths;
  GTNX_G float* logq;
  int64_t row_stride, label_stride;
  int n, M, C, blank, N, b0, fill_labels;
  unsigned seed_lo, seed_hi;
  float temperature;
};
void launch_ctc_sample(const CtcSampleArgs& a, int which, hipStream_t st);
// asg_sample.hip: N alignments of every chain of an [n][M][C] tensor drawn from the posterior of emissions o
// transitions at its own length frames[b] (device, 0 .. M) by forward filtering, backward sampling, then the merge of
// equal neighbours, results on the device (the contract: DESIGN section 34).  table [C + C * C]: start scores, then
// table[C + i * C + j] = the score of moving from label j to label i.  which = 0 (C > kAsgSampleRegisterC only, once per
// call): rmax [stride] and et [roundup4(C)][stride] = exp(table / temperature - rowmax) transposed, stride =
// asg_sample_et_stride(C), pads zero.  which = 1: the filter -- planes[(b * M + t) * C + i] = alpha_t[i] minus the
// running reference, -inf without mass, and logz[b] (or null) = logZ, -inf without a path.  which = 2: the draw, one
// wave per (b, k), from frames[b] - 1 down, against u = (2 * (word >> 9) + 1) * 2^-24, word = output (k & 3) of
// Philox4x32-10 with key (seed_lo, seed_hi) and counter (t, b0 + b, k >> 2, 1) -- labels[(b * N + k) * label_stride +
// t] and terms[(b * N + k) * M + (frames[b] - 1 - t)] = log(mass / total) of the drawn label; an utterance without a
// path: labels -1.  which = 3: one wave per (b, k) -- logq[b * N + k] (or null) = the terms added in draw order from
// 0, tokens[(b * N + k) * row_stride + i] the labels with equal neighbours merged, -1 from lengths[b * N + k] to M,
// the labels -1 from frames[b] to M when fill_labels is set (they are the caller's).  A label of -1 below frames[b], or
// frames[b] = 0: no path -- -1 rows, length 0, logq -inf.  Nothing from row frames[b] on is read.  N 1 .. 1024, C 1 ..
// 1024, temperature finite and > 0 (the engine has refused the rest).
constexpr int kAsgSampleMaxN = 1024;
constexpr int kAsgSampleMaxC = 1024;
constexpr int kAsgSampleRegisterC = 128;  // up to here the filter keeps the transitions in registers
struct AsgSampleArgs {
  const GTNX_G float* em;
  const GTNX_G int* frames;    // [n]
  const GTNX_G float* table;   // [C + C * C]
  GTNX_G float* planes;        // [n][M][C] of scratch
  GTNX_G float* et;            // [roundup4(C)][stride] of scratch (C > kAsgSampleRegisterC)
  GTNX_G float* rmax;          // [stride] of scratch (C > kAsgSampleRegisterC)
  GTNX_G int* labels;          // [n][N][label_stride]: the caller's rows, or scratch with label_stride = M
  GTNX_G float* terms;         // [n][N][M] of scratch
  GTNX_G int* tokens;
  GTNX_G int* lengths;
  GTNX_G float* logq;
  GTNX_G float* logz;
  int64_t row_stride, label_stride;
  int n, M, C, N, b0, fill_labels;
  unsigned seed_lo, seed_hi;
  float temperature;
};
int asg_sample_et_stride(int C);  // 0 up to kAsgSampleRegisterC labels
void launch_asg_sample(const AsgSampleArgs& a, int which, hipStream_t st);
// ctc_beam.hip: CTC prefix beam search with N-best output over every chain of an [n][M][C] tensor at its own length
// frames[b] (device, 0 .. M), results on the device (the contract: DESIGN section 20).  which = 0: the rows -- the
// token set S_t of every row that counts, (value, label) entries [n][M][topn + 1] and their counts [n][M] in scratch.
// which = 1: one workgroup per utterance, sequential over the frames -- at most `beam` prefixes with (pb, pnb), exact
// prefix identity through the trie in scratch (node 1 + t * beam + slot = (parent node, label), node 0 the empty
// prefix), then tokens[(b * nbest + r) * row_stride + k] (-1 from the length to M), lengths[b * nbest + r],
// scores[b * nbest + r]; slots without a hypothesis: -1, 0, -inf.  Nothing from row frames[b] on is read.
// beam 1 .. 64, topn 1 .. 32, nbest 1 .. beam, C <= 2^25, M * beam < 2^31 (the engine has refused the rest).
struct CtcBeamArgs {
  const GTNX_G float* em;
  const GTNX_G int* frames;  // [n]
  GTNX_G float* ent_val;     // [n][M][topn + 1], interleaved with ent_lab as 8-byte entries: see ctc_beam.hip
  GTNX_G int* ent_cnt;       // [n][M]
  GTNX_G int* trie;          // [n][M * beam + 1][2]
  GTNX_G int* tokens;
  GTNX_G int* lengths;
  GTNX_G float* scores;
  int64_t row_stride;
  int n, M, C, blank, beam, topn, nbest;
  // the bigram table, or null: [C + C * C], w[c] = c as first label, w[C + i * C + j] = j followed
  // by i.  With it candidates rank by acoustic total + L, L(prefix) = sum of lm_weight * w + lm_bonus, an extension
  // with a non-finite term is dropped, scores holds acoustic + L and am_scores (may be null) the acoustic total alone.
  // C <= 2^19 with a table (the engine has refused the rest).
  const GTNX_G float* lm;
  float lm_weight, lm_bonus;
  GTNX_G float* am_scores;
  // the compiled LM graph (lm_graph.h has the layout), or null; never together with `lm`.  One
  // array of 16-byte words: two per state, [0, 2 * lmg_states), then one per arc.  A prefix then also carries its state,
  // the term of an extension is lm_weight * walk(state, label) + lm_bonus, and everything else is as with the table.
  const GTNX_G gtnx_i4* lmg;
  int lmg_states, lmg_start;
};
void launch_ctc_beam(const CtcBeamArgs& a, int which, hipStream_t st);
// asg_beam.hip: ASG prefix beam search with N-best output over every chain of an [n][M][C] tensor at its own length
// frames[b] (device, 0 .. M), results on the device (the contract: DESIGN section 27).  The hypotheses are the label
// sequences without equal neighbours, each summed over its alignments under emissions o transitions.  table: [C + C * C]
// in the arc order of asgTransitions, entry c = start[c], entry C + i * C + j = label j followed by label i; an entry
// that is not finite forbids its candidates.  which = 0: the rows -- the token set S_t of every row that counts (its
// topn best labels, no blank), (value, label) entries [n][M][topn] and their counts [n][M] in scratch.  which = 1: one
// workgroup per utterance, sequential over the frames -- at most `beam` prefixes with one score each, exact prefix
// identity through the trie in scratch (node 1 + t * beam + slot = (parent node, label), node 0 the empty prefix), then
// tokens[(b * nbest + r) * row_stride + k] (-1 from the length to M), lengths[b * nbest + r], scores[b * nbest + r];
// slots without a hypothesis: -1, 0, -inf.  Nothing from row frames[b] on is read.
// beam 1 .. 64, topn 1 .. 32, nbest 1 .. beam, C <= 2^19, M * beam < 2^31 (the engine has refused the rest).
struct AsgBeamArgs {
  const GTNX_G float* em;
  const GTNX_G int* frames;    // [n]
  const GTNX_G float* table;   // [C + C * C]
  GTNX_G float* ent_val;       // [n][M][topn], interleaved with the labels as 8-byte entries: see beam_common.h
  GTNX_G int* ent_cnt;         // [n][M]
  GTNX_G int* trie;            // [n][M * beam + 1][2]
  GTNX_G int* tokens;
  GTNX_G int* lengths;
  GTNX_G float* scores;
  int64_t row_stride;
  int n, M, C, beam, topn, nbest;
  // the compiled LM graph (lm_graph.h has the layout), or null: the words, two per state in
  // [0, 2 * lmg_states), then one per arc.  With it a prefix also carries L and its LM state, an extension adds
  // lm_weight * walk(state, label) + lm_bonus to L, candidates rank by acoustic score + L, scores holds acoustic + L and
  // am_scores (may be null) the acoustic score alone.  which = 1 then launches the graph instantiation.
  const GTNX_G gtnx_i4* lmg;
  int lmg_states, lmg_start;
  float lm_weight, lm_bonus;
  GTNX_G float* am_scores;
};
void launch_asg_beam(const AsgBeamArgs& a, int which, hipStream_t st);
// edit_distance.hip: Levenshtein distance (unit costs) of the pairs pair0 .. pair0 + count - 1, pair p = b * N + k being
// (hyp + p * hyp_stride, hyp_len[p]) against (ref + b * ref_stride, ref_len[b]) -- one launch, one wave per pair, Myers'
// bit-vector recurrence in Hyyro's block form with the wave as the 64-bit word (the contract: DESIGN section 21).
// Lengths are device memory, clamped to 0 .. L / 0 .. U by the kernel; nothing at or past a clamped length is read.
// dist[p]; with ops non-null also ops[3 p ..] = (substitutions, deletions, insertions) of the walk back that prefers
// diagonal, then up, then left, from (Pv, Mv) of every (column, block) kept in scratch: 16 bytes * count * L * nbU.
// L <= kEditDistanceMaxL, U <= kEditDistanceMaxU (one block per lane; the engine has refused the rest).
constexpr int kEditDistanceMaxL = 65536;
constexpr int kEditDistanceMaxU = 4096;
typedef unsigned long long gtnx_ul2 __attribute__((ext_vector_type(2)));
struct EditDistanceArgs {
  const GTNX_G int* hyp;
  const GTNX_G int* hyp_len;  // [pairs]
  const GTNX_G int* ref;
  const GTNX_G int* ref_len;  // [pairs / N]
  GTNX_G int* dist;           // [pairs]
  GTNX_G int* ops;            // [pairs][3] or null
  GTNX_G gtnx_ul2* scratch;   // [count][L][nbU], with ops only
  int64_t hyp_stride, ref_stride;
  int64_t pair0;
  int count, N, L, U, nbU;
};
void launch_edit_distance(const EditDistanceArgs& a, hipStream_t st);
// ctc_score.hip: the log score forwardScore(ctcGraph(y) o emissions_b[:T_b]) of the pairs pair0 .. pair0 + count - 1,
// pair p = b * N + k being the hypothesis y = tokens[p * row_stride .. + clamp(lengths[p], 0, L)) of utterance b, and
// the gradient sum_k weights[p] * d score[p] / d emissions_b (the contract: DESIGN section 22).
//   forward:  one workgroup per pair; scores[p - score0] = the score (-inf: no path, length > U, a token outside
//             0 .. C - 1, T_b == 0).  With `alpha` non-null the alpha row of every frame also goes to
//             alpha[(p - pair0) * pair_stride + t * (2 U + 1) + s].
//   backward: one workgroup per utterance of the range walks its pairs of the range in k order: beta in LDS, the
//             occupancies exp(alpha + beta - score) summed per label in a fixed order and added into grad[b][t][label]
//             by plain loads and stores (no atomics).  The workgroup that holds k == 0 zeroes grad[b] first.
// The workgroup's width and the states per lane are chosen from 2 U + 1 alone (ctc_score_config).
constexpr int kCtcScoreMaxU = 4096;
struct CtcScoreArgs {
  const GTNX_G float* em;       // [n][M][C]
  const GTNX_G int* frames;     // [n]
  const GTNX_G int* tokens;     // pair p's row at tokens + p * row_stride
  const GTNX_G int* lengths;    // [pairs]
  GTNX_G float* scores;         // [.. - score0]
  GTNX_G float* alpha;          // [count][pair_stride] or null (forward); backward turns it into occupancies
  const GTNX_G float* weights;  // [pairs] (backward)
  GTNX_G float* grad;           // [n][M][C] (backward)
  int64_t row_stride, pair0, score0, pair_stride;
  int count, N, L, U, M, C, blank;
};
void ctc_score_config(int U, int* width, int* per_lane);  // the workgroup's width and the states a lane owns
void launch_ctc_score_forward(const CtcScoreArgs& a, hipStream_t st);
void launch_ctc_score_backward(const CtcScoreArgs& a, hipStream_t st);
// ctc_lattice.hip: the log score forwardScore(ctcAlignmentGraph(lattice_b) o emissions_b[:T_b]) of the utterances utt0 ..
// utt0 + count - 1, each with one acyclic token lattice of its own in device memory, and the gradients g[b] * d score[b] /
// d (emissions_b, arc weights of b) (the contract: DESIGN section 35).  Utterance b: K = num_nodes[b] nodes, the arcs
// arcs[b * row_stride + 3 a ..] = (src, dst, label), a < clamp(num_arcs[b], 0, A), dst-sorted, arc_weights[b * A + a].
//   forward:  one workgroup per utterance; scores[b - score0] = the score (-inf: T_b == 0, K < 1, K + arcs > SM, an arc
//             that is none, a weight that is +inf or NaN, no alignment).  With `alpha` non-null the alpha row of every
//             frame also goes to alpha[(b - utt0) * utt_stride + t * SM + s].
//   backward: one workgroup per utterance zeroes grad[b] (and arc_grad[b] if asked for), then writes weights[b] times the
//             occupancies summed per label in a fixed order by plain stores, and the arcs' posteriors.
// The workgroup's width and the states per lane are chosen from SM = max_states alone (ctc_lattice_config).
constexpr int kCtcLatticeMaxStates = 4096;
struct CtcLatticeArgs {
  const GTNX_G float* em;           // [n][M][C]
  const GTNX_G int* frames;         // [n]
  const GTNX_G int* arcs;           // utterance b's row at arcs + b * row_stride
  const GTNX_G int* num_arcs;       // [n]
  const GTNX_G int* num_nodes;      // [n]
  const GTNX_G float* arc_weights;  // [n][A] or null: all zeros
  GTNX_G float* scores;             // [.. - score0]
  GTNX_G float* alpha;              // [count][utt_stride] or null (forward)
  const GTNX_G float* weights;      // [n] (backward)
  GTNX_G float* grad;               // [n][M][C] (backward)
  GTNX_G float* arc_grad;           // [n][A] or null (backward)
  int64_t row_stride, utt_stride;
  int utt0, score0, count, A, SM, M, C, blank;
};
void ctc_lattice_config(int max_states, int* width, int* per_lane);  // the workgroup's width, the states a lane owns
void launch_ctc_lattice_forward(const CtcLatticeArgs& a, hipStream_t st);
void launch_ctc_lattice_backward(const CtcLatticeArgs& a, hipStream_t st);
// ctc_lattice_align.hip: the best (lattice path, alignment) pair (max-plus, of equal candidates the first in the
// forward's order) of the utterances utt0 .. utt0 + count - 1 in ctc_lattice.hip's lattice form (the contract: DESIGN
// section 38).  One workgroup per utterance, width and states per lane from ctc_lattice_config(SM); row b of every
// output is written over its whole width: scores[b] the pair's score, path_len[b] the arcs on the path, path_arcs /
// path_tokens / starts / ends [b * out_stride + i] the i-th arc, its label, its first frame and one past its last (the
// first P of a longer path), token_scores (or null) the arc's emissions summed in frame order, frame_arcs[b *
// frame_stride + t] (or null) the arc of frame t; -1 / -inf where no path covers an entry.  bp: the back-pointers of the
// launch, the 16-bit source state of every state and frame, entry t * SM + s of the utt_stride entries of workgroup
// blockIdx.x.
struct CtcLatticeAlignArgs {
  const GTNX_G float* em;           // [n][M][C]
  const GTNX_G int* frames;         // [n]
  const GTNX_G int* arcs;           // utterance b's row at arcs + b * row_stride
  const GTNX_G int* num_arcs;       // [n]
  const GTNX_G int* num_nodes;      // [n]
  const GTNX_G float* arc_weights;  // [n][A] or null: all zeros
  GTNX_G float* scores;             // [n]
  GTNX_G int* path_len;             // [n]
  GTNX_G int* path_arcs;            // utterance b's row at path_arcs + b * out_stride, width P
  GTNX_G int* path_tokens;          // the same
  GTNX_G int* starts;               // the same
  GTNX_G int* ends;                 // the same
  GTNX_G float* token_scores;       // the same, or null
  GTNX_G int* frame_arcs;           // utterance b's row at frame_arcs + b * frame_stride, width M, or null
  GTNX_G unsigned short* bp;        // [count][utt_stride]
  int64_t row_stride, out_stride, frame_stride, utt_stride;
  int utt0, count, A, SM, P, M, C, blank;
};
void launch_ctc_lattice_align(const CtcLatticeAlignArgs& a, hipStream_t st);
// asg_score.hip: the log score forwardScore(emissions_b[:T_b] o (forceAlign(y) o transitions)) of the pairs pair0 ..
// pair0 + count - 1 in ctc_score.hip's hypothesis form (no blank: position i = 0 .. len - 1 carries y[i]), and the
// gradients sum_p weights[p] * d score[p] / d (emissions_b, table) (the contract: DESIGN section 25).  table: [C + C * C]
// in the arc order of asgTransitions, entry y = start[y], entry C + i * C + j = label j followed by label i.
//   forward:  one workgroup per pair; scores[p - score0] = the score (-inf: len == 0, T_b < len, len > U, a token
//             outside 0 .. C - 1, no alignment above -inf).  With `alpha` non-null the alpha row of every frame also
//             goes to alpha[(p - pair0) * pair_stride + t * U + i].
//   backward: one workgroup per pair: beta in LDS; with `grad` non-null the occupancy p_self + p_step of frame t and
//             position i takes the place of alpha[.. + t * U + i] (that row was read for frame t + 1).  With `occ`
//             non-null the sums over the frames, times weights[p], go to occ[p * 2 * occ_half + i] (self) and
//             occ[p * 2 * occ_half + occ_half + i] (step; position 0: the start arc).
//   scatter:  one workgroup per (utterance of the range, tile of 8 rows of its slab) walks the utterance's pairs of the
//             range in k order: the occupancies of a frame summed per label along the chain of equal tokens and added
//             into grad[b][t][label] by plain loads and stores.  The launch that holds k == 0 zeroes the rows first.
//   table:    after the last backward; workgroup i < C owns row i of the transitions, workgroup C the start entries.
//             It walks the pairs in p order and the positions ascending, adding one at a time into an LDS row, and
//             writes its C entries of grad_table, zeros included.  Pairs the backward skipped are skipped again.
// The workgroup's width and the positions per lane are chosen from U alone (asg_score_config).
constexpr int kAsgScoreMaxU = 4096;
constexpr int kAsgScoreMaxC = 16384;  // the table kernel's LDS row: C floats in 64 KiB
struct AsgScoreArgs {
  const GTNX_G float* em;       // [n][M][C]
  const GTNX_G int* frames;     // [n]
  const GTNX_G int* tokens;     // pair p's row at tokens + p * row_stride
  const GTNX_G int* lengths;    // [pairs]
  const GTNX_G float* table;    // [C + C * C]
  GTNX_G float* scores;         // [.. - score0]
  GTNX_G float* alpha;          // [count][pair_stride] or null (forward); backward turns it into occupancies
  const GTNX_G float* weights;  // [pairs] (backward, table)
  GTNX_G float* grad;           // [n][M][C] or null (backward)
  GTNX_G float* occ;            // [pairs][2][occ_half] or null (backward); read by table
  GTNX_G float* grad_table;     // [C + C * C] (table)
  int64_t row_stride, pair0, score0, pair_stride;
  int count, N, L, U, M, C, occ_half, pairs;
};
void asg_score_config(int U, int* width, int* per_lane);  // the workgroup's width and the positions a lane owns
void launch_asg_score_forward(const AsgScoreArgs& a, hipStream_t st);
void launch_asg_score_backward(const AsgScoreArgs& a, hipStream_t st);
void launch_asg_score_scatter(const AsgScoreArgs& a, hipStream_t st);
void launch_asg_score_table(const AsgScoreArgs& a, hipStream_t st);
// asg_lattice.hip: the ASG log score of the utterances utt0 .. utt0 + count - 1, each with one acyclic token lattice of its
// own in device memory (ctc_lattice.hip's form), under asg_score.hip's [C + C * C] table, and the gradients g[b] * d
// score[b] / d (emissions_b, table, arc weights of b) (the contract: DESIGN section 37).  The states are the arcs; an
// edge (a' -> a), dst a' == src a, pays w_a + table[C + lab a * C + lab a'].
//   forward:  one workgroup per utterance; scores[b - score0] = the score (-inf: T_b == 0, K < 1, K + arcs > SM, more
//             than max_edges edges, an arc that is none, a weight that is +inf or NaN, no alignment).  With `alpha`
//             non-null the alpha row of every frame also goes to alpha[(b - utt0) * utt_stride + t * SM + a].
//   backward: one workgroup per utterance zeroes grad[b] and arc_grad[b] (those asked for), then writes weights[b] times
//             the occupancies summed per label in a fixed order by plain stores.  With `edge` non-null the occupancy of
//             every edge is summed over the frames in edge[(b - utt0) * max_edges + off a + k] (k-th arc entering src a);
//             with `occ` / `csr` non-null occ[(b - utt0) * 2 SM + a] = weights[b] * the self sum, [.. + SM + a] the start
//             term, csr[(b - utt0) * 3 SM + a] = off a, [.. + SM + a] the first arc entering src a, [.. + 2 SM + a] how
//             many.
//   table:    behind the backward of the same utterances; workgroup i < C owns row i of the transitions, workgroup C the
//             start entries.  It walks the utterances in order and the arcs ascending, adding one value at a time into
//             an LDS row that starts from zeros (table_first) or from what grad_table holds, and stores the row whole.
// The workgroup's width and the arcs per lane are chosen from SM = max_states alone (asg_lattice_config).
constexpr int kAsgLatticeMaxStates = 4096;
constexpr int kAsgLatticeMaxEdges = 1 << 21;
struct AsgLatticeArgs {
  const GTNX_G float* em;           // [n][M][C]
  const GTNX_G int* frames;         // [n]
  const GTNX_G float* table;        // [C + C * C]
  const GTNX_G int* arcs;           // utterance b's row at arcs + b * row_stride
  const GTNX_G int* num_arcs;       // [n]
  const GTNX_G int* num_nodes;      // [n]
  const GTNX_G float* arc_weights;  // [n][A] or null: all zeros
  GTNX_G float* scores;             // [.. - score0]
  GTNX_G float* alpha;              // [count][utt_stride] or null (forward)
  const GTNX_G float* weights;      // [n] (backward, table)
  GTNX_G float* grad;               // [n][M][C] or null (backward)
  GTNX_G float* arc_grad;           // [n][A] or null (backward)
  GTNX_G float* grad_table;         // [C + C * C] (table)
  GTNX_G float* edge;               // [count][max_edges] or null (backward); read by table
  GTNX_G float* occ;                // [count][2][SM] or null (backward); read by table
  GTNX_G int* csr;                  // [count][3][SM] or null (backward); read by table
  int64_t row_stride, utt_stride;
  int utt0, score0, count, A, SM, M, C, max_edges, table_first;
};
void asg_lattice_config(int max_states, int* width, int* per_lane);  // the workgroup's width, the arcs a lane owns
void launch_asg_lattice_forward(const AsgLatticeArgs& a, hipStream_t st);
void launch_asg_lattice_backward(const AsgLatticeArgs& a, hipStream_t st);
void launch_asg_lattice_table(const AsgLatticeArgs& a, hipStream_t st);
// ctc_token_align.hip: the best alignment (max-plus, the arithmetic and the tie rule of align.hip) of the pairs pair0 ..
// pair0 + count - 1 of ctc_score.hip's hypothesis form (the contract: DESIGN section 24).  One workgroup per pair, width
// and states per lane from ctc_score_config(U); row p of every output is written over its whole width: scores[p] the
// path's score, starts / ends [p * out_stride + i] the first frame of token i and one past its last, token_scores (or
// null) the token's emissions summed in frame order, frame_tokens[p * frame_stride + t] (or null) the token index of
// frame t; -1 / -inf where no path covers an entry.  bp: the back-pointers of the launch, 2 bits per state and frame,
// word (t / 16) * (2 U + 1) + s of the pair_stride words of workgroup blockIdx.x.
struct CtcTokenAlignArgs {
  const GTNX_G float* em;      // [n][M][C]
  const GTNX_G int* frames;    // [n]
  const GTNX_G int* tokens;    // pair p's row at tokens + p * row_stride
  const GTNX_G int* lengths;   // [pairs]
  GTNX_G float* scores;        // [pairs]
  GTNX_G int* starts;          // pair p's row at starts + p * out_stride, width L
  GTNX_G int* ends;            // the same
  GTNX_G float* token_scores;  // the same, or null
  GTNX_G int* frame_tokens;    // pair p's row at frame_tokens + p * frame_stride, width M, or null
  GTNX_G unsigned* bp;         // [count][pair_stride]
  int64_t row_stride, out_stride, frame_stride, pair0, pair_stride;
  int count, N, L, U, M, C, blank;
};
void launch_ctc_token_align(const CtcTokenAlignArgs& a, hipStream_t st);
// asg_token_align.hip: the best alignment (max-plus, the arithmetic and the tie rule of asg_align.hip: of equals the
// step) of the pairs pair0 .. pair0 + count - 1 of asg_score.hip's hypothesis form (the contract: DESIGN section 28).
// One workgroup per pair, width and positions per lane from asg_score_config(U); the outputs are those of
// CtcTokenAlignArgs, frame_tokens never -1 inside a path.  table: [C + C * C] as in AsgScoreArgs.  bp: the back-pointers
// of the launch, 1 bit per position and frame, word (t / 32) * U + i of the pair_stride words of workgroup blockIdx.x.
struct AsgTokenAlignArgs {
  const GTNX_G float* em;      // [n][M][C]
  const GTNX_G int* frames;    // [n]
  const GTNX_G int* tokens;    // pair p's row at tokens + p * row_stride
  const GTNX_G int* lengths;   // [pairs]
  const GTNX_G float* table;   // [C + C * C]
  GTNX_G float* scores;        // [pairs]
  GTNX_G int* starts;          // pair p's row at starts + p * out_stride, width L
  GTNX_G int* ends;            // the same
  GTNX_G float* token_scores;  // the same, or null
  GTNX_G int* frame_tokens;    // pair p's row at frame_tokens + p * frame_stride, width M, or null
  GTNX_G unsigned* bp;         // [count][pair_stride]
  int64_t row_stride, out_stride, frame_stride, pair0, pair_stride;
  int count, N, L, U, M, C;
};
void launch_asg_token_align(const AsgTokenAlignArgs& a, hipStream_t st);
// materialise a KIND_LINEAR graph's arc arrays
void launch_linear_materialize(int M, int C, int* src, int* dst, int* il, int* ol, hipStream_t st);

} // namespace gtnx
