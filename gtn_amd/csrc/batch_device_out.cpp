// batch_device_out.cpp -- the batch entry points that leave their results in the caller's device memory (declared and
// specified in batch.h): forced alignment, decode against one shared graph, best path of the chains plus the CTC
// collapse, CTC prefix beam search, ASG prefix beam search, edit distance, CTC score and its gradient, CTC token
// alignment, CTC lattice score and its gradients, ASG score and its gradients, ASG lattice score and its gradients, ASG
// token alignment, CTC and ASG posterior sampling.  The kernels differ;
// the host side around them is the helpers below.
//
// Recipe for the next entry point, in this order:
//   1. GTNX_HOST_T("batch.<name>"), then every check the arguments alone decide, each message "[gtnx_batch_<name>] ...":
//      no device is asked for an invalid call.  native_linear(x) says whether x is slabs a kernel can read;
//      check_frames(...) bounds the caller's frame counts.
//   2. Runtime::get(), the early return of an empty call, check_outputs_local(...) over the output pointers.
//   3. x.w_pend->settle() if the values are read, resolve_frames(...) (and upload_vec of it for a kernel that reads it),
//      scratch from rt.alloc (scratch_cap(...) where a call is sliced), one argument struct of kernels.h, the launch
//      under GTNX_PROF with its algorithmic bytes.
//   4. the entry's Counters, and a *_stats getter that is its get().
//   An entry with a route for every other batch computes the path graphs and hands them to paths_to_rows(...).
//   An entry that reads hypothesis rows (tokens [n][N][L], lengths [n][N], max_length, one workgroup per pair: CTC score,
//   CTC token alignment, ASG score, ASG token alignment) has its own argument-only checks first, then pairs =
//   check_hypotheses(...) and the return of a call without pairs; linear_hypothesis_batch(...) for step 2's refusals,
//   its own checks of the shape and of the device, settle_frames(...) for step 3's opening, and for_pair_slices(...)
//   around launches with scratch per pair.
#include "batch.h"
#include "lm_graph.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <initializer_list>
#include <limits>
#include <string>

namespace gtnx {

namespace {

[[noreturn]] void refuse(const char* entry, const char* text) { throw_invalid(std::string("[") + entry + "] " + text); }

// the two totals behind a *_stats getter: (fast, fallback) utterances of an entry with a path-graph route, (calls,
// items) of the others
struct Counters {
  std::atomic<int64_t> first{0}, second{0};
  void add(int64_t a, int64_t b) {
    if (a) first.fetch_add(a);
    if (b) second.fetch_add(b);
  }
  void get(int64_t* a, int64_t* b) const {
    if (a) *a = first.load();
    if (b) *b = second.load();
  }
};

// the caller's frame counts (null: none to check) lie in 0 .. limit and within the rows `x` carries
struct FrameTexts {
  const char *range, *rows;
};
constexpr FrameTexts kChainFrames{"a frame count outside 0 .. T", "a frame count beyond the rows the chain carries"};
constexpr FrameTexts kBatchFrames{"a frame count outside 0 .. M", "a frame count beyond the rows the batch carries"};
void check_frames(const char* entry, const int* frames, int n, int limit, const Batch& x,
                  const FrameTexts& texts = kBatchFrames) {
  if (!frames) return;
  for (int b = 0; b < n; ++b) {
    if (frames[b] < 0 || frames[b] > limit) refuse(entry, texts.range);
    if (frames[b] > x.rows_of(b)) refuse(entry, texts.rows);
  }
}

// a kernel of this device writes the results: memory of another GPU of the process is refused, not written
void check_outputs_local(const char* entry, std::initializer_list<const void*> outs) {
  const int dev = Runtime::get().device();
  for (const void* p : outs)
    if (p && !ptr_local_to(p, dev)) refuse(entry, "an output pointer is not memory of the engine's current device");
}

// slabs a kernel can read in place (gtnx_batch_linear / _rows)
bool native_linear(const Batch& b) { return b.kind == Batch::LINEAR && !b.leaf && b.w_dev; }

// T_b of every element: the caller's count, else the rows the batch carries
std::vector<int> resolve_frames(const int* frames, const Batch& x) {
  std::vector<int> fr(static_cast<size_t>(x.n));
  for (int b = 0; b < x.n; ++b) fr[size_t(b)] = frames ? frames[b] : x.rows_of(b);
  return fr;
}

// what the scratch of ONE launch may take; a call that needs more runs in slices of launches.  `env`: debug switch, read
// per call: tests lower the cap to see a sliced call without allocating gigabytes
struct ScratchCap {
  const char* env;
  int64_t bytes;
};
int64_t scratch_cap(const ScratchCap& cap) {
  const char* e = std::getenv(cap.env);
  if (e && *e) {
    const long long v = std::atoll(e);
    if (v > 0) return std::min<int64_t>(v, cap.bytes);
  }
  return cap.bytes;
}

// body(p0, count) over the pairs in slices whose scratch, `bytes_per_pair` each, stays within the cap; a pair that is
// above the cap by itself runs alone
template <class Body>
void for_pair_slices(int64_t pairs, int64_t bytes_per_pair, const ScratchCap& cap, Body&& body) {
  const int64_t room = scratch_cap(cap);
  const int64_t slice = bytes_per_pair > 0 ? std::max<int64_t>(1, room / bytes_per_pair) : pairs;
  for (int64_t p0 = 0; p0 < pairs; p0 += slice) body(p0, std::min(slice, pairs - p0));
}

// ---- what the entries that read hypothesis rows share (ctc_score.hip, ctc_token_align.hip, asg_score.hip,
// asg_token_align.hip) ----
// the rows as the caller describes them: pair p = b * N + k has tokens[p * row_stride .. + L) and lengths[p], and no
// length counts beyond max_length
struct Hypotheses {
  const int* tokens;
  int64_t row_stride;
  const int* lengths;
  int N, L, max_length;
};
static_assert(kCtcScoreMaxU == 4096 && kAsgScoreMaxU == 4096, "the text below says 4096");

// what the arguments alone decide about the rows.  Returns the number of pairs: a call without any returns OK without
// asking for a device
int64_t check_hypotheses(const char* who, const BatchP& ems, const Hypotheses& h) {
  if (!ems) refuse(who, "null batch");
  if (!h.tokens || !h.lengths) refuse(who, "null input pointer (tokens and lengths are both read)");
  if (h.N < 0 || h.L < 0) refuse(who, "negative N or L");
  if (h.row_stride < 0) refuse(who, "negative row stride");
  if (h.row_stride < h.L) refuse(who, "row_stride is shorter than the rows' width L");
  if (h.max_length < 1 || h.max_length > kCtcScoreMaxU) refuse(who, "max_length outside 1 .. 4096");
  const int64_t pairs = int64_t(ems->n) * h.N;
  if (pairs > std::numeric_limits<int>::max()) refuse(who, "n times N does not fit an int");
  return pairs;
}

// the first refusals of the device side.  There is no other route: the results are those of the slabs of a native linear
// batch
Batch& linear_hypothesis_batch(const char* who, const BatchP& ems, const int* frames) {
  Runtime::get();
  if (!native_linear(*ems)) refuse(who, "not a native linear batch (gtnx_batch_linear / _rows)");
  check_frames(who, frames, ems->n, ems->M, *ems);
  return *ems;
}

// behind the last refusal: the values settled, T_b of every utterance uploaded, and what every argument struct of these
// kernels says about the slabs and the rows filled in.  Returns the largest T_b and the mean one (every utterance has N
// pairs: the frames of a pair of the algorithmic bytes)
struct PairFrames {
  DevMemP dev;
  int maxT = 0;
  double mean = 0;
};
template <class Args>
PairFrames settle_frames(Batch& x, const int* frames, const Hypotheses& h, Args& a) {
  if (x.w_pend) x.w_pend->settle();  // (the values are read here: graph.h PendingCopy)
  const std::vector<int> fr = resolve_frames(frames, x);
  PairFrames f;
  double sum = 0;
  for (int t : fr) {
    f.maxT = std::max(f.maxT, t);
    sum += t;
  }
  f.mean = sum / double(x.n);
  f.dev = upload_vec(fr);
  a.em = x.w_dev;
  a.frames = f.dev->as<int>();
  a.tokens = h.tokens;
  a.lengths = h.lengths;
  a.row_stride = h.row_stride;
  a.N = h.N;
  a.L = h.L;
  a.U = h.max_length;
  a.M = x.M;
  a.C = x.C;
  return f;
}

// The route of every batch no kernel takes: the labels of the path graphs read on the host, one upload.  Row b of
// `labels` gets path b's labels and -1 up to the rows' width (`width_floor`, or the longest path if that is longer; a
// width of 0 copies no label plane), `scores` the weights summed in path order, -inf without a path; with `collapsed`
// the labels with repeats merged (and `blank` dropped if `drop_blank`), `starts` the first frame of each, `lengths` how
// many.  All but `labels` may be null.
struct PathRows {
  int64_t width_floor;
  bool arcless_scores_zero;  // a path with nodes and no arcs scores 0, not -inf
  bool drop_blank;
  int blank;
  int* labels;
  int64_t row_stride;
  float* scores;
  int *collapsed, *starts, *lengths;
};
void paths_to_rows(const char* entry, std::vector<Graph>& paths, const PathRows& o) {
  Runtime& rt = Runtime::get();
  const int n = int(paths.size());
  int64_t width = o.width_floor;
  for (Graph& g : paths) width = std::max<int64_t>(width, g.num_arcs());
  if (width > o.row_stride) refuse(entry, "row_stride is shorter than the longest path");
  const size_t cells = size_t(n) * size_t(width ? width : 1);
  int* dst[3] = {o.labels, o.collapsed, o.starts};
  PinnedMemP hl = rt.alloc_pinned(sizeof(int) * cells * 3);
  PinnedMemP hs = rt.alloc_pinned((sizeof(float) + sizeof(int)) * size_t(n));
  int* src[3] = {hl->as<int>(), hl->as<int>() + cells, hl->as<int>() + 2 * cells};
  float* sc = hs->as<float>();
  int* len_out = reinterpret_cast<int*>(sc + n);
  std::fill(src[0], src[0] + 3 * cells, -1);
  for (int b = 0; b < n; ++b) {
    Graph& g = paths[size_t(b)];
    const int64_t len = g.num_arcs();
    // (no path, zero frames included: the empty graph)
    float score = (g.num_nodes() > 0 && (o.arcless_scores_zero || len > 0)) ? 0.0f : -std::numeric_limits<float>::infinity();
    int k = 0;
    if (len > 0) {
      g.s->ensure_host();
      int* row = src[0] + size_t(b) * size_t(width);
      int* crow = src[1] + size_t(b) * size_t(width);
      int* srow = src[2] + size_t(b) * size_t(width);
      std::copy(g.s->il.begin(), g.s->il.begin() + len, row);
      const float* w = g.weights_host(false);
      for (int64_t t = 0; t < len; ++t) {
        score += w[t];  // (in path order, as the recursion accumulates it)
        if ((t == 0 || row[t] != row[t - 1]) && !(o.drop_blank && row[t] == o.blank)) {
          crow[k] = row[t];
          srow[k++] = int(t);
        }
      }
    }
    sc[b] = score;
    len_out[b] = k;
  }
  if (width > 0)
    for (int i = 0; i < 3; ++i)
      if (dst[i])
        HIP_CHECK(hipMemcpy2DAsync(dst[i], sizeof(int) * size_t(o.row_stride), src[i], sizeof(int) * size_t(width),
                                   sizeof(int) * size_t(width), size_t(n), hipMemcpyHostToDevice, rt.stream()));
  if (o.scores) rt.h2d_pinned(o.scores, sc, sizeof(float) * size_t(n));
  if (o.lengths) rt.h2d_pinned(o.lengths, len_out, sizeof(int) * size_t(n));
}

}  // namespace

// ---- forced alignment with device-resident output (align.hip, asg_align.hip) ---------------------------------
namespace {
constexpr const char* kAlign = "gtnx_batch_viterbi_align";
Counters g_align;  // (fast, fallback)

// every other batch: the path graphs of batch_viterbi_path
void align_fallback(const BatchP& x, const int* frames, int* labels_dev, int64_t row_stride, int* tokens_dev,
                    float* scores_dev) {
  if (tokens_dev)
    throw_invalid("[gtnx_batch_viterbi_align] token indices are defined for device-built CTC targets or ASG force-alignment "
                  "acceptors composed with a linear batch only (this batch takes the path-graph route)");
  if (frames)
    throw_invalid("[gtnx_batch_viterbi_align] per-utterance frame counts need device-built CTC targets or ASG "
                  "force-alignment acceptors composed with a linear batch (this batch takes the path-graph route)");
  GTNX_HOST_T("batch.viterbi_align.fallback");
  // (a PRODUCT's rows are as long as its chains; other batches: as long as the longest path)
  const int64_t floor = (x->kind == Batch::PRODUCT && x->chain && x->chain->kind == Batch::LINEAR) ? x->chain->M : 0;
  BatchP paths = batch_viterbi_path(x);
  paths_to_rows(kAlign, paths->graphs, {floor, true, false, 0, labels_dev, row_stride, scores_dev, nullptr, nullptr, nullptr});
  g_align.add(0, x->n);
}
}  // namespace

void batch_align_stats(int64_t* fast, int64_t* fallback) { g_align.get(fast, fallback); }

void batch_viterbi_align(const BatchP& x, const int* frames, int* labels_dev, int64_t row_stride, int* tokens_dev,
                         float* scores_dev) {
  GTNX_HOST_T("batch.viterbi_align");
  Runtime& rt = Runtime::get();  // (first: without a device this is a device error, whatever the arguments)
  if (!labels_dev) throw_invalid("[gtnx_batch_viterbi_align] null labels pointer");
  if (row_stride < 0) throw_invalid("[gtnx_batch_viterbi_align] negative row stride");
  const int n = x->n;
  if (n <= 0) return;
  check_outputs_local(kAlign, {labels_dev, tokens_dev, scores_dev});
  // device-built CTC targets (align.hip), or device-built force-alignment acceptors o ASG transitions (asg_align.hip),
  // composed with a linear batch in either argument order
  const bool built = x->kind == Batch::PRODUCT && x->fixed && x->chain && x->fixed->kind == Batch::CTC_TARGETS &&
                     x->chain->kind == Batch::LINEAR && x->fixed->rec_mem && x->fixed->n == n && x->chain->n == n;
  bool fast = built && !x->fixed->fal, asg = built && x->fixed->fal;
  if (built) {
    const Batch& fx = *x->fixed;
    const Batch& ch = *x->chain;
    const int vec = ch.C % 4 == 0 && (reinterpret_cast<uintptr_t>(ch.w_dev) & 15) == 0;
    fast = fast && band_align_ok(fx.max_nodes, ch.C, vec) && fx.max_label < ch.C;
    // the closed form of the queue ranks (ops_band.cpp tie_ranks) holds with the blank below every label
    for (size_t i = 0; i < fx.labels.size() && fast; ++i) fast = fx.labels[i] > fx.blank;
    asg = asg && asg_align_ok(fx.max_nodes, ch.C, vec) && fx.trans_labels == ch.C && fx.max_label < ch.C;
  }
  if (!fast && !asg) {
    align_fallback(x, frames, labels_dev, row_stride, tokens_dev, scores_dev);
    return;
  }
  Batch& fx = *x->fixed;
  Batch& ch = *x->chain;
  const int T = ch.M, C = ch.C;
  if (row_stride < T) throw_invalid("[gtnx_batch_viterbi_align] row_stride is shorter than the chains");
  check_frames(kAlign, frames, n, T, ch, kChainFrames);
  if (ch.w_pend) ch.w_pend->settle();  // (the values are read here: graph.h PendingCopy)
  const std::vector<int> fr = resolve_frames(frames, ch);
  // what AlignArgs and AsgAlignArgs share: element b's N band nodes, its emissions, its back-pointer plane, its rows
  auto common = [&](auto& a, int b, size_t N, unsigned* bp) {
    char* base = fx.rec_mem->as<char>(fx.rec_off[size_t(b)]);
    a.nodes = reinterpret_cast<BandNode*>(base);
    a.nflags = reinterpret_cast<uint8_t*>(base + align_up(sizeof(BandNode) * N, 64));
    a.em = ch.w_dev + size_t(b) * size_t(T) * size_t(C);
    a.bp = bp;
    a.labels = labels_dev + int64_t(b) * row_stride;
    a.tokens = tokens_dev ? tokens_dev + int64_t(b) * row_stride : nullptr;
    a.score = scores_dev ? scores_dev + b : nullptr;
    a.N = int(N);
    a.T = fr[size_t(b)];
    a.T_full = T;
    a.C = C;
  };
  double abytes = 0;
  if (asg) {
    // back-pointer planes: 1 bit per (time, node), one 256-byte row of words per 32 / NPL steps, NPL the LAUNCH's
    const int npl = asg_align_npl(fx.max_nodes);
    const size_t plane = asg_align_plane_bytes(T, npl);
    DevMemP work = rt.alloc(plane * size_t(n));
    std::vector<AsgAlignArgs> tab(static_cast<size_t>(n));
    for (int b = 0; b < n; ++b) {
      AsgAlignArgs& a = tab[size_t(b)];
      a = AsgAlignArgs{};
      const size_t N = size_t(fx.lab_off[size_t(b) + 1] - fx.lab_off[size_t(b)]) + 1;
      common(a, b, N, work->as<unsigned>(plane * size_t(b)));
      a.w = fx.rec_mem->as<float>(fx.w_off[size_t(b)]);
      abytes += 4.0 * a.T * C + 0.25 * double(a.T) * double(N) + 8.0 * a.T;
    }
    DevMemP d = upload_vec(tab);
    GTNX_PROF("asg_viterbi_align", abytes);
    launch_asg_align(d->as<AsgAlignArgs>(), n, fx.max_nodes, rt.stream());
    g_align.add(n, 0);
    return;
  }
  // back-pointer planes: 2 bits per (time, node), one 256-byte row of words per 16 / NPL steps (align.hip)
  const int npl = align_npl(fx.max_nodes);
  const size_t plane = align_up((size_t(T) * size_t(npl) + 15) / 16 * 256 + 256, 256);
  DevMemP work = rt.alloc(plane * size_t(n));
  std::vector<AlignArgs> tab(static_cast<size_t>(n));
  for (int b = 0; b < n; ++b) {
    AlignArgs& a = tab[size_t(b)];
    a = AlignArgs{};
    const int* t = fx.labels.data() + fx.lab_off[size_t(b)];
    const int U = fx.lab_off[size_t(b) + 1] - fx.lab_off[size_t(b)];
    const size_t N = size_t(2 * U + 1);
    common(a, b, N, work->as<unsigned>(plane * size_t(b)));
    int p = 0;
    while (p + 1 < U && t[p] < t[p + 1]) ++p;
    a.p = p;
    abytes += 4.0 * a.T * C + 0.5 * double(a.T) * double(N) + 8.0 * a.T;
  }
  DevMemP d = upload_vec(tab);
  GTNX_PROF("band_viterbi_align", abytes);
  launch_band_align(d->as<AlignArgs>(), n, fx.max_nodes, rt.stream());
  g_align.add(n, 0);
}

// ---- decode against one shared transitions graph with device-resident output (asg_decode.hip) ----------------
namespace {
constexpr const char* kDecode = "gtnx_batch_viterbi_decode";
Counters g_decode;  // (fast, fallback)

// every other graph or batch: viterbiPath over the composed elements
void decode_fallback(const BatchP& ems, Graph& transitions, const int* frames, int* labels_dev, int64_t row_stride,
                     float* scores_dev, int* collapsed_dev, int* lengths_dev) {
  if (frames)
    throw_invalid("[gtnx_batch_viterbi_decode] per-utterance frame counts need a linear batch and a dense transitions "
                  "graph of 8 .. 1024 nodes whose ties go by node order (this batch takes the path-graph route, which "
                  "decodes the rows the elements carry: pass frames = null)");
  GTNX_HOST_T("batch.viterbi_decode.fallback");
  batch_materialise(*ems);
  std::vector<Graph> tr{transitions};
  std::vector<Graph> comp = op_compose(ems->graphs, tr, false);
  std::vector<Graph> paths = op_viterbi_path(comp);
  paths_to_rows(kDecode, paths, {ems->kind == Batch::LINEAR ? ems->M : 0, false, false, 0, labels_dev, row_stride, scores_dev,
                                 collapsed_dev, nullptr, lengths_dev});
  g_decode.add(0, ems->n);
}
}  // namespace

void batch_decode_stats(int64_t* fast, int64_t* fallback) { g_decode.get(fast, fallback); }

void batch_viterbi_decode(const BatchP& ems, Graph& transitions, const int* frames, int* labels_dev, int64_t row_stride,
                          float* scores_dev, int* collapsed_dev, int* lengths_dev) {
  GTNX_HOST_T("batch.viterbi_decode");
  // what the arguments alone decide comes first: no device is asked for an invalid call
  if (!ems) throw_invalid("[gtnx_batch_viterbi_decode] null batch");
  if (!labels_dev) throw_invalid("[gtnx_batch_viterbi_decode] null labels pointer");
  if (row_stride < 0) throw_invalid("[gtnx_batch_viterbi_decode] negative row stride");
  if (lengths_dev && !collapsed_dev)
    throw_invalid("[gtnx_batch_viterbi_decode] lengths are those of the collapsed sequences: pass collapsed_device too");
  const int n = ems->n;
  // (a linear batch without values of its own is bounded like one with them, and refused by the route it takes)
  const bool linear = ems->kind == Batch::LINEAR && !ems->leaf;
  if (linear) check_frames(kDecode, frames, n, ems->M, *ems);
  if (linear && n > 0 && row_stride < ems->M)
    throw_invalid("[gtnx_batch_viterbi_decode] row_stride is shorter than the rows of the batch");
  Runtime::get();
  if (n <= 0) return;
  check_outputs_local(kDecode, {labels_dev, scores_dev, collapsed_dev, lengths_dev});
  if (!native_linear(*ems) || !lazy_decode_ok(transitions, ems->M, ems->C)) {
    decode_fallback(ems, transitions, frames, labels_dev, row_stride, scores_dev, collapsed_dev, lengths_dev);
    return;
  }
  Batch& x = *ems;
  if (x.w_pend) x.w_pend->settle();  // (the values are read here: graph.h PendingCopy)
  // full-length views of the slabs (batch_materialise's elements with M rows whatever `rows` says): one shape, one
  // group, one sweep -- the sweep reads the pad rows, the back-trace never looks at what it made of them
  std::vector<Graph> chains;
  chains.reserve(size_t(n));
  {
    GraphSlabScope slab_scope(size_t(n));
    const int64_t stride = int64_t(x.M) * x.C;
    for (int i = 0; i < n; ++i) {
      Graph g = Graph::make_result(false);
      Structure& s = *g.s;
      s.kind = KIND_LINEAR;
      s.M = x.M;
      s.C = x.C;
      s.N = int64_t(x.M) + 1;
      s.A = stride;
      s.ilabel_sorted = s.olabel_sorted = true;
      Weights& w = *g.w;
      w.n = stride;
      w.dev_mem = x.w_mem;
      w.dev = x.w_dev + size_t(i) * size_t(stride);
      w.dev_valid = true;
      w.host_valid = false;
      w.version++;
      chains.push_back(std::move(g));
    }
  }
  lazy_viterbi_decode(chains, transitions, resolve_frames(frames, x), labels_dev, row_stride, scores_dev, collapsed_dev,
                      lengths_dev);
  g_decode.add(n, 0);
}

// ---- best path of the chains themselves plus the CTC collapse, device-resident output (linear_decode.hip) ----
namespace {
constexpr const char* kLinearDecode = "gtnx_batch_linear_decode";
Counters g_linear_decode;  // (fast, fallback)
}  // namespace

void batch_linear_decode_stats(int64_t* fast, int64_t* fallback) { g_linear_decode.get(fast, fallback); }

void batch_linear_decode(const BatchP& ems, const int* frames, int blank, int* labels_dev, int64_t row_stride,
                         float* scores_dev, int* collapsed_dev, int* starts_dev, int* lengths_dev) {
  GTNX_HOST_T("batch.linear_decode");
  // what the arguments alone decide comes first: no device is asked for an invalid call
  if (!ems) throw_invalid("[gtnx_batch_linear_decode] null batch");
  if (!labels_dev) throw_invalid("[gtnx_batch_linear_decode] null labels pointer");
  if (row_stride < 0) throw_invalid("[gtnx_batch_linear_decode] negative row stride");
  if ((lengths_dev || starts_dev) && !collapsed_dev)
    throw_invalid("[gtnx_batch_linear_decode] lengths and starts are those of the collapsed sequences: pass "
                  "collapsed_device too");
  const int n = ems->n;
  const bool linear = native_linear(*ems);
  if (frames && !linear)
    throw_invalid("[gtnx_batch_linear_decode] per-utterance frame counts need a native linear batch (this batch takes "
                  "the path-graph route, which decodes the rows the elements carry: pass frames = null)");
  check_frames(kLinearDecode, frames, n, ems->M, *ems);
  if (linear && n > 0 && row_stride < ems->M)
    throw_invalid("[gtnx_batch_linear_decode] row_stride is shorter than the rows of the batch");
  if (linear && blank >= ems->C) throw_invalid("[gtnx_batch_linear_decode] blank is not below the number of labels");
  Runtime& rt = Runtime::get();
  if (n <= 0) return;
  check_outputs_local(kLinearDecode, {labels_dev, scores_dev, collapsed_dev, starts_dev, lengths_dev});
  Batch& x = *ems;
  if (x.w_pend) x.w_pend->settle();  // (the values are read here: graph.h PendingCopy)
  if (!linear) {
    // every other batch: the path graphs of batch_viterbi_path
    GTNX_HOST_T("batch.linear_decode.fallback");
    BatchP paths = batch_viterbi_path(ems);
    paths_to_rows(kLinearDecode, paths->graphs, {x.kind == Batch::LINEAR ? x.M : 0, true, true, blank, labels_dev, row_stride,
                                                 scores_dev, collapsed_dev, starts_dev, lengths_dev});
    g_linear_decode.add(0, n);
    return;
  }
  const std::vector<int> fr = resolve_frames(frames, x);
  // algorithmic bytes: every emission of the rows that count once, label and maximum out / back in, the pad of the
  // label rows, the collapsed rows
  double row_bytes = 0, col_bytes = 0;
  for (int t : fr) {
    row_bytes += 4.0 * x.C * t + 8.0 * t;
    col_bytes += 8.0 * t + 4.0 * (x.M - t) + (collapsed_dev ? 8.0 * x.M : 0.0);
  }
  DevMemP d_frames = upload_vec(fr);
  DevMemP rowmax = rt.alloc(sizeof(float) * std::max<size_t>(size_t(n) * size_t(x.M), 1));
  LinearDecodeArgs a{};
  a.em = x.w_dev;
  a.frames = d_frames->as<int>();
  a.labels = labels_dev;
  a.rowmax = rowmax->as<float>();
  a.scores = scores_dev;
  a.collapsed = collapsed_dev;
  a.starts = starts_dev;
  a.lengths = lengths_dev;
  a.row_stride = row_stride;
  a.n = n;
  a.M = x.M;
  a.C = x.C;
  a.blank = blank;
  {
    GTNX_PROF("linear_decode_rows", row_bytes);
    launch_linear_decode(a, 0, rt.stream());
  }
  {
    GTNX_PROF("linear_decode_collapse", col_bytes);
    launch_linear_decode(a, 1, rt.stream());
  }
  // (the scratch and the table go back to the stream-ordered pool behind the launches)
  g_linear_decode.add(n, 0);
}

// ---- N sampled alignments per chain plus the CTC collapse, device-resident (ctc_sample.hip) ----
namespace {
constexpr const char* kCtcSample = "gtnx_batch_ctc_sample";
Counters g_ctc_sample;  // (calls, utterances)
// label and term of every (b, k, t) of one launch
constexpr ScratchCap kCtcSampleScratch{"GTNX_CTC_SAMPLE_SCRATCH_BYTES", int64_t(256) << 20};
}  // namespace

void batch_ctc_sample_stats(int64_t* calls, int64_t* utterances) { g_ctc_sample.get(calls, utterances); }

void batch_ctc_sample(const BatchP& ems, const int* frames, int blank, int N, uint64_t seed, float temperature,
                      int* tokens_dev, int64_t row_stride, int* lengths_dev, float* logq_dev, int* labels_dev) {
  GTNX_HOST_T("batch.ctc_sample");
  // what the arguments alone decide comes first: no device is asked for an invalid call
  if (!ems) refuse(kCtcSample, "null batch");
  if (!tokens_dev || !lengths_dev) refuse(kCtcSample, "null output pointer (tokens and lengths are both written)");
  if (row_stride < 0) refuse(kCtcSample, "negative row stride");
  if (N < 1 || N > kCtcSampleMaxN) refuse(kCtcSample, "num_samples outside 1 .. 1024");
  if (!std::isfinite(temperature) || !(temperature > 0.0f)) refuse(kCtcSample, "temperature must be finite and above 0");
  Runtime& rt = Runtime::get();
  const int n = ems->n;
  // there is no other route: the sampler reads the slabs of a native linear batch
  if (!native_linear(*ems)) refuse(kCtcSample, "not a native linear batch (gtnx_batch_linear / _rows)");
  Batch& x = *ems;
  check_frames(kCtcSample, frames, n, x.M, x);
  if (n > 0 && row_stride < x.M) refuse(kCtcSample, "row_stride is shorter than the rows of the batch");
  if (blank >= x.C) refuse(kCtcSample, "blank is not below the number of labels");
  if (int64_t(n) * N > std::numeric_limits<int>::max()) refuse(kCtcSample, "n times num_samples does not fit an int");
  if (n <= 0) return;
  check_outputs_local(kCtcSample, {tokens_dev, lengths_dev, logq_dev, labels_dev});
  if (x.w_pend) x.w_pend->settle();  // (the values are read here: graph.h PendingCopy)
  const std::vector<int> fr = resolve_frames(frames, x);
  DevMemP d_frames = upload_vec(fr);
  CtcSampleArgs a{};
  a.row_stride = row_stride;
  a.label_stride = labels_dev ? row_stride : x.M;
  a.M = x.M;
  a.C = x.C;
  a.blank = blank;
  a.N = N;
  a.fill_labels = labels_dev ? 1 : 0;
  a.seed_lo = static_cast<unsigned>(seed & 0xffffffffu);
  a.seed_hi = static_cast<unsigned>(seed >> 32);
  a.temperature = temperature;
  // the utterances in slices whose scratch stays within the cap: the term of every (b, k, t), and its label where the
  // caller takes none
  const int64_t per_utt = int64_t(N) * x.M * (labels_dev ? 4 : 8);
  for_pair_slices(n, per_utt, kCtcSampleScratch, [&](int64_t b0, int64_t count) {
    // algorithmic bytes.  rows: every emission of the rows that count once, label and term out.  collapse: those back
    // in, the pad of the label rows, the token rows, length and logq.
    double row_bytes = 0, col_bytes = 0;
    for (int64_t b = b0; b < b0 + count; ++b) {
      const int t = fr[size_t(b)];
      row_bytes += 4.0 * x.C * t + 8.0 * N * t;
      col_bytes += N * (8.0 * t + (labels_dev ? 4.0 * (x.M - t) : 0.0) + 4.0 * x.M + 8.0);
    }
    const size_t cells = std::max<size_t>(size_t(count) * size_t(N) * size_t(x.M), 1);
    DevMemP terms = rt.alloc(sizeof(float) * cells);
    DevMemP labs = labels_dev ? DevMemP() : rt.alloc(sizeof(int) * cells);
    CtcSampleArgs s = a;
    s.em = x.w_dev + b0 * x.M * x.C;
    s.frames = d_frames->as<int>() + b0;
    s.labels = labels_dev ? labels_dev + b0 * N * row_stride : labs->as<int>();
    s.terms = terms->as<float>();
    s.tokens = tokens_dev + b0 * N * row_stride;
    s.lengths = lengths_dev + b0 * N;
    s.logq = logq_dev ? logq_dev + b0 * N : nullptr;
    s.n = static_cast<int>(count);
    s.b0 = static_cast<int>(b0);
    {
      GTNX_PROF("ctc_sample_rows", row_bytes);
      launch_ctc_sample(s, 0, rt.stream());
    }
    {
      GTNX_PROF("ctc_sample_collapse", col_bytes);
      launch_ctc_sample(s, 1, rt.stream());
    }
    // (the scratch goes back to the stream-ordered pool behind the launches)
  });
  g_ctc_sample.add(1, n);
}

// ---- CTC prefix beam search with N-best output, device-resident (ctc_beam.hip) ----
namespace {
constexpr const char* kCtcBeam = "gtnx_batch_ctc_beam_decode";
Counters g_ctc_beam;  // (calls, utterances)
}  // namespace

void batch_ctc_beam_stats(int64_t* calls, int64_t* utterances) { g_ctc_beam.get(calls, utterances); }

void batch_ctc_beam_decode(const BatchP& ems, const int* frames, int blank, int beam, int topn, int nbest,
                           int* tokens_dev, int64_t row_stride, int* lengths_dev, float* scores_dev) {
  batch_ctc_beam_decode(ems, frames, blank, beam, topn, nbest, nullptr, tokens_dev, row_stride, lengths_dev, scores_dev);
}

void batch_ctc_beam_decode(const BatchP& ems, const int* frames, int blank, int beam, int topn, int nbest,
                           const CtcBeamLm* lm, int* tokens_dev, int64_t row_stride, int* lengths_dev,
                           float* scores_dev) {
  GTNX_HOST_T("batch.ctc_beam_decode");
  // what the arguments alone decide comes first: no device is asked for an invalid call
  if (!ems) throw_invalid("[gtnx_batch_ctc_beam_decode] null batch");
  if (!tokens_dev || !lengths_dev || !scores_dev)
    throw_invalid("[gtnx_batch_ctc_beam_decode] null output pointer (tokens, lengths and scores are all written)");
  if (row_stride < 0) throw_invalid("[gtnx_batch_ctc_beam_decode] negative row stride");
  if (beam < 1 || beam > 64) throw_invalid("[gtnx_batch_ctc_beam_decode] beam_size outside 1 .. 64");
  if (topn < 1 || topn > 32) throw_invalid("[gtnx_batch_ctc_beam_decode] cutoff_top_n outside 1 .. 32");
  if (nbest < 1) throw_invalid("[gtnx_batch_ctc_beam_decode] nbest below 1");
  if (nbest > beam) throw_invalid("[gtnx_batch_ctc_beam_decode] nbest above beam_size");
  if (blank < 0) throw_invalid("[gtnx_batch_ctc_beam_decode] negative blank");
  LmGraphP lmg;
  if (lm && lm->graph) {
    if (lm->table_dev) throw_invalid("[gtnx_batch_ctc_beam_decode] a language model table and an LM graph together");
    lmg = lm_graph_lookup(lm->graph);
    if (!lmg) throw_invalid("[gtnx_batch_ctc_beam_decode] not a live LM graph handle (destroyed, or not from gtnx_lm_graph_create)");
  }
  if (lm) {
    if (!lm->table_dev && !lmg) throw_invalid("[gtnx_batch_ctc_beam_decode] null language model table");
    if (!std::isfinite(lm->weight) || !std::isfinite(lm->bonus))
      throw_invalid("[gtnx_batch_ctc_beam_decode] lm_weight and insertion_bonus must be finite");
  }
  Runtime& rt = Runtime::get();
  const int n = ems->n;
  // there is no other route: the search runs on the slabs of a native linear batch
  if (!native_linear(*ems)) throw_invalid("[gtnx_batch_ctc_beam_decode] not a native linear batch (gtnx_batch_linear / _rows)");
  Batch& x = *ems;
  check_frames(kCtcBeam, frames, n, x.M, x);
  if (n > 0 && row_stride < x.M)
    throw_invalid("[gtnx_batch_ctc_beam_decode] row_stride is shorter than the rows of the batch");
  if (blank >= x.C) throw_invalid("[gtnx_batch_ctc_beam_decode] blank is not below the number of labels");
  // (a candidate's key keeps its label in 25 bits; trie nodes are numbered 1 + t * beam + slot in an int)
  if (x.C > (1 << 25)) throw_invalid("[gtnx_batch_ctc_beam_decode] more than 2^25 labels");
  // (with a table the key also keeps the label's place in the token set, in 6 of those bits; a table of (2^19)^2
  //  entries is four terabytes)
  if (lm && x.C > (1 << 19)) throw_invalid("[gtnx_batch_ctc_beam_decode] more than 2^19 labels with a language model table");
  if (int64_t(x.M) * beam + 1 > std::numeric_limits<int>::max())
    throw_invalid("[gtnx_batch_ctc_beam_decode] rows times beam_size does not fit an int");
  if (n <= 0) return;
  check_outputs_local(kCtcBeam, {tokens_dev, lengths_dev, scores_dev});
  if (lm) {
    check_outputs_local(kCtcBeam, {lm->am_scores_dev});
    // (the kernel gathers from it: host memory is refused too, with one GPU as well)
    if (!lmg && !ptr_device_memory_of(lm->table_dev, rt.device()))
      refuse(kCtcBeam, "the language model table is not memory of the engine's current device");
  }
  // (uploaded by the first decode that uses it; a graph that lives on another device is refused here)
  const gtnx_i4* lmg_dev = lmg ? lm_graph_device(*lmg, kCtcBeam) : nullptr;
  if (x.w_pend) x.w_pend->settle();  // (the values are read here: graph.h PendingCopy)
  const std::vector<int> fr = resolve_frames(frames, x);
  // algorithmic bytes.  rows: every emission of the rows that count once, topn + 1 entries and a count out.  search:
  // those back in, a trie node per kept extension (at most beam per frame), the output rows; with a table one 4-byte
  // gather per (beam, member of the set) and frame at the most, and the second score.
  double row_bytes = 0, search_bytes = 0;
  for (int t : fr) {
    row_bytes += (4.0 * x.C + 8.0 * (topn + 1) + 4.0) * t;
    search_bytes += (8.0 * (topn + 1) + 4.0 + 8.0 * beam) * t + nbest * (4.0 * x.M + 8.0);
    if (lm) search_bytes += 4.0 * beam * (topn + 1) * t + (lm->am_scores_dev ? 4.0 * nbest : 0.0);
  }
  DevMemP d_frames = upload_vec(fr);
  const size_t rows = std::max<size_t>(size_t(n) * size_t(x.M), 1);
  DevMemP entries = rt.alloc(8 * rows * size_t(topn + 1));
  DevMemP counts = rt.alloc(sizeof(int) * rows);
  DevMemP trie = rt.alloc(8 * size_t(n) * (size_t(x.M) * size_t(beam) + 1));
  CtcBeamArgs a{};
  a.em = x.w_dev;
  a.frames = d_frames->as<int>();
  a.ent_val = entries->as<float>();
  a.ent_cnt = counts->as<int>();
  a.trie = trie->as<int>();
  a.tokens = tokens_dev;
  a.lengths = lengths_dev;
  a.scores = scores_dev;
  a.row_stride = row_stride;
  a.n = n;
  a.M = x.M;
  a.C = x.C;
  a.blank = blank;
  a.beam = beam;
  a.topn = topn;
  a.nbest = nbest;
  if (lm) {
    a.lm = lm->table_dev;
    a.lm_weight = lm->weight;
    a.lm_bonus = lm->bonus;
    a.am_scores = lm->am_scores_dev;
  }
  if (lmg) {
    a.lmg = lmg_dev;
    a.lmg_states = lmg->states;
    a.lmg_start = lmg->start;
  }
  {
    GTNX_PROF("ctc_beam_rows", row_bytes);
    launch_ctc_beam(a, 0, rt.stream());
  }
  {
    GTNX_PROF("ctc_beam_search", search_bytes);
    launch_ctc_beam(a, 1, rt.stream());
  }
  // (the scratch and the table go back to the stream-ordered pool behind the launches)
  g_ctc_beam.add(1, n);
}

// ---- ASG prefix beam search with N-best output, device-resident (asg_beam.hip) ----
namespace {
constexpr const char* kAsgBeam = "gtnx_batch_asg_beam_decode";
constexpr const char* kAsgBeamGraph = "gtnx_batch_asg_beam_decode_graph";
Counters g_asg_beam;  // (calls, utterances)
}  // namespace

void batch_asg_beam_stats(int64_t* calls, int64_t* utterances) { g_asg_beam.get(calls, utterances); }

void batch_asg_beam_decode(const BatchP& ems, const int* frames, const float* table_dev, int beam, int topn, int nbest,
                           int* tokens_dev, int64_t row_stride, int* lengths_dev, float* scores_dev) {
  batch_asg_beam_decode(ems, frames, table_dev, beam, topn, nbest, nullptr, tokens_dev, row_stride, lengths_dev,
                        scores_dev);
}

void batch_asg_beam_decode(const BatchP& ems, const int* frames, const float* table_dev, int beam, int topn, int nbest,
                           const AsgBeamLm* lm, int* tokens_dev, int64_t row_stride, int* lengths_dev,
                           float* scores_dev) {
  GTNX_HOST_T("batch.asg_beam_decode");
  const char* who = lm ? kAsgBeamGraph : kAsgBeam;
  // what the arguments alone decide comes first: no device is asked for an invalid call
  if (!ems) refuse(who, "null batch");
  if (!table_dev) refuse(who, "null table pointer");
  if (!tokens_dev || !lengths_dev || !scores_dev)
    refuse(who, "null output pointer (tokens, lengths and scores are all written)");
  if (row_stride < 0) refuse(who, "negative row stride");
  if (beam < 1 || beam > 64) refuse(who, "beam_size outside 1 .. 64");
  if (topn < 1 || topn > 32) refuse(who, "cutoff_top_n outside 1 .. 32");
  if (nbest < 1 || nbest > beam) refuse(who, "nbest outside 1 .. beam_size");
  LmGraphP lmg;
  if (lm) {
    if (!lm->graph) refuse(who, "null LM graph handle");
    lmg = lm_graph_lookup(lm->graph);
    if (!lmg) refuse(who, "not a live LM graph handle (destroyed, or not from gtnx_lm_graph_create)");
    if (!std::isfinite(lm->weight) || !std::isfinite(lm->bonus)) refuse(who, "lm_weight and insertion_bonus must be finite");
  }
  const int n = ems->n;
  if (n <= 0) return;
  Runtime& rt = Runtime::get();
  // there is no other route: the search runs on the slabs of a native linear batch
  if (!native_linear(*ems)) refuse(who, "not a native linear batch (gtnx_batch_linear / _rows)");
  Batch& x = *ems;
  check_frames(who, frames, n, x.M, x);
  if (row_stride < x.M) refuse(who, "row_stride is shorter than the rows of the batch");
  if (int64_t(x.M) * beam + 1 > std::numeric_limits<int>::max()) refuse(who, "rows times beam_size does not fit an int");
  // (a candidate's key keeps its label in 19 bits, above the label's place in the token set; a table of (2^19)^2
  //  entries is a terabyte)
  if (x.C > (1 << 19)) refuse(who, "more than 2^19 labels");
  // (the kernel gathers from it: host memory is refused too, with one GPU as well)
  if (!ptr_device_memory_of(table_dev, rt.device())) refuse(who, "the table is not memory of the engine's current device");
  check_outputs_local(who, {tokens_dev, lengths_dev, scores_dev});
  // (always asked, with one GPU as well: host memory handed over as the optional output is refused, not written)
  if (lm && lm->am_scores_dev && !ptr_device_memory_of(lm->am_scores_dev, rt.device()))
    refuse(who, "am_scores is not memory of the engine's current device");
  // (uploaded by the first decode that uses it; a graph that lives on another device is refused here)
  const gtnx_i4* lmg_dev = lmg ? lm_graph_device(*lmg, who) : nullptr;
  if (x.w_pend) x.w_pend->settle();  // (the values are read here: graph.h PendingCopy)
  const std::vector<int> fr = resolve_frames(frames, x);
  // algorithmic bytes.  rows: every emission of the rows that count once, topn entries and a count out.  search: those
  // back in, one 4-byte gather per (prefix, member of the set) and frame at the most, a trie node and a self-transition
  // per kept extension (at most beam per frame), the output rows; with a graph the walk of every (prefix, member) at its
  // shortest -- the state's two 16-byte words and one arc word -- and the second score.
  double row_bytes = 0, search_bytes = 0;
  for (int t : fr) {
    row_bytes += (4.0 * x.C + 8.0 * topn + 4.0) * t;
    search_bytes += (8.0 * topn + 4.0 + 12.0 * beam + 4.0 * beam * topn) * t + nbest * (4.0 * x.M + 8.0);
    if (lm) search_bytes += 48.0 * beam * topn * t + (lm->am_scores_dev ? 4.0 * nbest : 0.0);
  }
  DevMemP d_frames = upload_vec(fr);
  const size_t rows = std::max<size_t>(size_t(n) * size_t(x.M), 1);
  DevMemP entries = rt.alloc(8 * rows * size_t(topn));
  DevMemP counts = rt.alloc(sizeof(int) * rows);
  DevMemP trie = rt.alloc(8 * size_t(n) * (size_t(x.M) * size_t(beam) + 1));
  AsgBeamArgs a{};
  a.em = x.w_dev;
  a.frames = d_frames->as<int>();
  a.table = table_dev;
  a.ent_val = entries->as<float>();
  a.ent_cnt = counts->as<int>();
  a.trie = trie->as<int>();
  a.tokens = tokens_dev;
  a.lengths = lengths_dev;
  a.scores = scores_dev;
  a.row_stride = row_stride;
  a.n = n;
  a.M = x.M;
  a.C = x.C;
  a.beam = beam;
  a.topn = topn;
  a.nbest = nbest;
  if (lm) {
    a.lmg = lmg_dev;
    a.lmg_states = lmg->states;
    a.lmg_start = lmg->start;
    a.lm_weight = lm->weight;
    a.lm_bonus = lm->bonus;
    a.am_scores = lm->am_scores_dev;
  }
  {
    GTNX_PROF("asg_beam_rows", row_bytes);
    launch_asg_beam(a, 0, rt.stream());
  }
  {
    GTNX_PROF("asg_beam_search", search_bytes);
    launch_asg_beam(a, 1, rt.stream());
  }
  // (the scratch goes back to the stream-ordered pool behind the launches)
  g_asg_beam.add(1, n);
}

// ---- N sampled alignments per chain of emissions o transitions plus the merge, device-resident (asg_sample.hip) ----
namespace {
constexpr const char* kAsgSample = "gtnx_batch_asg_sample";
Counters g_asg_sample;  // (calls, utterances)
// the alpha planes of every utterance of one slice, and label and term of every (b, k, t)
constexpr ScratchCap kAsgSampleScratch{"GTNX_ASG_SAMPLE_SCRATCH_BYTES", int64_t(256) << 20};
}  // namespace

void batch_asg_sample_stats(int64_t* calls, int64_t* utterances) { g_asg_sample.get(calls, utterances); }

void batch_asg_sample(const BatchP& ems, const int* frames, const float* table_dev, int N, uint64_t seed,
                      float temperature, int* tokens_dev, int64_t row_stride, int* lengths_dev, float* logq_dev,
                      int* labels_dev, float* logz_dev) {
  GTNX_HOST_T("batch.asg_sample");
  // what the arguments alone decide comes first: no device is asked for an invalid call
  if (!ems) refuse(kAsgSample, "null batch");
  if (!table_dev) refuse(kAsgSample, "null table pointer");
  if (!tokens_dev || !lengths_dev) refuse(kAsgSample, "null output pointer (tokens and lengths are both written)");
  if (row_stride < 0) refuse(kAsgSample, "negative row stride");
  if (N < 1 || N > kAsgSampleMaxN) refuse(kAsgSample, "num_samples outside 1 .. 1024");
  if (!std::isfinite(temperature) || !(temperature > 0.0f)) refuse(kAsgSample, "temperature must be finite and above 0");
  static_assert(kAsgSampleMaxC == 1024, "the text below says 1024");
  if (ems->kind == Batch::LINEAR && (ems->C < 1 || ems->C > kAsgSampleMaxC))
    refuse(kAsgSample, "the number of labels is outside 1 .. 1024 (the filter is O(T C^2) per utterance and the draw "
                       "keeps a row in the registers of one wave)");
  Runtime& rt = Runtime::get();
  const int n = ems->n;
  // there is no other route: the sampler reads the slabs of a native linear batch
  if (!native_linear(*ems)) refuse(kAsgSample, "not a native linear batch (gtnx_batch_linear / _rows)");
  Batch& x = *ems;
  check_frames(kAsgSample, frames, n, x.M, x);
  if (n > 0 && row_stride < x.M) refuse(kAsgSample, "row_stride is shorter than the rows of the batch");
  if (int64_t(n) * N > std::numeric_limits<int>::max()) refuse(kAsgSample, "n times num_samples does not fit an int");
  if (n <= 0) return;
  // (the kernels gather from it: host memory is refused too, with one GPU as well)
  if (!ptr_device_memory_of(table_dev, rt.device())) refuse(kAsgSample, "the table is not memory of the engine's current device");
  check_outputs_local(kAsgSample, {tokens_dev, lengths_dev, logq_dev, labels_dev, logz_dev});
  if (x.w_pend) x.w_pend->settle();  // (the values are read here: graph.h PendingCopy)
  const std::vector<int> fr = resolve_frames(frames, x);
  DevMemP d_frames = upload_vec(fr);
  AsgSampleArgs a{};
  a.table = table_dev;
  a.row_stride = row_stride;
  a.label_stride = labels_dev ? row_stride : x.M;
  a.M = x.M;
  a.C = x.C;
  a.N = N;
  a.fill_labels = labels_dev ? 1 : 0;
  a.seed_lo = static_cast<unsigned>(seed & 0xffffffffu);
  a.seed_hi = static_cast<unsigned>(seed >> 32);
  a.temperature = temperature;
  // above the register variant's labels: exp(table / temperature - rowmax), transposed and padded, once per call
  const int stride = asg_sample_et_stride(x.C);
  DevMemP et, rmax;
  if (stride > 0) {
    const size_t rows4 = (size_t(x.C) + 3) & ~size_t(3);
    et = rt.alloc(sizeof(float) * rows4 * size_t(stride));
    rmax = rt.alloc(sizeof(float) * size_t(stride));
    a.et = et->as<float>();
    a.rmax = rmax->as<float>();
    GTNX_PROF("asg_sample_prep", 4.0 * x.C * x.C + 4.0 * double(rows4) * stride + 4.0 * stride);
    launch_asg_sample(a, 0, rt.stream());
  }
  // the utterances in slices whose scratch stays within the cap: the planes, the term of every (b, k, t), and its label
  // where the caller takes none
  const int64_t per_utt = 4 * int64_t(x.M) * x.C + int64_t(N) * x.M * (labels_dev ? 4 : 8);
  for_pair_slices(n, per_utt, kAsgSampleScratch, [&](int64_t b0, int64_t count) {
    // algorithmic bytes.  filter: every emission of the rows that count once, the planes out, the table once per
    // utterance (registers) or once per frame and workgroup of four utterances (L2).  draw: per (b, k, t) a plane row and a table row in,
    // label and term out.  collapse: those back in, the pad of the label rows, the token rows, length and logq.
    double fil_bytes = 0, draw_bytes = 0, col_bytes = 0;
    for (int64_t b = b0; b < b0 + count; ++b) {
      const int t = fr[size_t(b)];
      fil_bytes += 8.0 * x.C * t + (stride > 0 ? 1.0 * x.C * x.C * t : 4.0 * x.C * x.C) + 4.0;
      draw_bytes += N * t * (8.0 * x.C + 8.0);
      col_bytes += N * (8.0 * t + (labels_dev ? 4.0 * (x.M - t) : 0.0) + 4.0 * x.M + 8.0);
    }
    const size_t cells = std::max<size_t>(size_t(count) * size_t(N) * size_t(x.M), 1);
    DevMemP planes = rt.alloc(std::max<size_t>(sizeof(float) * size_t(count) * size_t(x.M) * size_t(x.C), 4));
    DevMemP terms = rt.alloc(sizeof(float) * cells);
    DevMemP labs = labels_dev ? DevMemP() : rt.alloc(sizeof(int) * cells);
    AsgSampleArgs s = a;
    s.em = x.w_dev + b0 * x.M * x.C;
    s.frames = d_frames->as<int>() + b0;
    s.planes = planes->as<float>();
    s.labels = labels_dev ? labels_dev + b0 * N * row_stride : labs->as<int>();
    s.terms = terms->as<float>();
    s.tokens = tokens_dev + b0 * N * row_stride;
    s.lengths = lengths_dev + b0 * N;
    s.logq = logq_dev ? logq_dev + b0 * N : nullptr;
    s.logz = logz_dev ? logz_dev + b0 : nullptr;
    s.n = static_cast<int>(count);
    s.b0 = static_cast<int>(b0);
    {
      GTNX_PROF("asg_sample_filter", fil_bytes);
      launch_asg_sample(s, 1, rt.stream());
    }
    {
      GTNX_PROF("asg_sample_draw", draw_bytes);
      launch_asg_sample(s, 2, rt.stream());
    }
    {
      GTNX_PROF("asg_sample_collapse", col_bytes);
      launch_asg_sample(s, 3, rt.stream());
    }
    // (the scratch goes back to the stream-ordered pool behind the launches)
  });
  g_asg_sample.add(1, n);
}

// ---- batched edit distance of device-resident token rows (edit_distance.hip) ----
namespace {
Counters g_edit_distance;  // (calls, pairs)
// the walk's scratch: a pair at the largest widths takes 64 MiB, so a slice always holds at least one pair
constexpr ScratchCap kEditDistanceScratch{"GTNX_EDIT_DISTANCE_SCRATCH_BYTES", int64_t(256) << 20};
}  // namespace

void batch_edit_distance_stats(int64_t* calls, int64_t* pairs) { g_edit_distance.get(calls, pairs); }

void batch_edit_distance(const int* hyp_dev, int64_t hyp_stride, const int* hyp_len_dev, const int* ref_dev,
                         int64_t ref_stride, const int* ref_len_dev, int B, int N, int L, int U, int* dist_dev,
                         int* ops_dev) {
  GTNX_HOST_T("batch.edit_distance");
  // what the arguments alone decide comes first: no device is asked for an invalid call
  if (!hyp_dev || !hyp_len_dev || !ref_dev || !ref_len_dev)
    throw_invalid("[gtnx_batch_edit_distance] null input pointer (hyp, hyp_lengths, ref and ref_lengths are all read)");
  if (!dist_dev) throw_invalid("[gtnx_batch_edit_distance] null dist pointer");
  if (B < 0 || N < 0 || L < 0 || U < 0) throw_invalid("[gtnx_batch_edit_distance] negative B, N, L or U");
  if (hyp_stride < 0 || ref_stride < 0) throw_invalid("[gtnx_batch_edit_distance] negative row stride");
  if (hyp_stride < L) throw_invalid("[gtnx_batch_edit_distance] hyp_stride is shorter than the rows' width L");
  if (ref_stride < U) throw_invalid("[gtnx_batch_edit_distance] ref_stride is shorter than the rows' width U");
  // (the carries of a row of columns and the reference live in LDS; a lane of the wave owns one block of 64 rows)
  if (L > kEditDistanceMaxL) throw_invalid("[gtnx_batch_edit_distance] L above 65536");
  if (U > kEditDistanceMaxU) throw_invalid("[gtnx_batch_edit_distance] U above 4096");
  const int64_t pairs = int64_t(B) * N;
  if (pairs > std::numeric_limits<int>::max()) throw_invalid("[gtnx_batch_edit_distance] B times N does not fit an int");
  if (pairs == 0) return;
  Runtime& rt = Runtime::get();
  check_outputs_local("gtnx_batch_edit_distance", {dist_dev, ops_dev});
  const int nbU = (U + 63) / 64;
  EditDistanceArgs a{};
  a.hyp = hyp_dev;
  a.hyp_len = hyp_len_dev;
  a.ref = ref_dev;
  a.ref_len = ref_len_dev;
  a.dist = dist_dev;
  a.ops = ops_dev;
  a.hyp_stride = hyp_stride;
  a.ref_stride = ref_stride;
  a.N = N;
  a.L = L;
  a.U = U;
  a.nbU = nbU;
  // algorithmic bytes, by the widths (the lengths are device memory: an upper bound): every token and length once, the
  // distance out; with ops the (Pv, Mv) words of every (column, block) out and back in, and the three counts
  const double io_bytes = double(pairs) * (4.0 * L + 8.0) + double(B) * (4.0 * U + 4.0);
  if (!ops_dev) {
    a.pair0 = 0;
    a.count = int(pairs);
    GTNX_PROF("edit_distance", io_bytes);
    launch_edit_distance(a, rt.stream());
  } else {
    const int64_t per_pair = int64_t(16) * L * nbU;
    for_pair_slices(pairs, per_pair, kEditDistanceScratch, [&](int64_t p0, int64_t cnt) {
      DevMemP words = rt.alloc(size_t(std::max<int64_t>(per_pair * cnt, 16)));
      a.scratch = words->as<gtnx_ul2>();
      a.pair0 = p0;
      a.count = int(cnt);
      GTNX_PROF("edit_distance_ops", (io_bytes / double(pairs) + 2.0 * double(per_pair) + 12.0) * double(cnt));
      launch_edit_distance(a, rt.stream());
      // (the words go back to the stream-ordered pool behind the launch)
    });
  }
  g_edit_distance.add(1, pairs);
}

// ---- batched CTC score of device-resident hypotheses, and its gradient (ctc_score.hip) ----
namespace {
Counters g_ctc_score;  // (calls, pairs)
// the alpha rows of a gradient call: a pair that is above the cap by itself runs alone with scratch of its own size
constexpr ScratchCap kCtcScoreScratch{"GTNX_CTC_SCORE_SCRATCH_BYTES", int64_t(256) << 20};

// both entry points: scores_dev for the score, weights_dev and grad_dev for the gradient
void ctc_score_impl(const char* who, const BatchP& ems, const int* frames, int blank, const Hypotheses& h,
                    float* scores_dev, const float* weights_dev, float* grad_dev) {
  const bool want_grad = scores_dev == nullptr;
  // what the arguments alone decide comes first: no device is asked for an invalid call
  if (want_grad && (!weights_dev || !grad_dev)) refuse(who, "null weights or grad pointer");
  if (blank < 0) refuse(who, "negative blank");
  const int64_t pairs = check_hypotheses(who, ems, h);
  if (pairs <= 0) return;
  Batch& x = linear_hypothesis_batch(who, ems, frames);
  if (blank >= x.C) refuse(who, "blank is not below the number of labels");
  check_outputs_local(who, {want_grad ? grad_dev : scores_dev});
  Runtime& rt = Runtime::get();
  CtcScoreArgs a{};
  const PairFrames fr = settle_frames(x, frames, h, a);
  const int N = h.N, L = h.L, U = h.max_length;
  const int64_t SM = 2 * int64_t(U) + 1;
  a.weights = weights_dev;
  a.grad = grad_dev;
  a.blank = blank;
  // algorithmic bytes, by the widths (the lengths are device memory: an upper bound).  forward: per pair and frame one
  // emission per state, the tokens and the length once, the score out.  With the rows kept: every alpha out as well.
  // backward: the alphas and the emissions back in, one load and one store of a gradient element per state and frame
  // at most, the tokens and the length, and the utterance's slab zeroed once.
  const double per_pair_frames = fr.mean;
  const double fwd_pair = 4.0 * double(SM) * per_pair_frames + 4.0 * std::min(L, U) + 8.0;
  if (!want_grad) {
    a.scores = scores_dev;
    a.pair0 = 0;
    a.score0 = 0;
    a.count = int(pairs);
    GTNX_PROF("ctc_score", fwd_pair * double(pairs));
    launch_ctc_score_forward(a, rt.stream());
  } else {
    const int64_t per_pair = std::max<int64_t>(int64_t(fr.maxT), 1) * SM;  // floats
    a.pair_stride = per_pair;
    for_pair_slices(pairs, 4 * per_pair, kCtcScoreScratch, [&](int64_t p0, int64_t cnt) {
      DevMemP rows = rt.alloc(size_t(4 * per_pair * cnt));
      DevMemP sc = rt.alloc(size_t(4 * cnt));
      a.alpha = rows->as<float>();
      a.scores = sc->as<float>();
      a.pair0 = p0;
      a.score0 = p0;
      a.count = int(cnt);
      {
        GTNX_PROF("ctc_score_alpha", 2.0 * fwd_pair * double(cnt));
        launch_ctc_score_forward(a, rt.stream());
      }
      {
        GTNX_PROF("ctc_score_grad", (4.0 * fwd_pair + 4.0 * double(x.M) * x.C / double(N)) * double(cnt));
        launch_ctc_score_backward(a, rt.stream());
      }
      // (the rows go back to the stream-ordered pool behind the launches)
    });
  }
  g_ctc_score.add(1, pairs);
}
}  // namespace

void batch_ctc_score_stats(int64_t* calls, int64_t* pairs) { g_ctc_score.get(calls, pairs); }

void batch_ctc_score(const BatchP& ems, const int* frames, int blank, const int* tokens_dev, int64_t row_stride,
                     const int* lengths_dev, int N, int L, int max_length, float* scores_dev) {
  GTNX_HOST_T("batch.ctc_score");
  if (!scores_dev) throw_invalid("[gtnx_batch_ctc_score] null scores pointer");
  ctc_score_impl("gtnx_batch_ctc_score", ems, frames, blank, {tokens_dev, row_stride, lengths_dev, N, L, max_length},
                 scores_dev, nullptr, nullptr);
}

void batch_ctc_score_grad(const BatchP& ems, const int* frames, int blank, const int* tokens_dev, int64_t row_stride,
                          const int* lengths_dev, int N, int L, int max_length, const float* weights_dev,
                          float* grad_dev) {
  GTNX_HOST_T("batch.ctc_score_grad");
  ctc_score_impl("gtnx_batch_ctc_score_grad", ems, frames, blank,
                 {tokens_dev, row_stride, lengths_dev, N, L, max_length}, nullptr, weights_dev, grad_dev);
}

// ---- batched CTC score of one device-resident token lattice per utterance, and its gradients (ctc_lattice.hip) ----
namespace {
Counters g_ctc_lattice;  // (calls, utterances)
// the alpha rows of a gradient call: an utterance that is above the cap by itself runs alone with scratch of its own size
constexpr ScratchCap kCtcLatticeScratch{"GTNX_CTC_LATTICE_SCRATCH_BYTES", int64_t(256) << 20};
static_assert(kCtcLatticeMaxStates == 4096, "the text below says 4096");

struct Lattices {
  const int* arcs;
  int64_t row_stride;
  const int *num_arcs, *num_nodes;
  const float* arc_weights;
  int A, max_states;
};

// both entry points: scores_dev for the score; weights_dev, grad_dev and arc_grad_dev (or null) for the gradients
void ctc_lattice_impl(const char* who, const BatchP& ems, const int* frames, int blank, const Lattices& h,
                      float* scores_dev, const float* weights_dev, float* grad_dev, float* arc_grad_dev) {
  const bool want_grad = scores_dev == nullptr;
  // what the arguments alone decide comes first: no device is asked for an invalid call
  if (!ems) refuse(who, "null batch");
  if (!h.arcs || !h.num_arcs || !h.num_nodes)
    refuse(who, "null input pointer (arcs, num_arcs and num_nodes are all read)");
  if (want_grad && (!weights_dev || !grad_dev)) refuse(who, "null weights or grad pointer");
  if (blank < 0) refuse(who, "negative blank");
  if (h.A < 0) refuse(who, "negative A");
  if (h.row_stride < 3 * int64_t(h.A)) refuse(who, "row_stride is shorter than the rows' width 3 A");
  if (h.max_states < 1 || h.max_states > kCtcLatticeMaxStates) refuse(who, "max_states outside 1 .. 4096");
  const int n = ems->n;
  if (n <= 0) return;
  Batch& x = linear_hypothesis_batch(who, ems, frames);
  if (blank >= x.C) refuse(who, "blank is not below the number of labels");
  check_outputs_local(who, {want_grad ? grad_dev : scores_dev, arc_grad_dev});
  Runtime& rt = Runtime::get();
  if (x.w_pend) x.w_pend->settle();  // (the values are read here: graph.h PendingCopy)
  const std::vector<int> fr = resolve_frames(frames, x);
  int maxT = 0;
  double sumT = 0;
  for (int t : fr) {
    maxT = std::max(maxT, t);
    sumT += t;
  }
  DevMemP fr_dev = upload_vec(fr);
  const int64_t SM = h.max_states;
  CtcLatticeArgs a{};
  a.em = x.w_dev;
  a.frames = fr_dev->as<int>();
  a.arcs = h.arcs;
  a.num_arcs = h.num_arcs;
  a.num_nodes = h.num_nodes;
  a.arc_weights = h.arc_weights;
  a.weights = weights_dev;
  a.grad = grad_dev;
  a.arc_grad = arc_grad_dev;
  a.row_stride = h.row_stride;
  a.A = h.A;
  a.SM = h.max_states;
  a.M = x.M;
  a.C = x.C;
  a.blank = blank;
  // algorithmic bytes, by the widths (the counts are device memory: an upper bound).  forward: per utterance and frame
  // one emission per state, the arcs (and their weights) once, the score out.  With the rows kept: every alpha out as
  // well.  backward: the alphas and the emissions back in, one store of a gradient element per state and frame at most,
  // the arcs again, the slab zeroed once, the arcs' gradient out.
  const int64_t states = std::min<int64_t>(SM, int64_t(h.A) + SM);
  const double lattice = (h.arc_weights ? 16.0 : 12.0) * std::min<int64_t>(h.A, SM) + 12.0;
  const double fwd_utt = 4.0 * double(states) * (sumT / double(n)) + lattice;
  if (!want_grad) {
    a.scores = scores_dev;
    a.utt0 = 0;
    a.score0 = 0;
    a.count = n;
    GTNX_PROF("ctc_lattice", fwd_utt * double(n));
    launch_ctc_lattice_forward(a, rt.stream());
  } else {
    const int64_t per_utt = std::max<int64_t>(int64_t(maxT), 1) * SM;  // floats
    a.utt_stride = per_utt;
    for_pair_slices(n, 4 * per_utt, kCtcLatticeScratch, [&](int64_t u0, int64_t cnt) {
      DevMemP rows = rt.alloc(size_t(4 * per_utt * cnt));
      DevMemP sc = rt.alloc(size_t(4 * cnt));
      a.alpha = rows->as<float>();
      a.scores = sc->as<float>();
      a.utt0 = int(u0);
      a.score0 = int(u0);
      a.count = int(cnt);
      {
        GTNX_PROF("ctc_lattice_alpha", 2.0 * fwd_utt * double(cnt));
        launch_ctc_lattice_forward(a, rt.stream());
      }
      {
        GTNX_PROF("ctc_lattice_grad", (3.0 * fwd_utt + 4.0 * double(x.M) * x.C + (arc_grad_dev ? 4.0 * h.A : 0.0)) * double(cnt));
        launch_ctc_lattice_backward(a, rt.stream());
      }
      // (the rows go back to the stream-ordered pool behind the launches)
    });
  }
  g_ctc_lattice.add(1, n);
}
}  // namespace

void batch_ctc_lattice_score_stats(int64_t* calls, int64_t* utterances) { g_ctc_lattice.get(calls, utterances); }

void batch_ctc_lattice_score(const BatchP& ems, const int* frames, int blank, const int* arcs_dev, int64_t row_stride,
                             const int* num_arcs_dev, const int* num_nodes_dev, const float* arc_weights_dev, int A,
                             int max_states, float* scores_dev) {
  GTNX_HOST_T("batch.ctc_lattice_score");
  if (!scores_dev) throw_invalid("[gtnx_batch_ctc_lattice_score] null scores pointer");
  ctc_lattice_impl("gtnx_batch_ctc_lattice_score", ems, frames, blank,
                   {arcs_dev, row_stride, num_arcs_dev, num_nodes_dev, arc_weights_dev, A, max_states}, scores_dev,
                   nullptr, nullptr, nullptr);
}

void batch_ctc_lattice_score_grad(const BatchP& ems, const int* frames, int blank, const int* arcs_dev,
                                  int64_t row_stride, const int* num_arcs_dev, const int* num_nodes_dev,
                                  const float* arc_weights_dev, int A, int max_states, const float* weights_dev,
                                  float* grad_dev, float* arc_grad_dev) {
  GTNX_HOST_T("batch.ctc_lattice_score_grad");
  ctc_lattice_impl("gtnx_batch_ctc_lattice_score_grad", ems, frames, blank,
                   {arcs_dev, row_stride, num_arcs_dev, num_nodes_dev, arc_weights_dev, A, max_states}, nullptr,
                   weights_dev, grad_dev, arc_grad_dev);
}

// ---- batched CTC Viterbi alignment of one device-resident token lattice per utterance (ctc_lattice_align.hip) ----
namespace {
constexpr const char* kCtcLatticeAlign = "gtnx_batch_ctc_lattice_align";
Counters g_ctc_lattice_align;  // (calls, utterances)
// the back-pointers: an utterance that is above the cap by itself runs alone with scratch of its own size
constexpr ScratchCap kCtcLatticeAlignScratch{"GTNX_CTC_LATTICE_ALIGN_SCRATCH_BYTES", int64_t(256) << 20};
}  // namespace

void batch_ctc_lattice_align_stats(int64_t* calls, int64_t* utterances) { g_ctc_lattice_align.get(calls, utterances); }

void batch_ctc_lattice_align(const BatchP& ems, const int* frames, int blank, const int* arcs_dev, int64_t row_stride,
                             const int* num_arcs_dev, const int* num_nodes_dev, const float* arc_weights_dev, int A,
                             int max_states, float* scores_dev, int* path_len_dev, int* path_arcs_dev,
                             int* path_tokens_dev, int* starts_dev, int* ends_dev, float* token_scores_dev, int P,
                             int64_t out_stride, int* frame_arcs_dev, int64_t frame_stride) {
  GTNX_HOST_T("batch.ctc_lattice_align");
  const char* who = kCtcLatticeAlign;
  // what the arguments alone decide comes first: no device is asked for an invalid call
  if (!ems) refuse(who, "null batch");
  if (!arcs_dev || !num_arcs_dev || !num_nodes_dev)
    refuse(who, "null input pointer (arcs, num_arcs and num_nodes are all read)");
  if (!scores_dev || !path_len_dev || !path_arcs_dev || !path_tokens_dev || !starts_dev || !ends_dev)
    refuse(who, "null output pointer (scores, path_len, path_arcs, path_tokens, starts and ends are all written)");
  if (blank < 0) refuse(who, "negative blank");
  if (A < 0) refuse(who, "negative A");
  if (row_stride < 3 * int64_t(A)) refuse(who, "row_stride is shorter than the rows' width 3 A");
  if (max_states < 1 || max_states > kCtcLatticeMaxStates) refuse(who, "max_states outside 1 .. 4096");
  if (P < 1) refuse(who, "P below 1");
  if (out_stride < P) refuse(who, "out_stride is shorter than the rows' width P");
  const int n = ems->n;
  if (n <= 0) return;
  Batch& x = linear_hypothesis_batch(who, ems, frames);
  if (blank >= x.C) refuse(who, "blank is not below the number of labels");
  if (frame_arcs_dev && frame_stride < x.M) refuse(who, "frame_stride is shorter than the rows of the batch");
  check_outputs_local(who, {scores_dev, path_len_dev, path_arcs_dev, path_tokens_dev, starts_dev, ends_dev,
                            token_scores_dev, frame_arcs_dev});
  Runtime& rt = Runtime::get();
  if (x.w_pend) x.w_pend->settle();  // (the values are read here: graph.h PendingCopy)
  const std::vector<int> fr = resolve_frames(frames, x);
  int maxT = 0;
  double sumT = 0;
  for (int t : fr) {
    maxT = std::max(maxT, t);
    sumT += t;
  }
  DevMemP fr_dev = upload_vec(fr);
  const int64_t SM = max_states;
  CtcLatticeAlignArgs a{};
  a.em = x.w_dev;
  a.frames = fr_dev->as<int>();
  a.arcs = arcs_dev;
  a.num_arcs = num_arcs_dev;
  a.num_nodes = num_nodes_dev;
  a.arc_weights = arc_weights_dev;
  a.scores = scores_dev;
  a.path_len = path_len_dev;
  a.path_arcs = path_arcs_dev;
  a.path_tokens = path_tokens_dev;
  a.starts = starts_dev;
  a.ends = ends_dev;
  a.token_scores = token_scores_dev;
  a.frame_arcs = frame_arcs_dev;
  a.row_stride = row_stride;
  a.out_stride = out_stride;
  a.frame_stride = frame_stride;
  a.A = A;
  a.SM = max_states;
  a.P = P;
  a.M = x.M;
  a.C = x.C;
  a.blank = blank;
  // algorithmic bytes, by the widths (the counts are device memory: an upper bound).  Per utterance and frame one
  // emission per state in and 2 bytes per state out; the walk reads one back-pointer per frame; the arcs (and their
  // weights) once, the score and the length out, the four path rows; with token scores one emission per frame at most
  // and the row; with frame arcs the row.
  const double frames_utt = sumT / double(n);
  const double lattice = (arc_weights_dev ? 16.0 : 12.0) * std::min<int64_t>(A, SM) + 12.0;
  const double utt_bytes = (4.0 + 2.0) * double(SM) * frames_utt + 2.0 * frames_utt + lattice + 8.0 + 16.0 * P +
                           (token_scores_dev ? 4.0 * frames_utt + 4.0 * P : 0.0) + (frame_arcs_dev ? 4.0 * x.M : 0.0);
  const int64_t per_utt = std::max<int64_t>(int64_t(maxT), 1) * SM;  // 16-bit entries
  a.utt_stride = per_utt;
  for_pair_slices(n, 2 * per_utt, kCtcLatticeAlignScratch, [&](int64_t u0, int64_t cnt) {
    DevMemP ptrs = rt.alloc(size_t(2 * per_utt * cnt));
    a.bp = ptrs->as<unsigned short>();
    a.utt0 = int(u0);
    a.count = int(cnt);
    GTNX_PROF("ctc_lattice_align", utt_bytes * double(cnt));
    launch_ctc_lattice_align(a, rt.stream());
    // (the back-pointers go back to the stream-ordered pool behind the launch)
  });
  g_ctc_lattice_align.add(1, n);
}

// ---- batched CTC token alignment of device-resident hypotheses (ctc_token_align.hip) ----
namespace {
constexpr const char* kCtcTokenAlign = "gtnx_batch_ctc_token_align";
Counters g_ctc_token_align;  // (calls, pairs)
// the back-pointer words: a pair that is above the cap by itself runs alone with scratch of its own size
constexpr ScratchCap kCtcTokenAlignScratch{"GTNX_CTC_TOKEN_ALIGN_SCRATCH_BYTES", int64_t(256) << 20};
}  // namespace

void batch_ctc_token_align_stats(int64_t* calls, int64_t* pairs) { g_ctc_token_align.get(calls, pairs); }

void batch_ctc_token_align(const BatchP& ems, const int* frames, int blank, const int* tokens_dev, int64_t row_stride,
                           const int* lengths_dev, int N, int L, int max_length, float* scores_dev, int* starts_dev,
                           int* ends_dev, float* token_scores_dev, int64_t out_stride, int* frame_tokens_dev,
                           int64_t frame_stride) {
  GTNX_HOST_T("batch.ctc_token_align");
  const char* who = kCtcTokenAlign;
  const Hypotheses h{tokens_dev, row_stride, lengths_dev, N, L, max_length};
  // what the arguments alone decide comes first: no device is asked for an invalid call
  if (!scores_dev || !starts_dev || !ends_dev) refuse(who, "null output pointer (scores, starts and ends are all written)");
  if (out_stride < 0 || frame_stride < 0) refuse(who, "negative row stride");
  if (blank < 0) refuse(who, "negative blank");
  if (out_stride < L) refuse(who, "out_stride is shorter than the rows' width L");
  const int64_t pairs = check_hypotheses(who, ems, h);
  if (pairs <= 0) return;
  Batch& x = linear_hypothesis_batch(who, ems, frames);
  if (blank >= x.C) refuse(who, "blank is not below the number of labels");
  if (frame_tokens_dev && frame_stride < x.M) refuse(who, "frame_stride is shorter than the rows of the batch");
  check_outputs_local(who, {scores_dev, starts_dev, ends_dev, token_scores_dev, frame_tokens_dev});
  Runtime& rt = Runtime::get();
  CtcTokenAlignArgs a{};
  const PairFrames fr = settle_frames(x, frames, h, a);
  const int U = max_length;
  const int64_t SM = 2 * int64_t(U) + 1;
  a.scores = scores_dev;
  a.starts = starts_dev;
  a.ends = ends_dev;
  a.token_scores = token_scores_dev;
  a.frame_tokens = frame_tokens_dev;
  a.out_stride = out_stride;
  a.frame_stride = frame_stride;
  a.blank = blank;
  // algorithmic bytes, by the widths (the lengths are device memory: an upper bound).  Per pair and frame one emission
  // per state and 2 bits per state out; the walk reads one window of 128 words per 16 frames; the tokens and the length
  // once, the score and the two span rows out; with token scores one emission per frame at most and the row; with
  // frame tokens the row.
  const double per_pair_frames = fr.mean;
  const double pair_bytes = (4.0 + 0.25) * double(SM) * per_pair_frames + 32.0 * per_pair_frames + 4.0 * std::min(L, U) +
                            8.0 + 8.0 * L + (token_scores_dev ? 4.0 * per_pair_frames + 4.0 * L : 0.0) +
                            (frame_tokens_dev ? 4.0 * x.M : 0.0);
  const int64_t per_pair = (std::max<int64_t>(int64_t(fr.maxT), 1) + 15) / 16 * SM;  // words
  a.pair_stride = per_pair;
  for_pair_slices(pairs, 4 * per_pair, kCtcTokenAlignScratch, [&](int64_t p0, int64_t cnt) {
    DevMemP words = rt.alloc(size_t(4 * per_pair * cnt));
    a.bp = words->as<unsigned>();
    a.pair0 = p0;
    a.count = int(cnt);
    GTNX_PROF("ctc_token_align", pair_bytes * double(cnt));
    launch_ctc_token_align(a, rt.stream());
    // (the words go back to the stream-ordered pool behind the launch)
  });
  g_ctc_token_align.add(1, pairs);
}

// ---- batched ASG score of device-resident hypotheses, and its gradients (asg_score.hip) ----
namespace {
Counters g_asg_score;  // (calls, pairs)
// the alpha rows of a gradient call: a pair that is above the cap by itself runs alone with scratch of its own size
constexpr ScratchCap kAsgScoreScratch{"GTNX_ASG_SCORE_SCRATCH_BYTES", int64_t(256) << 20};

// both entry points: scores_dev for the score; weights_dev and grad_em_dev / grad_table_dev for the gradients
void asg_score_impl(const char* who, const BatchP& ems, const int* frames, const float* table_dev, const Hypotheses& h,
                    float* scores_dev, const float* weights_dev, float* grad_em_dev, float* grad_table_dev) {
  const bool want_grad = scores_dev == nullptr;
  // what the arguments alone decide comes first: no device is asked for an invalid call
  if (!table_dev) refuse(who, "null table pointer");
  if (want_grad && !weights_dev) refuse(who, "null weights pointer");
  if (want_grad && !grad_em_dev && !grad_table_dev) refuse(who, "neither gradient asked for (both pointers null)");
  const int64_t pairs = check_hypotheses(who, ems, h);
  if (pairs <= 0) return;
  Batch& x = linear_hypothesis_batch(who, ems, frames);
  Runtime& rt = Runtime::get();
  // (the table kernel keeps one row of C floats in LDS)
  if (x.C > kAsgScoreMaxC) refuse(who, "more than 16384 labels");
  // (the kernel gathers from it: host memory is refused too, with one GPU as well)
  if (!ptr_device_memory_of(table_dev, rt.device())) refuse(who, "the table is not memory of the engine's current device");
  check_outputs_local(who, {scores_dev, grad_em_dev, grad_table_dev});
  AsgScoreArgs a{};
  const PairFrames fr = settle_frames(x, frames, h, a);
  const int N = h.N, L = h.L, U = h.max_length;
  a.table = table_dev;
  a.weights = weights_dev;
  a.grad = grad_em_dev;
  a.grad_table = grad_table_dev;
  a.pairs = int(pairs);
  a.occ_half = std::max(std::min(L, U), 1);
  // algorithmic bytes, by the widths (the lengths are device memory: an upper bound).  forward: per pair and frame one
  // emission per position, the tokens, two table entries per position and the length once, the score out.  With the
  // rows kept: every alpha out as well.  backward: the alphas (twice: a position and the one before it) and the
  // emissions back in, with an emission gradient the occupancies out in the alphas' place; the occupancy sums out.
  // scatter: the occupancies back in, one load and one store of a gradient element per position and frame at most,
  // and the utterance's slab zeroed once.  table: every workgroup streams the tokens, the sums come back in once, the
  // table goes out.
  const double per_pair_frames = fr.mean;
  const double width = std::min(L, U);
  const double fwd_pair = 4.0 * double(U) * per_pair_frames + 12.0 * width + 8.0;
  if (!want_grad) {
    a.scores = scores_dev;
    a.pair0 = 0;
    a.score0 = 0;
    a.count = int(pairs);
    GTNX_PROF("asg_score", fwd_pair * double(pairs));
    launch_asg_score_forward(a, rt.stream());
  } else {
    const int64_t per_pair = std::max<int64_t>(int64_t(fr.maxT), 1) * U;  // floats
    // (the scores and the occupancy sums outlive the slices: the table launch reads them)
    DevMemP sc = rt.alloc(size_t(4 * pairs));
    DevMemP occ;
    if (grad_table_dev) {
      occ = rt.alloc(size_t(8) * size_t(a.occ_half) * size_t(pairs));
      a.occ = occ->as<float>();
    }
    a.scores = sc->as<float>();
    a.score0 = 0;
    a.pair_stride = per_pair;
    for_pair_slices(pairs, 4 * per_pair, kAsgScoreScratch, [&](int64_t p0, int64_t cnt) {
      DevMemP rows = rt.alloc(size_t(4 * per_pair * cnt));
      a.alpha = rows->as<float>();
      a.pair0 = p0;
      a.count = int(cnt);
      {
        GTNX_PROF("asg_score_alpha", 2.0 * fwd_pair * double(cnt));
        launch_asg_score_forward(a, rt.stream());
      }
      {
        GTNX_PROF("asg_score_grad", ((grad_em_dev ? 4.0 : 3.0) * fwd_pair + (grad_table_dev ? 8.0 * width : 0.0)) *
                                        double(cnt));
        launch_asg_score_backward(a, rt.stream());
      }
      if (grad_em_dev) {
        GTNX_PROF("asg_score_scatter", (3.0 * fwd_pair + 4.0 * double(x.M) * x.C / double(N)) * double(cnt));
        launch_asg_score_scatter(a, rt.stream());
      }
      // (the rows go back to the stream-ordered pool behind the launches)
    });
    if (grad_table_dev) {
      GTNX_PROF("asg_score_table", (4.0 * width * double(x.C + 1) + 8.0 * width + 12.0) * double(pairs) +
                                       4.0 * double(x.C) * double(x.C + 1));
      launch_asg_score_table(a, rt.stream());
    }
  }
  g_asg_score.add(1, pairs);
}
}  // namespace

void batch_asg_score_stats(int64_t* calls, int64_t* pairs) { g_asg_score.get(calls, pairs); }

void batch_asg_score(const BatchP& ems, const int* frames, const float* table_dev, const int* tokens_dev,
                     int64_t row_stride, const int* lengths_dev, int N, int L, int max_length, float* scores_dev) {
  GTNX_HOST_T("batch.asg_score");
  if (!scores_dev) throw_invalid("[gtnx_batch_asg_score] null scores pointer");
  asg_score_impl("gtnx_batch_asg_score", ems, frames, table_dev, {tokens_dev, row_stride, lengths_dev, N, L, max_length},
                 scores_dev, nullptr, nullptr, nullptr);
}

void batch_asg_score_grad(const BatchP& ems, const int* frames, const float* table_dev, const int* tokens_dev,
                          int64_t row_stride, const int* lengths_dev, int N, int L, int max_length,
                          const float* weights_dev, float* grad_em_dev, float* grad_table_dev) {
  GTNX_HOST_T("batch.asg_score_grad");
  asg_score_impl("gtnx_batch_asg_score_grad", ems, frames, table_dev,
                 {tokens_dev, row_stride, lengths_dev, N, L, max_length}, nullptr, weights_dev, grad_em_dev, grad_table_dev);
}

// ---- batched ASG score of one device-resident token lattice per utterance, and its gradients (asg_lattice.hip) ----
namespace {
Counters g_asg_lattice;  // (calls, utterances)
// the alpha rows and the edge rows of a gradient call: an utterance that is above the cap by itself runs alone
constexpr ScratchCap kAsgLatticeScratch{"GTNX_ASG_LATTICE_SCRATCH_BYTES", int64_t(256) << 20};
static_assert(kAsgLatticeMaxStates == 4096 && kAsgLatticeMaxEdges == 1 << 21, "the text below says 4096 and 2^21");

// both entry points: scores_dev for the score; weights_dev and the three gradients (each or null) for the gradients
void asg_lattice_impl(const char* who, const BatchP& ems, const int* frames, const float* table_dev, const Lattices& h,
                      int max_edges, float* scores_dev, const float* weights_dev, float* grad_em_dev,
                      float* grad_table_dev, float* arc_grad_dev) {
  const bool want_grad = scores_dev == nullptr;
  // what the arguments alone decide comes first: no device is asked for an invalid call
  if (!ems) refuse(who, "null batch");
  if (!table_dev) refuse(who, "null table pointer");
  if (!h.arcs || !h.num_arcs || !h.num_nodes)
    refuse(who, "null input pointer (arcs, num_arcs and num_nodes are all read)");
  if (want_grad && !weights_dev) refuse(who, "null weights pointer");
  if (want_grad && !grad_em_dev && !grad_table_dev && !arc_grad_dev)
    refuse(who, "no gradient asked for (all three pointers null)");
  if (h.A < 0) refuse(who, "negative A");
  if (h.row_stride < 3 * int64_t(h.A)) refuse(who, "row_stride is shorter than the rows' width 3 A");
  if (h.max_states < 1 || h.max_states > kAsgLatticeMaxStates) refuse(who, "max_states outside 1 .. 4096");
  if (max_edges < 1 || max_edges > kAsgLatticeMaxEdges) refuse(who, "max_edges outside 1 .. 2^21");
  const int n = ems->n;
  if (n <= 0) return;
  Batch& x = linear_hypothesis_batch(who, ems, frames);
  Runtime& rt = Runtime::get();
  // (the table kernel keeps one row of C floats in LDS)
  if (x.C > kAsgScoreMaxC) refuse(who, "more than 16384 labels");
  // (the kernel gathers from it: host memory is refused too, with one GPU as well)
  if (!ptr_device_memory_of(table_dev, rt.device())) refuse(who, "the table is not memory of the engine's current device");
  check_outputs_local(who, {scores_dev, grad_em_dev, grad_table_dev, arc_grad_dev});
  if (x.w_pend) x.w_pend->settle();  // (the values are read here: graph.h PendingCopy)
  const std::vector<int> fr = resolve_frames(frames, x);
  int maxT = 0;
  double sumT = 0;
  for (int t : fr) {
    maxT = std::max(maxT, t);
    sumT += t;
  }
  DevMemP fr_dev = upload_vec(fr);
  const int64_t SM = h.max_states;
  AsgLatticeArgs a{};
  a.em = x.w_dev;
  a.frames = fr_dev->as<int>();
  a.table = table_dev;
  a.arcs = h.arcs;
  a.num_arcs = h.num_arcs;
  a.num_nodes = h.num_nodes;
  a.arc_weights = h.arc_weights;
  a.weights = weights_dev;
  a.grad = grad_em_dev;
  a.grad_table = grad_table_dev;
  a.arc_grad = arc_grad_dev;
  a.row_stride = h.row_stride;
  a.A = h.A;
  a.SM = h.max_states;
  a.M = x.M;
  a.C = x.C;
  a.max_edges = max_edges;
  // algorithmic bytes, by the widths and the caller's bounds (the counts are device memory: an upper bound).  forward:
  // per utterance and frame one emission per arc and one table entry per edge, the arcs (and their weights) once, the
  // score out.  With the rows kept: every alpha out as well.  backward: the alphas and the emissions back in, two table
  // entries per edge and frame, an edge cell in and out per frame, one store of a gradient element per arc and frame at
  // most, the slab zeroed once.  table: every workgroup streams the labels, the sums come back in once, the table out.
  const int64_t arcs_max = std::min<int64_t>(h.A, SM);
  const double mean_t = sumT / double(n);
  const double lattice = (h.arc_weights ? 16.0 : 12.0) * double(arcs_max) + 12.0;
  const double fwd_utt = 4.0 * (double(arcs_max) + double(max_edges)) * mean_t + lattice;
  if (!want_grad) {
    a.scores = scores_dev;
    a.utt0 = 0;
    a.score0 = 0;
    a.count = n;
    GTNX_PROF("asg_lattice", fwd_utt * double(n));
    launch_asg_lattice_forward(a, rt.stream());
  } else {
    const bool want_edges = grad_table_dev || arc_grad_dev;
    const int64_t alpha_utt = std::max<int64_t>(int64_t(maxT), 1) * SM;  // floats
    const int64_t per_utt = alpha_utt + (want_edges ? int64_t(max_edges) : 0) + (grad_table_dev ? 5 * SM : 0);
    a.utt_stride = alpha_utt;
    a.table_first = 1;
    for_pair_slices(n, 4 * per_utt, kAsgLatticeScratch, [&](int64_t u0, int64_t cnt) {
      DevMemP rows = rt.alloc(size_t(4 * alpha_utt * cnt));
      DevMemP sc = rt.alloc(size_t(4 * cnt));
      DevMemP edges, occ, csr;
      if (want_edges) {
        edges = rt.alloc(size_t(4) * size_t(max_edges) * size_t(cnt));
        a.edge = edges->as<float>();
      }
      if (grad_table_dev) {
        occ = rt.alloc(size_t(8 * SM * cnt));
        csr = rt.alloc(size_t(12 * SM * cnt));
        a.occ = occ->as<float>();
        a.csr = csr->as<int>();
      }
      a.alpha = rows->as<float>();
      a.scores = sc->as<float>();
      a.utt0 = int(u0);
      a.score0 = int(u0);
      a.count = int(cnt);
      {
        GTNX_PROF("asg_lattice_alpha", (fwd_utt + 4.0 * double(arcs_max) * mean_t) * double(cnt));
        launch_asg_lattice_forward(a, rt.stream());
      }
      {
        GTNX_PROF("asg_lattice_grad", (2.0 * fwd_utt + (want_edges ? 8.0 * double(max_edges) * mean_t : 0.0) +
                                       (grad_em_dev ? 4.0 * double(x.M) * x.C : 0.0) + (arc_grad_dev ? 4.0 * h.A : 0.0)) *
                                          double(cnt));
        launch_asg_lattice_backward(a, rt.stream());
      }
      if (grad_table_dev) {
        GTNX_PROF("asg_lattice_table", (4.0 * double(arcs_max) * double(x.C + 1) + 8.0 * double(max_edges)) * double(cnt) +
                                           8.0 * double(x.C) * double(x.C + 1));
        launch_asg_lattice_table(a, rt.stream());
        a.table_first = 0;
      }
      // (the rows go back to the stream-ordered pool behind the launches)
    });
  }
  g_asg_lattice.add(1, n);
}
}  // namespace

void batch_asg_lattice_score_stats(int64_t* calls, int64_t* utterances) { g_asg_lattice.get(calls, utterances); }

void batch_asg_lattice_score(const BatchP& ems, const int* frames, const float* table_dev, const int* arcs_dev,
                             int64_t row_stride, const int* num_arcs_dev, const int* num_nodes_dev,
                             const float* arc_weights_dev, int A, int max_states, int max_edges, float* scores_dev) {
  GTNX_HOST_T("batch.asg_lattice_score");
  if (!scores_dev) throw_invalid("[gtnx_batch_asg_lattice_score] null scores pointer");
  asg_lattice_impl("gtnx_batch_asg_lattice_score", ems, frames, table_dev,
                   {arcs_dev, row_stride, num_arcs_dev, num_nodes_dev, arc_weights_dev, A, max_states}, max_edges,
                   scores_dev, nullptr, nullptr, nullptr, nullptr);
}

void batch_asg_lattice_score_grad(const BatchP& ems, const int* frames, const float* table_dev, const int* arcs_dev,
                                  int64_t row_stride, const int* num_arcs_dev, const int* num_nodes_dev,
                                  const float* arc_weights_dev, int A, int max_states, int max_edges,
                                  const float* weights_dev, float* grad_em_dev, float* grad_table_dev,
                                  float* arc_grad_dev) {
  GTNX_HOST_T("batch.asg_lattice_score_grad");
  asg_lattice_impl("gtnx_batch_asg_lattice_score_grad", ems, frames, table_dev,
                   {arcs_dev, row_stride, num_arcs_dev, num_nodes_dev, arc_weights_dev, A, max_states}, max_edges, nullptr,
                   weights_dev, grad_em_dev, grad_table_dev, arc_grad_dev);
}

// ---- batched ASG token alignment of device-resident hypotheses (asg_token_align.hip) ----
namespace {
constexpr const char* kAsgTokenAlign = "gtnx_batch_asg_token_align";
Counters g_asg_token_align;  // (calls, pairs)
// the back-pointer words: a pair that is above the cap by itself runs alone with scratch of its own size
constexpr ScratchCap kAsgTokenAlignScratch{"GTNX_ASG_TOKEN_ALIGN_SCRATCH_BYTES", int64_t(256) << 20};
}  // namespace

void batch_asg_token_align_stats(int64_t* calls, int64_t* pairs) { g_asg_token_align.get(calls, pairs); }

void batch_asg_token_align(const BatchP& ems, const int* frames, const float* table_dev, const int* tokens_dev,
                           int64_t row_stride, const int* lengths_dev, int N, int L, int max_length, float* scores_dev,
                           int* starts_dev, int* ends_dev, float* token_scores_dev, int64_t out_stride,
                           int* frame_tokens_dev, int64_t frame_stride) {
  GTNX_HOST_T("batch.asg_token_align");
  const char* who = kAsgTokenAlign;
  const Hypotheses h{tokens_dev, row_stride, lengths_dev, N, L, max_length};
  // what the arguments alone decide comes first: no device is asked for an invalid call
  if (!table_dev) refuse(who, "null table pointer");
  if (!scores_dev || !starts_dev || !ends_dev) refuse(who, "null output pointer (scores, starts and ends are all written)");
  if (out_stride < 0 || frame_stride < 0) refuse(who, "negative row stride");
  if (out_stride < L) refuse(who, "out_stride is shorter than the rows' width L");
  const int64_t pairs = check_hypotheses(who, ems, h);
  if (pairs <= 0) return;
  Batch& x = linear_hypothesis_batch(who, ems, frames);
  if (frame_tokens_dev && frame_stride < x.M) refuse(who, "frame_stride is shorter than the rows of the batch");
  Runtime& rt = Runtime::get();
  // (the kernel gathers from it: host memory is refused too, with one GPU as well)
  if (!ptr_device_memory_of(table_dev, rt.device())) refuse(who, "the table is not memory of the engine's current device");
  check_outputs_local(who, {scores_dev, starts_dev, ends_dev, token_scores_dev, frame_tokens_dev});
  AsgTokenAlignArgs a{};
  const PairFrames fr = settle_frames(x, frames, h, a);
  const int U = max_length;
  a.table = table_dev;
  a.scores = scores_dev;
  a.starts = starts_dev;
  a.ends = ends_dev;
  a.token_scores = token_scores_dev;
  a.frame_tokens = frame_tokens_dev;
  a.out_stride = out_stride;
  a.frame_stride = frame_stride;
  // algorithmic bytes, by the widths (the lengths are device memory: an upper bound).  Per pair and frame one emission
  // per position and 1 bit per position out; the walk reads one window of 64 words per 32 frames; the tokens, two table
  // entries per position and the length once, the score and the two span rows out; with token scores one emission per
  // frame at most and the row; with frame tokens the row.
  const double per_pair_frames = fr.mean;
  const double pair_bytes = (4.0 + 0.125) * double(U) * per_pair_frames + 8.0 * per_pair_frames +
                            12.0 * std::min(L, U) + 8.0 + 8.0 * L +
                            (token_scores_dev ? 4.0 * per_pair_frames + 4.0 * L : 0.0) +
                            (frame_tokens_dev ? 4.0 * x.M : 0.0);
  const int64_t per_pair = (std::max<int64_t>(int64_t(fr.maxT), 1) + 31) / 32 * U;  // words
  a.pair_stride = per_pair;
  for_pair_slices(pairs, 4 * per_pair, kAsgTokenAlignScratch, [&](int64_t p0, int64_t cnt) {
    DevMemP words = rt.alloc(size_t(4 * per_pair * cnt));
    a.bp = words->as<unsigned>();
    a.pair0 = p0;
    a.count = int(cnt);
    GTNX_PROF("asg_token_align", pair_bytes * double(cnt));
    launch_asg_token_align(a, rt.stream());
    // (the words go back to the stream-ordered pool behind the launch)
  });
  g_asg_token_align.add(1, pairs);
}

}  // namespace gtnx
