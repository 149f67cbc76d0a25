// batch.h -- B graphs held as ONE record.
//
// The reference runs a criterion as parallelMap over per-utterance graphs
// (benchmarks/ctc.cpp:136-168, bindings/python/examples/pytorch_loss.py:46-102); the vector
// overloads of ops.h already turn that into one launch per function, but they still hand back B
// graph objects per call (structure + weights + autograd node each), and at C3 the host spent
// four times the GPU's time creating and destroying them.  A Batch is what such a call returns
// when nobody looks at the elements: one object, one tape node, dense device arrays.  Taking an
// element out (batch_get) builds the ordinary per-graph expression once, tape included, so
// anything the batch functions do not cover natively still works -- through the vector ops.
//
// Native (no per-element objects):   CTC target acceptors built on the device from label
// sequences, linear chains over one [B][M][C] tensor, their composition (kept symbolic),
// forwardScore of both, negate / add / subtract, backward, item / gradient gathers.
#pragma once

#include <memory>
#include <vector>

#include "ops.h"

namespace gtnx {

struct Batch;
using BatchP = std::shared_ptr<Batch>;

struct BatchOp {
  uint64_t seq = 0;
  std::vector<BatchP> inputs;
  virtual void backward(Batch& out) = 0;
  virtual ~BatchOp() {}
};

struct Batch {
  enum Kind { GRAPHS, CTC_TARGETS, LINEAR, PRODUCT, SCALAR };
  Kind kind = GRAPHS;
  int n = 0;
  bool calc_grad = false;

  // the elements as graphs: always there for GRAPHS, built on demand otherwise (then THEY carry the
  // gradients: batch-level results are pushed into them)
  bool materialised = false;
  std::vector<Graph> graphs;
  // CTC_TARGETS / LINEAR made FROM the caller's graphs (region.cpp: the leaves of a parallelMap region): `graphs`
  // are those graphs from the start, the native arrays describe the same values, and every gradient the batch
  // functions produce is pushed into the graphs (that is where the caller looks)
  bool leaf = false;
  // ... taken from the digests of a region's slices (region.cpp): when the record dies, the graphs of each range
  // go back to the thread that built them (give_back(home, graphs)) instead of being taken apart here
  struct Origin {
    std::shared_ptr<void> home;
    size_t begin, end;
  };
  std::vector<Origin> origins;
  void (*give_back)(const std::shared_ptr<void>& home, std::vector<Graph>* part) = nullptr;
  // SCALAR: the values on the host, fetched once when an element's item() is asked for (batch_item_host)
  std::vector<float> host_vals;
  bool host_vals_valid = false;
  // ... or on their way: copied to pinned memory BEHIND the launch that produced them (batch_prefetch_items), so
  // that reading a loss waits for the forward sweep only, not for whatever was queued after it (the backward
  // sweep of the same step: the host prepares the next step meanwhile)
  PinnedMemP host_pin;
  void* host_ev = nullptr;  // hipEvent_t

  // ---- CTC_TARGETS: label sequences back to back; records (BandNode, flags, sorted lists) on the device
  std::vector<int> labels, lab_off;  // lab_off[n + 1]
  int blank = 0;
  int max_label = -1, max_nodes = 0;
  DevMemP rec_mem;
  std::vector<size_t> rec_off;       // byte offset of element b's records
  // ... or force-alignment acceptors composed with an ASG transitions graph (examples/asg.cpp:50-68):
  // U + 1 nodes and 2U weighted arcs per sequence, weights gathered from the transitions on the device
  bool fal = false;
  Graph trans;                       // the transitions graph (its gradient is scattered back into it)
  int trans_labels = 0;
  std::vector<size_t> w_off, map_off;  // byte offsets of element b's arc weights / arc -> transitions arc map
  // ---- LINEAR: [n][M][C] device tensor (owned copy or the caller's)
  int M = 0, C = 0;
  DevMemP w_mem;
  float* w_dev = nullptr;
  std::shared_ptr<PendingCopy> w_pend;  // LINEAR over a region's staged weights: the values may not be at w_dev yet
                                        // (graph.h PendingCopy; batch.cpp linear_values settles, the band forward fuses)
  DevMemP nc_mem;                    // forwardScore of every chain + per-row log-sum-exps, left behind by a sweep
  float* nc_norm = nullptr;
  float* nc_rowlse = nullptr;
  // ... ragged: element b is linearGraph(rows[b], C) over the first rows[b] rows of its [M][C] slab (1 <= rows[b] <= M;
  // the slab stride, the gradient layout and every arena stay on M).  Empty: every element has M rows.  The gradient's
  // rows [rows[b], M) are zero: the sweeps write rows < rows[b] and ONE launch of padfill.hip stores the rest
  // (pad_floats of them; its table -- rows [n] and the prefix sums of the pads [n + 1] -- is uploaded on first use)
  std::vector<int> rows;
  int64_t pad_floats = 0;
  DevMemP pad_mem;
  int rows_of(int b) const { return rows.empty() ? M : rows[size_t(b)]; }
  // ---- PRODUCT: compose(fixed, chain) / compose(chain, fixed), never built
  BatchP fixed, chain;
  bool chain_first = false, intersect = false;
  bool wide = false;  // force-alignment acceptors x an alphabet of 1025 .. 2048 labels: past the band sweeps, kept for
                      // batch_viterbi_align's launch (asg_align.hip) -- everything else composes the element graphs
  bool full = false;  // `fixed` is a GRAPHS batch of ONE asgTransitions(C) graph, C <= asg_full_max_labels(), and `chain`
                      // carries row counts (or GTNX_FULL_CONNECT=1): kept for forwardScore's launch (asg_full.hip) --
                      // everything else composes the element graphs
  // ---- SCALAR: one float per element
  DevMemP v_mem;
  float* v_dev = nullptr;

  // ---- autograd
  std::shared_ptr<BatchOp> op;
  bool tape_cleared = false;         // backward without retain went through here (autograd.cpp:48-51)
  DevMemP g_mem;                     // gradient, elements back to back at g_off[b] (floats)
  float* g_dev = nullptr;
  std::vector<int64_t> g_off;        // n + 1
  DevMemP dest_mem;                  // batch_grads_bind: where the first gradient should be written
  float* dest = nullptr;

  int64_t elem_size(int b) const;    // gradient floats of element b (arcs; an upper bound for CTC_TARGETS)
  ~Batch();                          // the element graphs go to the runtime's deferred list in chunks
};

BatchP batch_from_graphs(std::vector<Graph> gs);
BatchP batch_ctc_targets(const int* labels, const int* lengths, int n, int blank, bool calc_grad);
// One CTC criterion step in ONE launch (ctc_step.hip): loss_b = forwardScore(emissions_b) - forwardScore(target_b o
// emissions_b) into loss[b], d loss / d emissions into grad, and -- target_grad -- the targets' arc gradients into
// target_grad_dev (utterance b's at the running sum of the arc counts in front of it; null: computed and dropped).
// What the graph-level operations compute for the same batch, bit for bit.  ctc_step_fused_ok: is the batch one the
// launch is instantiated for?  A pure host function (no device is asked); batch_ctc_loss_step throws
// GTNX_INVALID_ARGUMENT for a batch it is not.
bool ctc_step_fused_ok(const int* labels, const int* lengths, int n, int T, int C, int blank, const void* emissions,
                       const void* grad);
void batch_ctc_loss_step(const void* emissions, const int* labels, const int* lengths, int n, int T, int C, int blank,
                         void* loss, void* grad, bool target_grad, void* target_grad_dev);
BatchP batch_asg_force_align(const int* labels, const int* lengths, int n, Graph& transitions, int n_labels);
// rows (host, [n], or null): the rows of each element that count (Batch::rows); outside 1 .. M: invalid argument
BatchP batch_linear(int n, int M, int C, bool calc_grad, const void* dev, bool borrow, const int* rows = nullptr);
BatchP batch_compose(const BatchP& a, const BatchP& b, bool intersect);
BatchP batch_shortest_distance(const BatchP& x, bool tropical);
// utterances whose full-connect score forwardScore(chain_b o asgTransitions) came from the one launch of asg_full.hip /
// utterances of a padded batch against such a graph that took the composed elements instead (an alphabet above
// asg_full_max_labels(), or a consumer other than forwardScore)
void batch_full_connect_stats(int64_t* fast, int64_t* fallback);
BatchP batch_viterbi_path(const BatchP& x);
// Forced alignment with device-resident output: labels_dev[b * row_stride + t] = the label of frame t on utterance b's
// best path (-1 from the path's end on, everywhere when there is no path), tokens_dev likewise the index into the label
// sequence (-1 on blank frames), scores_dev[b] the path's score.  A PRODUCT of device-built CTC targets (blank below
// every label) with a LINEAR batch is aligned by one launch on the engine's stream (align.hip): no graphs, no copy
// back, no synchronisation; frames (host, [n], or null): rows of each utterance to align (null: the chain's own row
// counts; more than those: invalid argument).  A PRODUCT of device-built force-alignment acceptors o ASG transitions
// (batch_asg_force_align) with a LINEAR batch over the same alphabet likewise, either argument order (asg_align.hip;
// tokens = index into the label sequence, never -1 inside a path; exact ties: the step wins).  Every other batch goes
// through batch_viterbi_path and one upload; tokens_dev and frames are invalid arguments there.
void batch_viterbi_align(const BatchP& x, const int* frames, int* labels_dev, int64_t row_stride, int* tokens_dev,
                         float* scores_dev);
void batch_align_stats(int64_t* fast, int64_t* fallback);  // utterances aligned by the launch / by the path graphs
// viterbiPath(ems_b o transitions) of a whole batch against ONE shared graph, results on the device: labels_dev[b *
// row_stride + t] = the label of frame t of utterance b's best path for t < T_b, -1 from T_b to the row's width M (and
// everywhere without an accepting path: score -inf, length 0); scores_dev[b] (or null) the path score; collapsed_dev[b *
// row_stride + ..] (or null) the labels with runs of equal consecutive frames merged, -1 up to M; lengths_dev[b] (or
// null; needs collapsed_dev) how many.  frames (host, [n], or null): T_b, null = rows_of(b); outside 0 .. M or above
// rows_of(b): invalid argument, before anything is launched.  A native LINEAR batch against a graph in the dense regime
// whose ties go by node order (lazy_decode_ok: asgTransitions-shaped, 8 .. 1024 nodes) with outputs local to the
// device: full-length views of the slabs form ONE max-plus group (the sweep reads the pad rows; what they hold never
// changes a bit of any output), asg_decode.hip is launched once, no download, no path graphs, no wait.  Ties: first
// accept node in accept-list order, then the smallest source node.  Everything else: op_viterbi_path over the composed
// elements, labels read and collapsed on the host, one upload; frames must be null there.
void batch_viterbi_decode(const BatchP& ems, Graph& transitions, const int* frames, int* labels_dev, int64_t row_stride,
                          float* scores_dev, int* collapsed_dev, int* lengths_dev);
void batch_decode_stats(int64_t* fast, int64_t* fallback);  // utterances decoded by the launch / by the path graphs
// viterbiPath(ems_b) of a whole batch of chains plus the CTC collapse, results on the device (the decode a CTC model
// runs at inference).  labels_dev[b * row_stride + t] = the first label holding the maximum of frame t for t < T_b
// (shortest.cpp:190-272: `>` from -inf, so the smallest label among equal maxima; NaN and -inf are never taken), -1
// from T_b to the row's width M; scores_dev[b] (or null) = ((0 + m_0) + m_1) + ... in float32 in frame order;
// collapsed_dev[b * row_stride + k] (or null) the labels with repeats merged and `blank` dropped (blank < 0: nothing is
// dropped), starts_dev (or null; needs collapsed_dev) the first frame of each, both -1 from the length to M;
// lengths_dev[b] (or null; needs collapsed_dev) how many.  A frame without an entry above -inf: no path -- every entry
// of every row -1, score -inf, length 0; T_b = 0 likewise (creations.cpp:22: the start node does not accept).  frames (host, [n], or null): T_b,
// null = rows_of(b); outside 0 .. M or above rows_of(b), row_stride < M, blank >= C: invalid argument, before a device
// is asked for.  A native LINEAR batch: two launches of linear_decode.hip on the engine's stream, rows from T_b on are
// never read, no download, no path graphs, no wait.  Everything else: batch_viterbi_path, labels read and collapsed
// on the host by the same rules, one upload; frames must be null there.
void batch_linear_decode(const BatchP& ems, const int* frames, int blank, int* labels_dev, int64_t row_stride,
                         float* scores_dev, int* collapsed_dev, int* starts_dev, int* lengths_dev);
void batch_linear_decode_stats(int64_t* fast, int64_t* fallback);  // utterances decoded by the launches / the path graphs
// N alignments of every chain of a native LINEAR batch drawn from its frame posteriors, plus the CTC collapse, results
// on the device (DESIGN section 32 holds the contract: frame t < T_b of sample k takes label c with probability
// exp(x[b,t,c] / temperature) / Z[b,t] over the finite entries, by inverse CDF in label order against the uniform of
// Philox4x32-10 at key `seed`, counter (t, b, k >> 2, 0), word k & 3).  tokens_dev[(b * N + k) * row_stride + i]: the
// alignment with repeats merged and `blank` dropped (blank < 0: nothing dropped), -1 from its length to the row's width
// M; lengths_dev[b * N + k]; logq_dev[b * N + k] (or null) = sum_t (x[b,t,c_t] / temperature - log Z[b,t]) in float32
// in frame order; labels_dev (or null) the frame labels in the layout of tokens_dev, -1 from T_b to M.  A frame without
// a finite entry, or T_b = 0: no path -- every sample of the utterance gets -1 rows, length 0, logq -inf.  frames (host,
// [n], or null): T_b, null = rows_of(b).  Invalid argument before a device is asked for: a null batch, tokens or
// lengths pointer, a negative stride, N outside 1 .. 1024, a temperature that is not finite and > 0.  With the device:
// a batch that is not a native LINEAR one (there is no other route), a count outside 0 .. M or above rows_of(b),
// row_stride < M, blank >= C, n * N beyond an int, outputs that are not memory of the current device.  Two launches of
// ctc_sample.hip on the engine's stream per slice; 4 (with labels_dev) or 8 bytes per (b, k, t) of scratch from the
// stream-ordered pool, at most 256 MiB per launch: beyond that the utterances run in slices with the same bytes (the
// environment variable GTNX_CTC_SAMPLE_SCRATCH_BYTES, read per call, lowers the cap: a debug switch for tests).  Rows
// from T_b on are never read, no download, no wait.
void batch_ctc_sample(const BatchP& ems, const int* frames, int blank, int N, uint64_t seed, float temperature,
                      int* tokens_dev, int64_t row_stride, int* lengths_dev, float* logq_dev, int* labels_dev);
void batch_ctc_sample_stats(int64_t* calls, int64_t* utterances);  // calls that launched / utterances they sampled
// CTC prefix beam search with N-best output over a native LINEAR batch, results on the device (DESIGN section 20 holds
// the contract: token set of a frame = its topn best labels plus blank, at most `beam` distinct prefixes with (pb, pnb),
// exact prefix merging, the total order of the candidates).  tokens_dev[(b * nbest + r) * row_stride + k]: the labels of
// hypothesis r of utterance b, -1 from its length to the row's width M; lengths_dev[b * nbest + r]; scores_dev[b * nbest
// + r] = logadd(pb, pnb); slots without a hypothesis (fewer than nbest prefixes, a frame with an empty token set,
// T_b = 0): -1, 0, -inf.  frames (host, [n], or null): T_b, null = rows_of(b).  Invalid argument before a device is
// asked for: null outputs, a negative stride, beam outside 1 .. 64, topn outside 1 .. 32, nbest outside 1 .. beam, a
// negative blank.  With the device: a batch that is not a native LINEAR one (there is no other route), a count outside
// 0 .. M or above rows_of(b), row_stride < M, blank >= C, outputs that are not memory of the current device.  Two
// launches of ctc_beam.hip on the engine's stream, scratch from the stream-ordered pool; rows from T_b on are never
// read, no download, no wait.
void batch_ctc_beam_decode(const BatchP& ems, const int* frames, int blank, int beam, int topn, int nbest,
                           int* tokens_dev, int64_t row_stride, int* lengths_dev, float* scores_dev);
// The same search with a bigram over the labels fused in (DESIGN section 23 holds the contract).  table_dev: device
// float32 [C + C * C] in the arc order of criteria::asgTransitions -- table[c] scores c as first label, table[C + i * C
// + j] label j followed by label i.  A prefix carries L = the sum over its labels of weight * table(...) + bonus,
// float32, left to right; candidates rank by acoustic total + L, an extension whose term is not finite is dropped (-inf
// in the table forbids it), row pruning and (pb, pnb) stay acoustic.  scores_dev gets acoustic + L, am_scores_dev (may
// be null) the acoustic total, -inf in both for a slot without a hypothesis.  lm = null is the call above.  On top of
// its refusals, before a device is asked for: a null table, a weight or bonus that is not finite; with the device: more
// than 2^19 labels, a table that is not memory allocated on the current device (pageable, pinned or registered host
// memory and managed memory are all refused: the kernel gathers from it), an am_scores_dev the device may not write.
// Counted by batch_ctc_beam_stats like the call above.
// With a compiled LM graph in the table's place (lm_graph.h): `graph` is a handle of
// lm_graph_register and table_dev is null.  A prefix then also carries its LM state, an extension's table entry is the
// weight of the walk of (state, label) -- failure-arc semantics -- and a label the walk does not find, or whose weight
// is not finite, is forbidden.  Everything else is as with the table, C <= 2^19 included.  Refused on top, before a
// device is asked for: a table and a graph together, a handle that is not a live one.  The first decode with a graph
// uploads it and waits for the copy, once.
struct CtcBeamLm {
  const float* table_dev;
  float weight, bonus;
  float* am_scores_dev;
  const void* graph = nullptr;
};
void batch_ctc_beam_decode(const BatchP& ems, const int* frames, int blank, int beam, int topn, int nbest,
                           const CtcBeamLm* lm, int* tokens_dev, int64_t row_stride, int* lengths_dev, float* scores_dev);
void batch_ctc_beam_stats(int64_t* calls, int64_t* utterances);  // calls that launched / utterances they decoded
// ASG prefix beam search with N-best output over a native LINEAR batch, results on the device (DESIGN section 27 holds
// the contract: the hypotheses are the label sequences without equal neighbours, each summed over its alignments under
// emissions o transitions; token set of a frame = its topn best labels, no blank, restricting stays as well as
// extensions; at most `beam` distinct prefixes with one score each; exact prefix merging; the total order of the
// candidates).  table_dev: device float32 [C + C * C] in the arc order of criteria::asgTransitions -- table[c] =
// start[c], table[C + i * C + j] = label j followed by label i; an entry that is not finite drops its candidates (-inf
// forbids a bigram or a first label).  tokens_dev[(b * nbest + r) * row_stride + k]: the labels of hypothesis r of
// utterance b, -1 from its length to the row's width M; lengths_dev[b * nbest + r]; scores_dev[b * nbest + r]; slots
// without a hypothesis (fewer than nbest prefixes, a frame with an empty token set, T_b = 0): -1, 0, -inf.  frames
// (host, [n], or null): T_b, null = rows_of(b).  Invalid argument before a device is asked for: a null batch, table or
// output, a negative stride, beam outside 1 .. 64, topn outside 1 .. 32, nbest outside 1 .. beam; n == 0 returns
// without a device.  With the device: a batch that is not a native LINEAR one (there is no other route), a count
// outside 0 .. M or above rows_of(b), row_stride < M, M * beam beyond an int, more than 2^19 labels, a table that is
// not memory allocated on the current device, outputs that are not memory of the current device.  Two launches of
// asg_beam.hip on the engine's stream, scratch from the stream-ordered pool; rows from T_b on are never read, no
// download, no wait.
void batch_asg_beam_decode(const BatchP& ems, const int* frames, const float* table_dev, int beam, int topn, int nbest,
                           int* tokens_dev, int64_t row_stride, int* lengths_dev, float* scores_dev);
// The same search with a compiled LM graph fused into the ranking (lm_graph.h): `graph` is a handle
// of lm_graph_register.  Every prefix also carries L and its LM state -- the empty prefix 0 and the start state; an
// extension by c walks (state, c) with failure-arc semantics and adds weight * walk + bonus (the product rounded, then
// the sum) to L; a stay copies both -- and candidates rank by acoustic score + L.  A label the walk forbids, or whose
// term is not finite, drops the extension; the stays, the merging and the rows stay acoustic; table_dev is still the
// criterion's own table.  scores_dev gets acoustic + L and am_scores_dev (may be null) the acoustic score alone, -inf
// in slots without a hypothesis.  Refused on top, under the name gtnx_batch_asg_beam_decode_graph like every refusal
// of this call: before a device is asked for a handle that is not a live one and a weight or bonus that is not finite;
// with the device an am_scores_dev that is not memory allocated on the current device (host memory included, with one
// GPU as well) and a graph that lives on another device.  The first decode with a graph uploads it and waits for the
// copy, once.  Counted by batch_asg_beam_stats like the call above.
struct AsgBeamLm {
  const void* graph;
  float weight, bonus;
  float* am_scores_dev;
};
void batch_asg_beam_decode(const BatchP& ems, const int* frames, const float* table_dev, int beam, int topn, int nbest,
                           const AsgBeamLm* lm, int* tokens_dev, int64_t row_stride, int* lengths_dev,
                           float* scores_dev);
void batch_asg_beam_stats(int64_t* calls, int64_t* utterances);  // calls that launched / utterances they decoded
// N alignments of every chain of a native LINEAR batch drawn from the posterior of emissions o transitions, plus the
// merge of equal neighbours, results on the device (DESIGN section 34 holds the contract: forward filtering in a
// per-frame rescaled form, then backward sampling -- frame T_b - 1 from exp(alpha), frame t below it from exp(alpha_t[j]
// + table[C + y_{t+1} * C + j] / temperature), by inverse CDF in label order against the uniform of Philox4x32-10 at
// key `seed`, counter (t, b, k >> 2, 1), word k & 3).  table_dev: [C + C * C], the table of batch_asg_score.
// tokens_dev[(b * N + k) * row_stride + i]: the alignment with equal neighbours merged, -1 from its length to the
// row's width M; lengths_dev[b * N + k]; logq_dev[b * N + k] (or null): the sum of the drawn conditionals' logs in
// draw order in float32 (= s(y) / temperature - logZ_b); labels_dev (or null): the frame labels in the layout of
// tokens_dev, -1 from T_b to M; logz_dev[b] (or null): logZ_b.  An utterance without an alignment of finite score, or
// T_b = 0: no path -- every sample of it gets -1 rows, length 0, logq -inf, and logz -inf.  frames (host, [n], or
// null): T_b, null = rows_of(b).  Invalid argument before a device is asked for: a null batch, table, tokens or
// lengths pointer, a negative stride, N outside 1 .. 1024, a temperature that is not finite and > 0, C outside 1 ..
// 1024 (the filter is O(T C^2) per utterance and the draw keeps a row in the registers of one wave).  With the device:
// a batch that is not a native LINEAR one (there is no other route), a count outside 0 .. M or above rows_of(b),
// row_stride < M, n * N beyond an int, a table or outputs that are not memory of the current device.  Per slice three
// launches of asg_sample.hip on the engine's stream (filter, draw, collapse), before them one prep launch per call
// above 128 labels; 4 M C bytes of planes per utterance plus 4 (with labels_dev) or 8 bytes per (b, k, t) of scratch
// from the stream-ordered pool, at most 256 MiB per slice: beyond that the utterances run in slices with the same
// bytes (the environment variable GTNX_ASG_SAMPLE_SCRATCH_BYTES, read per call, lowers the cap: a debug switch for
// tests).  Rows from T_b on are never read, no download, no wait.
void batch_asg_sample(const BatchP& ems, const int* frames, const float* table_dev, int N, uint64_t seed,
                      float temperature, int* tokens_dev, int64_t row_stride, int* lengths_dev, float* logq_dev,
                      int* labels_dev, float* logz_dev);
void batch_asg_sample_stats(int64_t* calls, int64_t* utterances);  // calls that launched / utterances they sampled
// Levenshtein distance (unit costs) of all B * N pairs (hyp[b, k], ref[b]) of device-resident token rows, results on the
// device (DESIGN section 21 holds the contract).  hyp_dev: int32 [B][N] rows of width L, hyp_stride elements apart;
// hyp_len_dev: int32 [B][N]; ref_dev: int32 [B] rows of width U, ref_stride apart; ref_len_dev: int32 [B] -- lengths
// are DEVICE memory, clamped to 0 .. L / 0 .. U by the kernel, and nothing at or past a clamped length is read.  Tokens
// are compared with == only.  dist_dev[b * N + k]; ops_dev (or null) [b * N + k][3] = (substitutions, deletions,
// insertions) of the walk back from (len_ref, len_hyp) that takes the first move attaining D[i][j] of diagonal, up
// (deletion), left (insertion).  Invalid argument before a device is asked for: a null input or dist pointer, negative
// B, N, L, U or stride, a stride below its width, L > 65536, U > 4096, B * N beyond an int; B * N == 0 returns without
// a device.  With the device: an output that is not memory of the current device.  Without ops one launch; with ops
// the walk's scratch (16 bytes * L * ceil(U / 64) per pair, from the stream-ordered pool) is capped at 256 MiB per
// launch (GTNX_EDIT_DISTANCE_SCRATCH_BYTES lowers the cap: a debug switch) and the pairs run in slices of launches.
// No download, no wait.
void batch_edit_distance(const int* hyp_dev, int64_t hyp_stride, const int* hyp_len_dev, const int* ref_dev,
                         int64_t ref_stride, const int* ref_len_dev, int B, int N, int L, int U, int* dist_dev,
                         int* ops_dev);
void batch_edit_distance_stats(int64_t* calls, int64_t* pairs);  // calls that launched / pairs they computed
// The exact log score of all n * N device-resident hypotheses under the n emission slabs of a native linear batch,
// score[b * N + k] = forwardScore(ctcGraph(tokens[b, k, :len], blank) o emissions_b[:T_b]) with len = clamp(lengths[b, k],
// 0, L), nothing subtracted, results on the device (DESIGN section 22 holds the contract).  tokens_dev: int32 n * N rows
// of width L, row_stride elements apart; lengths_dev: int32 [n][N], DEVICE memory; frames: HOST, T_b per element or null.
// -inf (never NaN): no alignment fits, len > max_length, a token inside the length outside 0 .. C - 1, T_b == 0.
// Invalid argument before a device is asked for: a null pointer, negative N, L, stride or blank, row_stride < L,
// max_length outside 1 .. 4096; n * N == 0 returns without a device.  With the device: not a native linear batch, a
// frame count outside 0 .. M, blank >= C, an output that is not memory of the current device.  One launch, no scratch.
void batch_ctc_score(const BatchP& ems, const int* frames, int blank, const int* tokens_dev, int64_t row_stride,
                     const int* lengths_dev, int N, int L, int max_length, float* scores_dev);
// grad_dev[b][t][c] = sum over k of weights_dev[b * N + k] * d score[b, k] / d emissions[b][t][c], every element of
// [n][M][C] written (zeros where nothing lands, pad rows included); a pair whose score is -inf or whose weight is
// exactly 0 adds nothing.  The alpha rows are recomputed into scratch from the stream-ordered pool (max T_b * (2 *
// max_length + 1) floats per pair), at most 256 MiB per launch pair (GTNX_CTC_SCORE_SCRATCH_BYTES lowers the cap: a
// debug switch); beyond it the pairs run in slices with the same bits.  No floating-point atomics: bit-repeatable.
void batch_ctc_score_grad(const BatchP& ems, const int* frames, int blank, const int* tokens_dev, int64_t row_stride,
                          const int* lengths_dev, int N, int L, int max_length, const float* weights_dev,
                          float* grad_dev);
void batch_ctc_score_stats(int64_t* calls, int64_t* pairs);  // calls that launched (either kind) / pairs they took
// The exact CTC log score of one device-resident acyclic token lattice per utterance under the n emission slabs of a
// native linear batch, results on the device (DESIGN section 35 holds the contract): scores_dev[b] = log sum over the
// lattice's paths p of exp(w(p) + ctc_score(emissions_b[:T_b], labels(p))), nothing subtracted.  arcs_dev: int32 n rows
// of A arcs (src, dst, label), row_stride (>= 3 A) elements apart, dst-sorted within a row; num_arcs_dev / num_nodes_dev:
// int32 [n], DEVICE memory (node 0 starts, node num_nodes - 1 accepts); arc_weights_dev: float32 [n][A] or null (zeros);
// max_states (1 .. 4096) bounds nodes + arcs and sizes LDS and scratch; frames: HOST, T_b per element or null.
// -inf (never NaN): T_b == 0, num_nodes < 1, nodes + arcs > max_states, an arc with src < 0, src >= dst or dst >=
// num_nodes, an arc out of dst order, a label outside 0 .. C - 1, a weight that is +inf or NaN, no alignment.  Invalid
// argument before a device is asked for: a null pointer, negative A or blank, row_stride < 3 A, max_states outside
// 1 .. 4096; n == 0 returns without a device.  With the device: not a native linear batch, a frame count outside 0 .. M,
// blank >= C, an output that is not memory of the current device.  One launch, no scratch, no download, no wait.
void batch_ctc_lattice_score(const BatchP& ems, const int* frames, int blank, const int* arcs_dev, int64_t row_stride,
                             const int* num_arcs_dev, const int* num_nodes_dev, const float* arc_weights_dev, int A,
                             int max_states, float* scores_dev);
// grad_dev[b][t][c] = weights_dev[b] * d score[b] / d emissions[b][t][c], every element of [n][M][C] written (zeros where
// nothing lands, pad rows included); arc_grad_dev (or null) [n][A] = weights_dev[b] * d score[b] / d arc weight, the
// posterior of the arc, zeros at or past num_arcs[b]; an utterance whose score is -inf or whose weight is exactly 0 gets
// zeros.  The alpha rows are recomputed into scratch from the stream-ordered pool (max T_b * max_states floats per
// utterance), at most 256 MiB per launch pair (GTNX_CTC_LATTICE_SCRATCH_BYTES lowers the cap: a debug switch); beyond it
// the utterances run in slices with the same bits.  No floating-point atomics: bit-repeatable.
void batch_ctc_lattice_score_grad(const BatchP& ems, const int* frames, int blank, const int* arcs_dev,
                                  int64_t row_stride, const int* num_arcs_dev, const int* num_nodes_dev,
                                  const float* arc_weights_dev, int A, int max_states, const float* weights_dev,
                                  float* grad_dev, float* arc_grad_dev);
void batch_ctc_lattice_score_stats(int64_t* calls, int64_t* utterances);  // calls that launched / utterances they took
// The best (lattice path, alignment) pair of one device-resident acyclic token lattice per utterance (the lattice
// arguments, blank, frames and max_states of batch_ctc_lattice_score, with the same meaning), results on the device
// (DESIGN section 38 holds the contract): scores_dev [n] the best w(p) + alignment score, path_len_dev [n] the arcs on the
// best path, path_arcs_dev / path_tokens_dev / starts_dev / ends_dev (n rows of width P, out_stride apart) the arc
// indices in path order, their labels, the first frame of each and one past its last (the first P of a longer path),
// token_scores_dev (same layout, or null) the arc's emissions summed in frame order, frame_arcs_dev (n rows of width M,
// frame_stride apart, or null) the arc of every frame, -1 on blank frames.  Float32 max-plus; of equal candidates the
// first in the forward recurrence's order wins: bit-reproducible.  -1 / -inf wherever no path covers an entry (path_len
// 0, score -inf); an utterance has no path where batch_ctc_lattice_score gives -inf.  Every element of every row is
// written over its width, nothing beyond.
// Invalid argument before a device is asked for: what batch_ctc_lattice_score refuses there, a null scores, path_len,
// path_arcs, path_tokens, starts or ends pointer, P < 1, out_stride < P; n == 0 returns without a device.  With the
// device: not a native linear batch, a frame count outside 0 .. M, blank >= C, frame_stride < M with frame arcs, an
// output that is not memory of the current device.  The back-pointers (16 bits per state and frame, max T_b * max_states
// of them per utterance) come from the stream-ordered pool, at most 256 MiB per launch
// (GTNX_CTC_LATTICE_ALIGN_SCRATCH_BYTES lowers the cap: a debug switch); beyond it the utterances run in slices, same
// bits.
void batch_ctc_lattice_align(const BatchP& ems, const int* frames, int blank, const int* arcs_dev, int64_t row_stride,
                             const int* num_arcs_dev, const int* num_nodes_dev, const float* arc_weights_dev, int A,
                             int max_states, float* scores_dev, int* path_len_dev, int* path_arcs_dev,
                             int* path_tokens_dev, int* starts_dev, int* ends_dev, float* token_scores_dev, int P,
                             int64_t out_stride, int* frame_arcs_dev, int64_t frame_stride);
void batch_ctc_lattice_align_stats(int64_t* calls, int64_t* utterances);  // calls that launched / utterances they took
// The best alignment of all n * N device-resident hypotheses (the pair form of batch_ctc_score) under the n emission
// slabs of a native linear batch, results on the device (DESIGN section 24 holds the contract): scores_dev [n][N] the
// Viterbi score, starts_dev / ends_dev (n * N rows of width L, out_stride apart) the first frame of token i and one past
// its last, token_scores_dev (same layout, or null) the token's emissions summed in frame order, frame_tokens_dev (n * N
// rows of width M, frame_stride apart, or null) the token index of every frame, -1 on blank frames.  Float32 max-plus
// with the tie rule of align.hip: bit-reproducible.  -1 / -inf wherever no path covers an entry; a pair has no path
// where batch_ctc_score gives -inf.  Every element of every row is written over its width, nothing beyond.
// Invalid argument before a device is asked for: a null batch, input, scores, starts or ends pointer, negative N, L,
// stride or blank, row_stride < L, out_stride < L, max_length outside 1 .. 4096; n * N == 0 returns without a device.
// With the device: not a native linear batch, a frame count outside 0 .. M, blank >= C, frame_stride < M with frame
// tokens, an output that is not memory of the current device.  The back-pointers (2 bits per state and frame, ceil(max
// T_b / 16) * (2 max_length + 1) words per pair) come from the stream-ordered pool, at most 256 MiB per launch
// (GTNX_CTC_TOKEN_ALIGN_SCRATCH_BYTES lowers the cap: a debug switch); beyond it the pairs run in slices, same bits.
void batch_ctc_token_align(const BatchP& ems, const int* frames, int blank, const int* tokens_dev, int64_t row_stride,
                           const int* lengths_dev, int N, int L, int max_length, float* scores_dev, int* starts_dev,
                           int* ends_dev, float* token_scores_dev, int64_t out_stride, int* frame_tokens_dev,
                           int64_t frame_stride);
void batch_ctc_token_align_stats(int64_t* calls, int64_t* pairs);  // calls that launched / pairs they aligned
// The ASG force-align term of all n * N device-resident hypotheses under the n emission slabs of a native linear batch,
// score[b * N + k] = forwardScore(emissions_b[:T_b] o (forceAlign(tokens[b, k, :len]) o transitions)) with len =
// clamp(lengths[b, k], 0, L), log semiring, nothing subtracted, results on the device (DESIGN section 25 holds the
// contract).  tokens_dev / lengths_dev / frames: as in batch_ctc_score (labels only: there is no blank, equal
// neighbours are legal).  table_dev: float32 [C + C * C], DEVICE memory of the current device (the kernel gathers from
// it), in the arc order of asgTransitions: entry y = start[y], entry C + i * C + j = transitions[i, j], label j
// followed by i.  -inf (never NaN): len == 0, T_b < len, len > max_length, a token inside the length outside
// 0 .. C - 1, every alignment crosses a -inf emission or table entry.
// Invalid argument before a device is asked for: a null pointer, negative N, L or stride, row_stride < L, max_length
// outside 1 .. 4096; n * N == 0 returns without a device.  With the device: not a native linear batch, a frame count
// outside 0 .. M, C > 16384, a table that is not device memory of the current device, an output that is not memory of
// the current device.  One launch, no scratch.
void batch_asg_score(const BatchP& ems, const int* frames, const float* table_dev, const int* tokens_dev,
                     int64_t row_stride, const int* lengths_dev, int N, int L, int max_length, float* scores_dev);
// grad_em_dev (or null) [b][t][c] = sum over k of weights_dev[b * N + k] * d score[b, k] / d emissions[b][t][c], every
// element of [n][M][C] written (zeros where nothing lands, pad rows included); grad_table_dev (or null) [C + C * C] =
// sum over all pairs of weights * d score / d table, every entry written; not both null.  A pair whose score is -inf
// or whose weight is exactly 0 adds nothing.  The alpha rows are recomputed into scratch from the stream-ordered pool
// (max T_b * max_length floats per pair), at most 256 MiB per slice (GTNX_ASG_SCORE_SCRATCH_BYTES lowers the cap:
// a debug switch); beyond it the pairs run in slices with the same bits.  With a table gradient the per-position
// occupancy sums (2 * min(L, max_length) floats per pair) stay in scratch until one reduction launch behind the last
// slice.  No floating-point atomics: bit-repeatable.
void batch_asg_score_grad(const BatchP& ems, const int* frames, const float* table_dev, const int* tokens_dev,
                          int64_t row_stride, const int* lengths_dev, int N, int L, int max_length,
                          const float* weights_dev, float* grad_em_dev, float* grad_table_dev);
void batch_asg_score_stats(int64_t* calls, int64_t* pairs);  // calls that launched (either kind) / pairs they took
// The exact ASG log score of one device-resident acyclic token lattice per utterance (batch_ctc_lattice_score's form)
// under the n emission slabs of a native linear batch and the [C + C * C] table of batch_asg_score, results on the device
// (DESIGN section 37 holds the contract): scores_dev[b] = log sum over the lattice's paths p of exp(w(p) +
// asg_score(emissions_b[:T_b], table, labels(p))), nothing subtracted.  The states are the arcs: there is no blank and
// equal neighbouring labels are legal.  max_states (1 .. 4096) bounds nodes + arcs, as for the CTC call; max_edges
// (1 .. 2^21) bounds E_b = the sum over the arcs of the in-degree of their src -- the kernel counts E_b and an utterance
// above the bound scores -inf.  -inf (never NaN): T_b == 0, num_nodes < 1, nodes + arcs > max_states, E_b > max_edges,
// every arc field batch_ctc_lattice_score refuses, a weight that is +inf or NaN, no alignment (a one-node lattice has
// none), every alignment through a -inf emission or table entry.  Invalid argument before a device is asked for: a null
// pointer, negative A, row_stride < 3 A, max_states outside 1 .. 4096, max_edges outside 1 .. 2^21; n == 0 returns
// without a device.  With the device: not a native linear batch, a frame count outside 0 .. M, more than 16384 labels, a
// table that is not device memory, an output that is not memory of the current device.  One launch, no scratch, no wait.
void batch_asg_lattice_score(const BatchP& ems, const int* frames, const float* table_dev, const int* arcs_dev,
                             int64_t row_stride, const int* num_arcs_dev, const int* num_nodes_dev,
                             const float* arc_weights_dev, int A, int max_states, int max_edges, float* scores_dev);
// The gradients for weights_dev [n], each output nullable but not all three: grad_em_dev [n][M][C] = weights[b] * d
// score[b] / d emissions (every element written, pad rows included); grad_table_dev [C + C * C] = sum_b weights[b] * d
// score[b] / d table (every element written); arc_grad_dev [n][A] = weights[b] * the posterior of the arc, zeros at or
// past num_arcs[b].  An utterance whose score is -inf or whose weight is exactly 0 adds nothing.  The alpha rows (max T_b
// * max_states floats per utterance), and with a table or arc gradient one cell per edge (max_edges floats) plus five
// rows of max_states words, come from the stream-ordered pool, at most 256 MiB per launch group
// (GTNX_ASG_LATTICE_SCRATCH_BYTES lowers the cap: a debug switch); beyond it the utterances run in slices with the same
// bits, the table launch of a slice carrying on from what the one before stored.  No floating-point atomics.
void batch_asg_lattice_score_grad(const BatchP& ems, const int* frames, const float* table_dev, const int* arcs_dev,
                                  int64_t row_stride, const int* num_arcs_dev, const int* num_nodes_dev,
                                  const float* arc_weights_dev, int A, int max_states, int max_edges,
                                  const float* weights_dev, float* grad_em_dev, float* grad_table_dev,
                                  float* arc_grad_dev);
void batch_asg_lattice_score_stats(int64_t* calls, int64_t* utterances);  // calls that launched / utterances they took
// The best ASG alignment of all n * N device-resident hypotheses (the pair form and the table of batch_asg_score) under
// the n emission slabs of a native linear batch, results on the device (DESIGN section 28 holds the contract): the
// outputs are those of batch_ctc_token_align, frame_tokens_dev never -1 inside a path (there is no blank).  Float32
// max-plus with the association of asg_align.hip, alpha + (w + e), of two equal candidates the step: bit-reproducible,
// scores bit-equal to batch_viterbi_align's ASG launch where both apply.  -1 / -inf wherever no path covers an entry; a
// pair has no path where batch_asg_score gives -inf.  Every element of every row is written over its width, nothing
// beyond.  No cap on C of its own: table indices are 64-bit and there is no per-label LDS row.
// Invalid argument before a device is asked for: a null table, scores, starts or ends pointer, negative out_stride or
// frame_stride, out_stride < L, then check_hypotheses; n * N == 0 returns without a device.  With the device: not a
// native linear batch, a frame count outside 0 .. M, frame_stride < M with frame tokens, a table that is not device
// memory of the current device, an output that is not memory of the current device.  The back-pointers (1 bit per
// position and frame, ceil(max T_b / 32) * max_length words per pair) come from the stream-ordered pool, at most 256 MiB
// per launch (GTNX_ASG_TOKEN_ALIGN_SCRATCH_BYTES lowers the cap: a debug switch); beyond it the pairs run in slices, same
// bits.
void batch_asg_token_align(const BatchP& ems, const int* frames, const float* table_dev, const int* tokens_dev,
                           int64_t row_stride, const int* lengths_dev, int N, int L, int max_length, float* scores_dev,
                           int* starts_dev, int* ends_dev, float* token_scores_dev, int64_t out_stride,
                           int* frame_tokens_dev, int64_t frame_stride);
void batch_asg_token_align_stats(int64_t* calls, int64_t* pairs);  // calls that launched / pairs they aligned
// items_dev (optional): device memory of the CALLER's that the n result values are written into directly (borrowed: it
// must outlive the result); a later batch_items_device to the same address copies nothing
BatchP batch_scalar(ScalarKind k, const BatchP& a, const BatchP& b, void* items_dev = nullptr);
void batch_backward(const BatchP& root, bool retain);
void batch_items_host(const BatchP& x, float* out);
void batch_items_device(const BatchP& x, void* dev_out);
void batch_grads_device(const BatchP& x, void* dev_out, const int64_t* offsets);
void batch_grads_bind(const BatchP& x, void* dev_out, const int64_t* offsets);
Graph batch_get(const BatchP& x, int i);
float batch_item_host(const BatchP& x, int i);  // x SCALAR and not materialised
void batch_prefetch_items(const BatchP& x);      // x SCALAR: start the device->host copy of its values now
// the caller's graphs as native leaves (nullptr when they do not qualify): acceptors that are each exactly
// ctcGraph(labels) of benchmarks/ctc.cpp:40-58 (Structure::ctc_labels) / linear chains of one shape whose
// weights are (made) one [n][M][C] device tensor
BatchP batch_ctc_targets_from_graphs(const std::vector<Graph>& gs);
BatchP batch_linear_from_graphs(const std::vector<Graph>& gs);
void batch_materialise(Batch& x);

} // namespace gtnx
