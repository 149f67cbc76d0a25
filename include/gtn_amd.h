/*
 * gtn_amd.h -- C ABI of the MI355X-native WFST engine (libgtn_amd.so).
 *
 * The reference (facebookresearch/gtn) has no FFI layer of its own: its
 * language binding (bindings/python/gtn/_*.cpp, pybind11) binds the public C++
 * API of libgtn directly.  This header is therefore the C restatement of that
 * public API for the hot path, one entry point per reference member/function,
 * each citing what it replaces.  Everything crossing the boundary is a plain
 * pointer, an integer or an opaque handle; no C++/HIP/torch types.
 *
 * Conventions
 *  - every call returns gtnx_status_t; GTNX_OK == 0.  On failure the message is
 *    available (thread-local) from gtnx_last_error().  Status codes map 1:1 to
 *    the exception types the reference throws (see below); the header-only C++
 *    shim in include/gtn/ rethrows them.
 *  - gtnx_graph_t is an owning reference to a graph *value handle* with the
 *    reference's aliasing semantics (gtn/graph.h:461-464): gtnx_graph_copy()
 *    aliases structure, weights and grad; gtnx_graph_deep_copy() detaches.
 *  - the "_n" forms take arrays of n handles and run ONE batched device launch
 *    per kernel for the whole array.  They are the device analogue of the
 *    reference's batch entry points: the std::vector<Graph> overloads of the
 *    Python binding (bindings/python/gtn/_functions.cpp:84-135) which call
 *    parallelMap (gtn/parallel/parallel_map.h:153-188).  An input array of
 *    length 1 is broadcast, as parallelMap does (parallel_map.h:77-89).
 *  - device pointers are raw HIP device addresses (e.g. torch.Tensor.data_ptr()
 *    on a ROCm tensor); a stream is a hipStream_t passed as void*.
 */
#ifndef GTN_AMD_H
#define GTN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int gtnx_status_t;
#define GTNX_OK 0
#define GTNX_INVALID_ARGUMENT 1 /* std::invalid_argument  (shortest.cpp:149-152, autograd.cpp:43-45, graph.cpp:70-73) */
#define GTNX_LOGIC_ERROR 2      /* std::logic_error       (graph.cpp:82-95, functions.cpp:19-21,33-35,49-51) */
#define GTNX_RUNTIME_ERROR 3    /* std::runtime_error     (parallel_map.h:85-88) */
#define GTNX_OUT_OF_RANGE 4     /* std::out_of_range      (bad node / arc index; the reference only asserts) */
#define GTNX_DEVICE_ERROR 5     /* HIP failure or no usable gfx950 device; std::runtime_error in the C++ shim */

typedef struct gtnx_graph_s* gtnx_graph_t;

#define GTNX_EPSILON (-1) /* gtn/graph.h:21 */

/* ------------------------------------------------------------------ runtime */
const char* gtnx_last_error(void);
const char* gtnx_version(void);
/* "hip:gfx950" for libgtn_amd.so; the reference-backed test shim
 * (oracle/_ref/libgtn_ref.so) answers "reference-cpu". */
const char* gtnx_backend(void);
int gtnx_device_count(void);                /* 0 when no GPU is visible */
/* The device of the CALLING THREAD (hipSetDevice + the engine's per-device context: stream, memory pools).  A thread
 * that never chose is on the process default: the device of the first gtnx_set_device call, else the device the
 * first calling thread ALREADY has with HIP (a rank that only did torch.cuda.set_device(k) works on k and stays on k),
 * never a silent 0.  Every entry point tells HIP the engine's device again (a hipSetDevice by the host framework on the
 * same thread is not trusted to have been undone).  One rank per GPU (torch.distributed) sets it once; a host that
 * drives several GPUs gives each its own thread (gtn::parallelMapSharded,
 * include/gtn/parallel.h; the pool threads of a parallelMap are put on the device of the thread that called it).
 * Graphs live on the device they were made on: using one from a thread on another device is GTNX_INVALID_ARGUMENT. */
gtnx_status_t gtnx_set_device(int device);
gtnx_status_t gtnx_get_device(int* device);
gtnx_status_t gtnx_set_stream(void* hip_stream); /* NULL = the engine's own stream */
gtnx_status_t gtnx_synchronize(void);
/* How compose / intersect of an implicit emissions chain with an epsilon-free graph treat their
 * result, for the calling thread.  0: build it, unless the batch would not fit in memory.
 * 1: keep it symbolic whenever eligible.  2: keep it symbolic when the per-utterance sweep kernels
 * apply (partner of <= 512 nodes and <= 4 arcs per node: CTC targets).  -1 (default, "nobody asked"): as 2
 * when the partner is a graph the caller built on the host, else as 0.  The mode of the thread that CALLS
 * gtn::parallelMap goes with the tasks (include/gtn/parallel.h sets it on the pool's threads; a call made inside a
 * region runs under the mode it was recorded with -- 0 builds every composition there too).  A symbolic result supports
 * forwardScore / viterbiScore / viterbiPath and backward through them; any other use builds it.  What
 * a symbolic result does not have is its OWN gradient graph (Graph::grad() of the composition), so
 * this is a hint for criteria that never read it.  `previous` (may be NULL) receives the old mode.
 * The environment variable GTNX_LAZY_COMPOSE (0 / 1 / 2) overrides the hint. */
gtnx_status_t gtnx_compose_mode(int mode, int* previous);
/* bytes currently held by the engine's device arena pool / bytes in use */
gtnx_status_t gtnx_memory_stats(uint64_t* reserved, uint64_t* in_use);
/* Takes apart EVERY thread's deferred garbage (also that of threads which never come to a reclamation point), waits
 * for the stream and gives the pooled device and pinned blocks back to the HIP runtime; also what an allocation does
 * by itself before it reports out-of-memory. */
gtnx_status_t gtnx_empty_cache(void);
/* Destroys what the CALLING THREAD has let go of, or built for others and nobody refers to any more, since its last
 * reclamation point (released handles, finished tapes, the recorded calls of a parallelMap region); never waits for
 * the GPU, cheap when nothing is pending.  Every thread takes apart what it allocated: the engine reclaims by itself
 * wherever a thread would wait for the device and whenever a thread's own list stands for more than 8 192 graphs
 * (GTNX_DEFER_FULL); the pool threads of include/gtn/parallel.h call this when their share of a region is done.  A
 * thread's list takes at most 16 384 objects from OTHER threads: beyond that the thread that lets go destroys. */
gtnx_status_t gtnx_reclaim(void);
/* The calling thread is one of several host threads mapping per-graph functions over a batch
 * (gtn::parallelMap, parallel/parallel_map.h:153-188) from here until gtnx_parallel_leave: its
 * function calls (negate .. viterbiPath, backward) are DEFERRED -- they return placeholder handles at
 * once, no thread waits for another -- and gtnx_parallel_flush, called by the thread that joins the
 * region (parallel_map.h:182-186), runs the calls of all the region's threads as ONE batched launch per
 * function; a criterion step over CTC-shaped targets and linear emission graphs runs as the batch records
 * below.  Results per graph are unchanged: a placeholder that is looked at before the join (sizes, arcs,
 * item(), a gradient) runs what it depends on right then, and a graph that is changed while a deferred call
 * still reads it has those calls run first.  What moves is when an error surfaces: at the first look at the
 * result, or from gtnx_parallel_flush (parallelMap rethrows after its join either way).  setWeights inside
 * a region copies a host source at the call (graph.cpp:179-181) and reads a DEVICE source at the join, with one
 * launch for the whole region: LIFETIME REQUIREMENT -- a device buffer handed to setWeights inside a parallelMap
 * task must stay allocated and unchanged until that parallelMap call returns (rows of a tensor that outlives the
 * call, as in pytorch_loss.py:46-71, are; a buffer the task itself frees or overwrites is not).
 * GTNX_REGION_EAGER_WEIGHTS=1 copies at the call instead, like the reference, one launch per call.  Inputs of the
 * recorded calls stay referenced until the results of the thread that recorded them are released.
 * Made by include/gtn/parallel.h; a hint -- without it every call is a batch of one. */
gtnx_status_t gtnx_parallel_enter(void);
gtnx_status_t gtnx_parallel_leave(void);
gtnx_status_t gtnx_parallel_flush(void);

/* ------------------------------------------------------------------ Graph
 * class Graph, gtn/graph.h:75-415 */
gtnx_status_t gtnx_graph_create(int calc_grad, gtnx_graph_t* out);          /* graph.h:89  */
gtnx_status_t gtnx_graph_copy(gtnx_graph_t g, gtnx_graph_t* out);           /* copy-ctor: alias */
gtnx_status_t gtnx_graph_deep_copy(gtnx_graph_t g, gtnx_graph_t* out);      /* graph.h:150 */
gtnx_status_t gtnx_graph_destroy(gtnx_graph_t g);
gtnx_status_t gtnx_graph_add_node(gtnx_graph_t g, int start, int accept, int* id);      /* graph.h:97 */
gtnx_status_t gtnx_graph_add_arc(gtnx_graph_t g, int src, int dst, int ilabel,
                                 int olabel, float weight, int* id);                    /* graph.h:118-123 */
/* bulk forms of the two above (same order semantics as n successive calls) */
gtnx_status_t gtnx_graph_add_nodes(gtnx_graph_t g, int n, const uint8_t* start,
                                   const uint8_t* accept);
gtnx_status_t gtnx_graph_add_arcs(gtnx_graph_t g, int n, const int* src,
                                  const int* dst, const int* ilabel,
                                  const int* olabel, const float* weight /* NULL = 0 */);
gtnx_status_t gtnx_graph_num_nodes(gtnx_graph_t g, int64_t* out);   /* graph.h:130 */
gtnx_status_t gtnx_graph_num_arcs(gtnx_graph_t g, int64_t* out);    /* graph.h:126 */
gtnx_status_t gtnx_graph_num_start(gtnx_graph_t g, int64_t* out);   /* graph.h:134 */
gtnx_status_t gtnx_graph_num_accept(gtnx_graph_t g, int64_t* out);  /* graph.h:138 */
gtnx_status_t gtnx_graph_item(gtnx_graph_t g, float* out);          /* graph.h:143; sync point */
gtnx_status_t gtnx_graph_arc_sort(gtnx_graph_t g, int olabel);      /* graph.h:158 */
gtnx_status_t gtnx_graph_mark_arc_sorted(gtnx_graph_t g, int olabel); /* graph.h:166 */
gtnx_status_t gtnx_graph_ilabel_sorted(gtnx_graph_t g, int* out);   /* graph.h:178 */
gtnx_status_t gtnx_graph_olabel_sorted(gtnx_graph_t g, int* out);   /* graph.h:186 */
/* weights(): a pointer into the live host buffer of numArcs floats (graph.h:194-204).
 * Forces a device->host sync when the weights were produced on the GPU; the
 * non-const form marks the host copy authoritative. */
gtnx_status_t gtnx_graph_weights(gtnx_graph_t g, int mutable_, float** out);
gtnx_status_t gtnx_graph_get_weights(gtnx_graph_t g, float* out);   /* copy-out of the above */
/* graph.h:210; `weights` may also be a DEVICE address (detected: hipPointerGetAttributes) -- then as below.  Copies at
 * the call, except inside a parallelMap region with a device source: see gtnx_parallel_enter for the lifetime rule. */
gtnx_status_t gtnx_graph_set_weights(gtnx_graph_t g, const float* weights);
/* the same copy from a DEVICE buffer of numArcs floats (no host round-trip;
 * replaces pytorch_loss.py:53-61's inputs.cpu() + set_weights(data_ptr)) */
gtnx_status_t gtnx_graph_set_weights_device(gtnx_graph_t g, const void* device_weights);
/* device address of the weight buffer (numArcs floats), uploading if needed */
gtnx_status_t gtnx_graph_weights_device(gtnx_graph_t g, void** out);
gtnx_status_t gtnx_graph_labels_to_array(gtnx_graph_t g, int* out, int ilabel); /* graph.h:219 */
/* node accessors, graph.h:330-376 */
gtnx_status_t gtnx_graph_get_start(gtnx_graph_t g, int* out);   /* numStart ints  */
gtnx_status_t gtnx_graph_get_accept(gtnx_graph_t g, int* out);  /* numAccept ints */
gtnx_status_t gtnx_graph_is_start(gtnx_graph_t g, int node, int* out);
gtnx_status_t gtnx_graph_is_accept(gtnx_graph_t g, int node, int* out);
gtnx_status_t gtnx_graph_make_accept(gtnx_graph_t g, int node);
gtnx_status_t gtnx_graph_num_out(gtnx_graph_t g, int node, int64_t* out);
gtnx_status_t gtnx_graph_num_in(gtnx_graph_t g, int node, int64_t* out);
gtnx_status_t gtnx_graph_get_out(gtnx_graph_t g, int node, int* out); /* numOut arc ids, list order */
gtnx_status_t gtnx_graph_get_in(gtnx_graph_t g, int node, int* out);  /* numIn arc ids, list order  */
/* arc accessors, graph.h:384-414 (bulk; any pointer may be NULL) */
gtnx_status_t gtnx_graph_get_arcs(gtnx_graph_t g, int* src, int* dst, int* ilabel, int* olabel);
gtnx_status_t gtnx_graph_get_arc(gtnx_graph_t g, int arc, int* src, int* dst,
                                 int* ilabel, int* olabel, float* weight);
gtnx_status_t gtnx_graph_set_weight(gtnx_graph_t g, int arc, float weight);
/* autograd members, graph.h:244-321 */
gtnx_status_t gtnx_graph_calc_grad(gtnx_graph_t g, int* out);
gtnx_status_t gtnx_graph_set_calc_grad(gtnx_graph_t g, int calc_grad);
gtnx_status_t gtnx_graph_is_grad_available(gtnx_graph_t g, int* out);
gtnx_status_t gtnx_graph_grad(gtnx_graph_t g, gtnx_graph_t* out);  /* new handle aliasing the grad graph */
gtnx_status_t gtnx_graph_zero_grad(gtnx_graph_t g);
gtnx_status_t gtnx_graph_add_grad(gtnx_graph_t g, const float* host_grad, int64_t n); /* graph.h:244-250 */
gtnx_status_t gtnx_graph_add_grad_graph(gtnx_graph_t g, gtnx_graph_t other);           /* graph.h:256 */
gtnx_status_t gtnx_graph_id(gtnx_graph_t g, uintptr_t* out);                            /* graph.h:281 */
/* Graph(GradFunc, inputs), graph.h:76-78: a user-defined differentiable op.
 * grad_fn(ctx, inputs, n_inputs, deltas) is called by gtnx_backward on the host;
 * ctx_free(ctx) when the op is released (either may be NULL). */
typedef gtnx_status_t (*gtnx_grad_fn)(void* ctx, gtnx_graph_t* inputs, int n_inputs, gtnx_graph_t deltas);
gtnx_status_t gtnx_graph_create_op(gtnx_graph_t* inputs, int n_inputs, gtnx_grad_fn grad_fn,
                                   void* ctx, void (*ctx_free)(void*), gtnx_graph_t* out);
gtnx_status_t gtnx_graph_num_inputs(gtnx_graph_t g, int64_t* out);                      /* graph.h:303 */
gtnx_status_t gtnx_graph_get_input(gtnx_graph_t g, int i, gtnx_graph_t* out);           /* graph.h:303 (new handle) */
gtnx_status_t gtnx_graph_set_inputs(gtnx_graph_t g, const gtnx_graph_t* inputs, int n); /* graph.h:311 */
gtnx_status_t gtnx_graph_set_grad_fn(gtnx_graph_t g, gtnx_grad_fn grad_fn, void* ctx,
                                     void (*ctx_free)(void*));                          /* graph.h:293 */
gtnx_status_t gtnx_graph_has_grad_fn(gtnx_graph_t g, int* out);                         /* graph.h:286 */

/* ------------------------------------------------------------------ creations
 * gtn/creations.h:25,32 */
gtnx_status_t gtnx_scalar_graph(float value, int calc_grad, gtnx_graph_t* out);
gtnx_status_t gtnx_linear_graph(int M, int N, int calc_grad, gtnx_graph_t* out);
/* B linear graphs whose weights are COPIED from one contiguous device tensor
 * [B][M][N] (the (B,T,C) emissions of pytorch_loss.py:46-71), one launch. */
gtnx_status_t gtnx_linear_graph_n(int B, int M, int N, int calc_grad,
                                  const void* device_weights, gtnx_graph_t* out /* B handles */);
/* The same without the copy: the graphs' weights ARE the caller's tensor (what a
 * torch.autograd.Function holds on to between forward and backward anyway,
 * pytorch_loss.py:46-71).  The caller keeps it alive and unchanged while any of the
 * handles -- or a result computed from them -- is in use. */
gtnx_status_t gtnx_linear_graph_borrow_n(int B, int M, int N, int calc_grad,
                                         const void* device_weights, gtnx_graph_t* out /* B handles */);

/* ------------------------------------------------------------------ functions
 * gtn/functions.h:19-152.  Single-graph forms, then batched forms. */
gtnx_status_t gtnx_negate(gtnx_graph_t g, gtnx_graph_t* out);                   /* functions.cpp:18-30 */
gtnx_status_t gtnx_add(gtnx_graph_t a, gtnx_graph_t b, gtnx_graph_t* out);      /* functions.cpp:32-46 */
gtnx_status_t gtnx_subtract(gtnx_graph_t a, gtnx_graph_t b, gtnx_graph_t* out); /* functions.cpp:48-64 */
gtnx_status_t gtnx_compose(gtnx_graph_t a, gtnx_graph_t b, gtnx_graph_t* out);  /* functions.cpp:225-237 */
gtnx_status_t gtnx_intersect(gtnx_graph_t a, gtnx_graph_t b, gtnx_graph_t* out);/* functions.cpp:239-251 */
gtnx_status_t gtnx_forward_score(gtnx_graph_t g, gtnx_graph_t* out);            /* functions.cpp:320-322 */
gtnx_status_t gtnx_viterbi_score(gtnx_graph_t g, gtnx_graph_t* out);            /* functions.cpp:324-326 */
gtnx_status_t gtnx_viterbi_path(gtnx_graph_t g, gtnx_graph_t* out);             /* functions.cpp:328-330 */

gtnx_status_t gtnx_negate_n(const gtnx_graph_t* g, int n, gtnx_graph_t* out);
gtnx_status_t gtnx_add_n(const gtnx_graph_t* a, int na, const gtnx_graph_t* b, int nb, gtnx_graph_t* out);
gtnx_status_t gtnx_subtract_n(const gtnx_graph_t* a, int na, const gtnx_graph_t* b, int nb, gtnx_graph_t* out);
gtnx_status_t gtnx_compose_n(const gtnx_graph_t* a, int na, const gtnx_graph_t* b, int nb, gtnx_graph_t* out);
gtnx_status_t gtnx_intersect_n(const gtnx_graph_t* a, int na, const gtnx_graph_t* b, int nb, gtnx_graph_t* out);
gtnx_status_t gtnx_forward_score_n(const gtnx_graph_t* g, int n, gtnx_graph_t* out);
gtnx_status_t gtnx_viterbi_score_n(const gtnx_graph_t* g, int n, gtnx_graph_t* out);
gtnx_status_t gtnx_viterbi_path_n(const gtnx_graph_t* g, int n, gtnx_graph_t* out);
/* item() of n single-arc graphs with one device->host copy (batched graph.h:143) */
gtnx_status_t gtnx_items_n(const gtnx_graph_t* g, int n, float* out);
/* the same, written to a DEVICE buffer of n floats without a host sync */
gtnx_status_t gtnx_items_device_n(const gtnx_graph_t* g, int n, void* device_out);
/* grad().weights() of n graphs gathered into ONE device buffer, graph i at
 * byte offset offsets[i]*4 (replaces pytorch_loss.py:94-102's per-sample
 * weights_to_numpy + torch.from_numpy + .to(device)) */
gtnx_status_t gtnx_grads_device_n(const gtnx_graph_t* g, int n, void* device_out, const int64_t* offsets);
/* Called BEFORE backward: names the device buffer gtnx_grads_device_n will be asked to
 * fill, so that kernels which produce graph i's first gradient may store it at
 * device_out + offsets[i] directly (the later gtnx_grads_device_n then finds it in
 * place and copies nothing).  A hint: results are the same without it. */
gtnx_status_t gtnx_grads_bind_device_n(const gtnx_graph_t* g, int n, void* device_out, const int64_t* offsets);

/* ------------------------------------------------------------------ rational operations
 * gtn/functions.h:45-123, functions.cpp:66-223 -- built on the device: the output's arrays are the inputs'
 * arrays copied with node offsets, epsilon connectors written from the inputs' start / accept lists,
 * adjacency lists rebuilt by a stable sort of the arc ids.  Node and arc ids as the reference numbers them;
 * gradients of the inputs are slices of the output's. */
gtnx_status_t gtnx_clone(gtnx_graph_t g, int projection /* 0 none, 1 input, 2 output */, gtnx_graph_t* out); /* functions.cpp:66-92 */
gtnx_status_t gtnx_concat(const gtnx_graph_t* g, int n, gtnx_graph_t* out);                                  /* functions.cpp:97-153 */
gtnx_status_t gtnx_closure(gtnx_graph_t g, gtnx_graph_t* out);                                               /* functions.cpp:155-189 */
gtnx_status_t gtnx_union(const gtnx_graph_t* g, int n, gtnx_graph_t* out);                                   /* functions.cpp:191-223 */
/* remove(g, ilabel, olabel): arcs carrying the label pair are contracted (breadth-first over them from every kept
 * node, the reference's node / arc order); weights are dropped and backward through the result throws, as there */
gtnx_status_t gtnx_remove(gtnx_graph_t g, int ilabel, int olabel, gtnx_graph_t* out);                        /* functions.cpp:253-318 */

/* ------------------------------------------------------------------ batch records
 * B graphs held as ONE object: what gtn::parallelMap over the per-graph functions
 * (parallel/parallel_map.h:153-188; benchmarks/ctc.cpp:150-165) returns when nobody looks at
 * the elements -- one record and one tape node per call instead of B graphs.  Elements can be
 * taken out as ordinary graphs at any time (gtnx_batch_get): the per-graph expression is then
 * built once, tape included, and everything the batch functions do not cover natively runs
 * through the vector functions above.  Results per element equal the per-graph functions'. */
typedef struct gtnx_batch_s* gtnx_batch_t;
gtnx_status_t gtnx_batch_from_graphs(const gtnx_graph_t* g, int n, gtnx_batch_t* out);
/* the CTC target acceptor of benchmarks/ctc.cpp:40-58 / examples/ctc.cpp:21-41 for n label
 * sequences (labels back to back, lengths[i] each), built on the device */
gtnx_status_t gtnx_batch_ctc_targets(const int* labels, const int* lengths, int n, int blank, int calc_grad,
                                     gtnx_batch_t* out);
/* One CTC criterion step (benchmarks/ctc.cpp:150-165 for a batch) in ONE launch: loss[b] = forwardScore(emissions_b) -
 * forwardScore(target_b o emissions_b), grad = d loss / d emissions, and -- target_grad != 0 -- the arc gradients of the
 * target acceptors (arc ids in benchmarks/ctc.cpp:40-58's addArc order; utterance b's at target_grad_dev + the number of
 * arcs of utterances 0 .. b-1; target_grad_dev may be NULL: computed and dropped).  Bit for bit what gtnx_batch_ctc_targets,
 * gtnx_batch_linear, gtnx_batch_intersect, the two gtnx_batch_forward_score, gtnx_batch_subtract_into and
 * gtnx_batch_backward compute.  emissions, loss, grad, target_grad_dev: DEVICE float [n][T][C], [n], [n][T][C], [arcs];
 * labels, lengths: host.  No batch record, no tape.  GTNX_INVALID_ARGUMENT before anything is launched for n <= 0, a
 * negative length, a null emissions / lengths / loss / grad pointer, or a batch for which gtnx_batch_ctc_loss_step_ok
 * says 0: labels outside 0 .. C-1, a target longer than 127 labels, C not a multiple of 4 or above 512, emissions or
 * grad not 16-byte aligned (such batches take the graph-level operations; gtn::criteria::ctcLossBatch decides).
 * gtnx_batch_ctc_loss_step_ok is a pure host function: no device is asked. */
gtnx_status_t gtnx_batch_ctc_loss_step(const void* emissions, const int* labels, const int* lengths, int n, int T, int C,
                                       int blank, void* loss, void* grad, int target_grad, void* target_grad_dev);
gtnx_status_t gtnx_batch_ctc_loss_step_ok(const int* labels, const int* lengths, int n, int T, int C, int blank,
                                          const void* emissions, const void* grad, int* ok);
/* compose(forceAlign(target), transitions) of examples/asg.cpp:50-68 for n label sequences, built
 * on the device: `transitions` must have the arc layout of examples/asg.cpp:36-47 over n_labels labels
 * (arc i: start -> label i; arc n_labels + i * n_labels + j: label j -> label i); its weights are
 * gathered into the acceptors' arcs and their gradients are added back into its gradient */
gtnx_status_t gtnx_batch_asg_force_align(const int* labels, const int* lengths, int n, gtnx_graph_t transitions,
                                         int n_labels, gtnx_batch_t* out);
/* n linear graphs (creations.cpp:20-33) over one device tensor [n][M][N]; borrow != 0: read in
 * place (see gtnx_linear_graph_borrow_n) */
gtnx_status_t gtnx_batch_linear(int n, int M, int N, int calc_grad, const void* device_weights, int borrow,
                                gtnx_batch_t* out);
/* ... over a PADDED tensor: element b is linearGraph(rows[b], N) over the first rows[b] rows of its [M][N] slab (rows:
 * host [n], 1 <= rows[b] <= M, else GTNX_INVALID_ARGUMENT; null: gtnx_batch_linear).  The slab stride stays M*N, and so
 * does the layout of the gradients (gtnx_batch_grads_device / _bind_device): rows [rows[b], M) of element b's gradient
 * are 0, and the values of the pad rows are never read.  gtnx_batch_viterbi_align with frames == NULL aligns rows[b]
 * frames; frames[b] > rows[b] is GTNX_INVALID_ARGUMENT. */
gtnx_status_t gtnx_batch_linear_rows(int n, int M, int N, const int* rows, int calc_grad, const void* device_weights,
                                     int borrow, gtnx_batch_t* out);
gtnx_status_t gtnx_batch_destroy(gtnx_batch_t b);
gtnx_status_t gtnx_batch_size(gtnx_batch_t b, int* out);
gtnx_status_t gtnx_batch_get(gtnx_batch_t b, int i, gtnx_graph_t* out);               /* new handle */
gtnx_status_t gtnx_batch_negate(gtnx_batch_t a, gtnx_batch_t* out);                   /* functions.cpp:18-30 */
gtnx_status_t gtnx_batch_add(gtnx_batch_t a, gtnx_batch_t b, gtnx_batch_t* out);      /* functions.cpp:32-46 */
gtnx_status_t gtnx_batch_subtract(gtnx_batch_t a, gtnx_batch_t b, gtnx_batch_t* out); /* functions.cpp:48-64 */
/* subtract with the n result values written straight into the caller's device memory (borrowed: it must outlive the
 * result batch) -- a criterion's losses land where the caller wants them without a copy; gtnx_batch_items_device to the
 * same address is then a no-op */
gtnx_status_t gtnx_batch_subtract_into(gtnx_batch_t a, gtnx_batch_t b, void* items_device, gtnx_batch_t* out);
gtnx_status_t gtnx_batch_compose(gtnx_batch_t a, gtnx_batch_t b, gtnx_batch_t* out);  /* functions.cpp:225-237 */
gtnx_status_t gtnx_batch_intersect(gtnx_batch_t a, gtnx_batch_t b, gtnx_batch_t* out);/* functions.cpp:239-251 */
gtnx_status_t gtnx_batch_forward_score(gtnx_batch_t a, gtnx_batch_t* out);            /* functions.cpp:320-322 */
gtnx_status_t gtnx_batch_viterbi_score(gtnx_batch_t a, gtnx_batch_t* out);            /* functions.cpp:324-326 */
gtnx_status_t gtnx_batch_viterbi_path(gtnx_batch_t a, gtnx_batch_t* out);             /* functions.cpp:328-330 */
/* Forced alignment with device-resident output: what a caller of the reference gets from viterbiPath
 * (shortest.cpp:190-272) plus the per-utterance host loop written around it (read every path graph's arc labels, pad,
 * upload), as one call that leaves the results in the caller's device memory.  Row b of labels_device
 * (int32, row_stride entries apart) receives the label of every frame on utterance b's best path and -1 from the
 * path's end on (everywhere when no accepting path exists); tokens_device (or null) likewise the index into the
 * utterance's label sequence, -1 on blank frames; scores_device (float32 [n], or null) the path's score, -inf without
 * a path.  frames (host, [n], or null): how many of the T emission rows of each utterance are aligned.
 * A composition of gtnx_batch_ctc_targets (blank below every label) with gtnx_batch_linear (alphabet a multiple of 4,
 * at most 2048; at most 512 nodes) is aligned by ONE launch on the engine's stream: nothing is copied back and the
 * call does not wait for the device.  So is a composition, in either argument order, of gtnx_batch_asg_force_align
 * over n_labels labels with gtnx_batch_linear over the same alphabet (a multiple of 4, at most 2048; targets of at most
 * 511 labels): there tokens_device is the index into the label sequence of the label the frame carries -- never -1
 * inside a path, ASG has no blanks -- and of two equal candidates the step from the previous label wins, as in the
 * reference's viterbiPath on the built lattice.  Any other batch goes through gtnx_batch_viterbi_path and one upload;
 * tokens_device and frames are GTNX_INVALID_ARGUMENT there.  Output pointers must be memory the engine's current device may write. */
gtnx_status_t gtnx_batch_viterbi_align(gtnx_batch_t a, const int* frames, void* labels_device, int64_t row_stride,
                                       void* tokens_device, void* scores_device);
/* utterances aligned so far (process-wide) by the launch / by the path-graph route */
gtnx_status_t gtnx_batch_align_stats(int64_t* fast, int64_t* fallback);
/* Decode of a whole batch against ONE shared graph with device-resident output: viterbiPath(ems_b o transitions)
 * (shortest.cpp:190-272 over compose.cpp:377-522), the call an ASG model makes at inference, without the path graphs.
 * Row b of labels_device (int32, row_stride entries apart, row_stride >= M) receives the label of every frame t < T_b of
 * utterance b's best path and -1 from T_b to the row's width M; scores_device (float32 [n], or null) the path's score;
 * collapsed_device (int32 rows like labels_device, or null) the labels with runs of equal consecutive frames merged,
 * then -1 up to M; lengths_device (int32 [n], or null; needs collapsed_device) how many.  Without an accepting path
 * (T_b = 0 included): every entry -1, score -inf, length 0.  frames (host, [n], or null): T_b; null means the rows the
 * batch carries (gtnx_batch_linear_rows; M otherwise); a count outside 0 .. M or above those rows is
 * GTNX_INVALID_ARGUMENT, raised before anything is launched.
 * ems = gtnx_batch_linear / _rows and a transitions graph of 8 .. 1024 nodes whose every node's in-arcs share one
 * label and whose nodes all reach all nodes with in-arcs, lists in node order (gtn::criteria::asgTransitions over 7 ..
 * 1023 labels, arc-sorted or not): the whole padded batch is swept ONCE at full length M -- whatever the frame counts;
 * the pad rows are read by that sweep, and what they hold (NaN included) never changes a bit of any output -- and ONE
 * launch on the engine's stream walks every utterance back from its own row T_b: nothing is copied back, no graph is
 * built and the call does not wait for the device.  Exact ties: the first accept node in the graph's accept order,
 * then the arc from the smallest source node -- the reference's choice on the built lattice of such a graph.
 * Any other graph or batch (fewer than 7 or more than 1023 labels, another shape, GTNX_NO_DENSE=1) goes through
 * gtnx_viterbi_path_n over the composed elements, the labels read and collapsed on the host, one upload; frames must be
 * null there (GTNX_INVALID_ARGUMENT otherwise).  Output pointers must be memory the engine's current device may write. */
gtnx_status_t gtnx_batch_viterbi_decode(gtnx_batch_t ems, gtnx_graph_t transitions, const int* frames,
                                        void* labels_device, int64_t row_stride, void* scores_device,
                                        void* collapsed_device, void* lengths_device);
/* utterances decoded so far (process-wide) by the launch / by the path-graph route */
gtnx_status_t gtnx_batch_decode_stats(int64_t* fast, int64_t* fallback);
/* gtnx_batch_compose / _intersect of a gtnx_batch_linear_rows batch with a one-element batch holding an ASG transitions
 * graph over the same alphabet (N + 1 nodes, N (N + 1) arcs in the order of examples/asg.cpp:36-47), in either argument
 * order, stays symbolic for N <= 128: gtnx_batch_forward_score of it is ONE launch that walks every utterance's own
 * rows (pad rows are never read), its backward two more, and the transitions graph receives one gradient summed in
 * utterance order (bit-repeatable).  Batches without row counts take that launch only under GTNX_FULL_CONNECT=1.
 * Utterances scored so far (process-wide) by the launch / padded utterances that took the composed elements instead
 * (a larger alphabet, or a consumer other than forwardScore). */
gtnx_status_t gtnx_batch_full_connect_stats(int64_t* fast, int64_t* fallback);
/* Best-path decode of a whole batch of chains with device-resident output: viterbiPath(ems_b) (shortest.cpp:190-272
 * on creations.cpp:20-33) followed by the CTC collapse (merge repeats, then drop blanks), the call a CTC model makes at
 * inference, without the path graphs.  Row b of labels_device (int32, row_stride entries apart, row_stride >= M)
 * receives for every frame t < T_b the FIRST label holding the row's maximum (the reference compares with `>` from
 * -inf: the smallest label among equal maxima; NaN and -inf are never taken) and -1 from T_b to the row's width M;
 * scores_device (float32 [n], or null) ((0 + m_0) + m_1) + ... + m_{T_b - 1} in float32 in frame order;
 * collapsed_device (int32 rows like labels_device, or null) the labels with runs of equal consecutive frames merged and
 * `blank` dropped (blank < 0: nothing is dropped -- viterbiPath of a linear graph, nothing CTC about it), then -1 up to
 * M; starts_device (rows alike, or null; needs collapsed_device) the first frame of each kept label, then -1;
 * lengths_device (int32 [n], or null; needs collapsed_device) how many.  A frame without an entry above -inf leaves
 * no path: every entry of every row -1, score -inf, length 0.  T_b = 0 likewise: linearGraph(0, C) is a start node that
 * does not accept (creations.cpp:22).
 * frames (host, [n], or null): T_b; null means the rows the batch carries (gtnx_batch_linear_rows; M otherwise).
 * GTNX_INVALID_ARGUMENT, raised before a device is asked for: a null batch or labels pointer, a negative stride,
 * lengths or starts without collapsed, a count outside 0 .. M or above the rows the batch carries, row_stride < M,
 * blank >= C.
 * ems = gtnx_batch_linear / _rows: two launches on the engine's stream (every emission of the rows that count is read
 * once; rows from T_b on are never read), nothing is copied back, no graph is built and the call does not wait for
 * the device.  Any other batch goes through gtnx_batch_viterbi_path, the labels read and collapsed on the host by the
 * same rules, one upload; frames must be null there (GTNX_INVALID_ARGUMENT otherwise).  Output pointers must be memory
 * the engine's current device may write. */
gtnx_status_t gtnx_batch_linear_decode(gtnx_batch_t ems, const int* frames, int blank, void* labels_device,
                                       int64_t row_stride, void* scores_device, void* collapsed_device,
                                       void* starts_device, void* lengths_device);
/* utterances decoded so far (process-wide) by the launches / by the path-graph route */
gtnx_status_t gtnx_batch_linear_decode_stats(int64_t* fast, int64_t* fallback);
/* num_samples alignments of every chain of a batch drawn from its frame posteriors, plus the CTC collapse, results left
 * on the device: exact samples of P(y | x) of a CTC model, whose frames are independent (DESIGN section 32 has the
 * whole contract).  For utterance b, sample k and frame t < T_b the label is c with probability
 * exp(x[b,t,c] / temperature) / Z[b,t], independently, Z[b,t] the sum over the entries that carry mass.
 *   Mass: only finite entries carry mass; -inf, +inf and NaN are never chosen and are left out of Z.  A frame without a
 *   finite entry, or T_b == 0, leaves the utterance without a path: every sample of it gets -1 rows, length 0 and
 *   logq = -inf (what gtnx_batch_linear_decode does).  No output is ever NaN.
 *   Draw: inverse CDF in label order.  With u the uniform of (b, k, t), the label is the smallest c whose cumulative
 *   mass over labels 0 .. c exceeds u * Z; if rounding leaves none, the last label with mass.  A label without mass is
 *   never returned.
 *   Randomness is counter-based: Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (t, b, k >> 2, 0);
 *   sample k uses output word k & 3, u = (2 * (word >> 9) + 1) * 2^-24, strictly inside (0, 1) and exact in float32.
 *   The same seed gives the same bytes whatever the strides, the slicing, the frame counts of the other utterances or
 *   the contents of pad rows, and the first N samples of a call with more are those of a call with N.
 * tokens_device: int32 [n][num_samples][row_stride], row_stride >= M: the alignment with repeats merged and `blank`
 * dropped (blank = -1: repeats merged only), -1 from its length to M -- the layout gtnx_batch_ctc_beam_decode writes;
 * lengths_device: int32 [n][num_samples]; logq_device (may be null): float32 [n][num_samples], sum_t (x[b,t,c_t] /
 * temperature - log Z[b,t]), added in frame order from 0 in float32; labels_device (may be null): int32
 * [n][num_samples][row_stride], the frame labels, -1 from T_b to M.
 * frames (host, [n], or null): T_b; null means the rows the batch carries.  Rows from T_b on are never read.
 * GTNX_INVALID_ARGUMENT before a device is asked for: a null batch, tokens or lengths pointer, a negative stride,
 * num_samples outside 1 .. 1024, a temperature that is not finite and > 0.  With the device: ems is not a
 * gtnx_batch_linear / _rows batch (there is no other route), a count outside 0 .. M or above the rows the batch carries,
 * row_stride < M, blank >= C, n * num_samples beyond an int, outputs the engine's current device may not write.  A
 * refused call writes nothing.
 * Two launches on the engine's stream (ctc_sample.hip); the label and term of every (b, k, t) live in scratch from the
 * stream-ordered pool, at most 256 MiB per launch: beyond that the utterances run in slices with the same bytes
 * (GTNX_CTC_SAMPLE_SCRATCH_BYTES, read per call, lowers the cap: a debug switch for tests).  Nothing is copied back and
 * the call does not wait for the device. */
gtnx_status_t gtnx_batch_ctc_sample(gtnx_batch_t ems, const int* frames, int blank, int num_samples, uint64_t seed,
                                    float temperature, void* tokens_device, int64_t row_stride, void* lengths_device,
                                    void* logq_device /* may be null */, void* labels_device /* may be null */);
/* calls that have launched so far (process-wide) / utterances they sampled */
gtnx_status_t gtnx_batch_ctc_sample_stats(int64_t* calls, int64_t* utterances);
/* CTC prefix beam search with N-best output over a whole batch of chains, results left on the device: the best LABEL
 * SEQUENCES, summed over their alignments, where gtnx_batch_linear_decode gives the best alignment.  Per frame the
 * token set is the cutoff_top_n best labels of the row (value descending, of equal values the smaller label; NaN and
 * -inf are never chosen) plus `blank` where its entry is above -inf; the state is at most beam_size distinct prefixes
 * with the log scores (pb, pnb) of their alignments that end / do not end in blank, starting from the empty prefix with
 * (0, -inf); a frame gives every prefix a stay candidate and one extension per non-blank member of the set, an
 * extension that is a prefix of the list already is added into that prefix (exact prefix identity, not hashed), and
 * the first beam_size candidates by (total descending, stay before extension, parent's rank, label) are the new list.
 * log-add is m + log1p(exp(n - m)) in float32 (DESIGN section 20 has the whole contract; unpruned, a hypothesis's score
 * is forwardScore(ctcTarget(y) intersected with emissions_b)).
 * tokens_device: int32 [n][nbest][row_stride], row_stride >= M: the labels of hypothesis r, -1 from its length to M;
 * lengths_device: int32 [n][nbest]; scores_device: float32 [n][nbest].  Slots without a hypothesis -- fewer than nbest
 * prefixes, a frame without anything above -inf, T_b = 0 (linearGraph(0, C) does not accept) -- get -1, 0 and -inf.
 * frames (host, [n], or null): T_b; null means the rows the batch carries.  Rows from T_b on are never read.
 * GTNX_INVALID_ARGUMENT before a device is asked for: a null batch or output pointer, a negative stride, beam_size
 * outside 1 .. 64, cutoff_top_n outside 1 .. 32, nbest outside 1 .. beam_size, a negative blank.  With the device: ems is
 * not a gtnx_batch_linear / _rows batch (there is no other route), a count outside 0 .. M or above the rows the batch
 * carries, row_stride < M, blank >= C, more than 2^25 labels, outputs the engine's current device may not write.
 * Two launches on the engine's stream (ctc_beam.hip), scratch from the stream-ordered pool, nothing is copied back
 * and the call does not wait for the device. */
gtnx_status_t gtnx_batch_ctc_beam_decode(gtnx_batch_t ems, const int* frames, int blank, int beam_size,
                                         int cutoff_top_n, int nbest, void* tokens_device, int64_t row_stride,
                                         void* lengths_device, void* scores_device);
/* gtnx_batch_ctc_beam_decode with a bigram over the labels fused into the ranking.
 * lm_device: DEVICE float32 [C + C * C] in the arc order of gtn::criteria::asgTransitions: lm[c] is the score of c as
 * first label, lm[C + i * C + j] the score of label j followed by label i -- the tables asg_loss learns. Every prefix
 * y carries L(y) = sum_k (lm_weight * lm(y_{k-1} -> y_k) + insertion_bonus), float32, accumulated left to right;
 * L(()) = 0.
 * Everything above holds with these changes: a candidate ranks by its acoustic total plus L of its prefix (a stay by
 * logadd(pb', pnb') + L(y), an extension of y by c by s + (L(y) + inc), s as above; the same order; a candidate whose
 * acoustic total is -inf is dropped as above); an extension whose inc is -inf, +inf or NaN is dropped, so a -inf entry
 * forbids a bigram or a first label; rows and columns of `blank` are never read; an extension that joins a prefix of
 * the list adds acoustic mass only; the cutoff_top_n pruning of a row and (pb, pnb) stay acoustic; a prefix that
 * leaves the list and is created again gets the same L bit for bit.
 * scores_device: float32 [n][nbest], acoustic total + L; am_scores_device (may be null): float32 [n][nbest], the
 * acoustic total alone -- unpruned, what gtnx_batch_ctc_score gives for those tokens. Slots without a hypothesis get
 * -1, 0, -inf, -inf. With lm_weight = insertion_bonus = 0 and a finite table every output is byte-identical to
 * gtnx_batch_ctc_beam_decode and am_scores to scores.
 * GTNX_INVALID_ARGUMENT on top of gtnx_batch_ctc_beam_decode's, before a device is asked for: a null lm_device, an
 * lm_weight or insertion_bonus that is not finite; with the device: more than 2^19 labels (such a table has no device
 * to live on); lm_device is anything but memory allocated on the engine's current device -- the kernel gathers from
 * it, so pageable host memory is refused with one GPU as well, and so are pinned or registered host memory and managed
 * memory, which a kernel could read: copy such a table to the device first; am_scores_device is memory the device may
 * not write. Nothing is written by a refused call. Counted by gtnx_batch_ctc_beam_stats. */
gtnx_status_t gtnx_batch_ctc_beam_decode_lm(gtnx_batch_t ems, const int* frames, int blank, int beam_size,
                                            int cutoff_top_n, int nbest, const void* lm_device, float lm_weight,
                                            float insertion_bonus, void* tokens_device, int64_t row_stride,
                                            void* lengths_device, void* scores_device,
                                            void* am_scores_device /* may be null */);
/* A language model held as a graph, compiled for the search above: a deterministic acceptor with
 * back-off (failure) arcs -- an n-gram model in ARPA form, or a lexicon or grammar acceptor that forbids sequences.
 * gtnx_lm_graph_create reads the input labels of g's arcs (output labels and accept flags are ignored: an n-gram
 * acceptor accepts everywhere, and end-of-sentence handling is out of scope) and its weights AS THEY ARE AT THAT
 * MOMENT: a snapshot, later changes of g are not seen, and there is no autograd. The arcs need not be sorted. It is
 * host work and needs no device; the compiled form is uploaded once, by the first decode that uses it, which waits for
 * that copy.
 * Walk semantics, the same on host and device. From state s with label c: if s has an arc labelled c, add its weight
 * and move to its destination; otherwise, if s has an epsilon arc (label -1, gtn::epsilon), add its weight, go to its
 * destination and repeat; if neither exists, c is forbidden from s. The weight of a walk is the float32 sum of the
 * walked weights in walk order, starting from the first one. These are failure (phi) semantics, what ARPA back-off
 * means -- not what compose does with epsilon, where the direct arc and the back-off path would both count.
 * GTNX_INVALID_ARGUMENT, with a message, nothing is repaired: no start node or more than one; two arcs with the same
 * input label out of one node; more than one epsilon arc out of a node; an epsilon chain that is cyclic or longer than
 * 8 arcs; a label below -1; more than 2^24 nodes; a linear graph. */
typedef struct gtnx_lm_graph_s* gtnx_lm_graph_t;
typedef struct {
  int64_t num_states;        /* the nodes of the graph */
  int64_t num_arcs;          /* its arcs, epsilon arcs included */
  int32_t start_state;
  int32_t longest_epsilon_chain; /* epsilon arcs on the longest back-off chain, 0 .. 8 */
} gtnx_lm_graph_info_t;
gtnx_status_t gtnx_lm_graph_create(gtnx_graph_t g, gtnx_lm_graph_t* out);
gtnx_status_t gtnx_lm_graph_destroy(gtnx_lm_graph_t lm); /* null: nothing; a handle that is not live is refused */
/* the host-side probe: the walk of `label` from `state`. A forbidden label gives *weight = -inf and *next_state = -1;
 * a walk that is found may still have a weight that is not finite, which the search drops. GTNX_OUT_OF_RANGE for a
 * state that is none; a label below 0 is forbidden. */
gtnx_status_t gtnx_lm_graph_walk(gtnx_lm_graph_t lm, int state, int label, float* weight, int* next_state);
gtnx_status_t gtnx_lm_graph_info(gtnx_lm_graph_t lm, gtnx_lm_graph_info_t* out);
/* gtnx_batch_ctc_beam_decode_lm with a compiled LM graph in the table's place. Every prefix also carries its LM state:
 * the empty prefix the start state; an extension of y by c walks (state(y), c) and gets
 * inc = lm_weight * (weight of the walk) + insertion_bonus (the product rounded, then the sum) and the walk's
 * destination as its state. A label that is forbidden, or whose walk weight is not finite, is dropped as a -inf table
 * entry is. `blank` and labels outside the token set are never walked, so arcs labelled blank or >= C are never found.
 * The graph is deterministic, so equal prefixes have equal states and equal L: the total order, prefix identity and
 * all four outputs are as with the table, and a graph that spells a bigram table gives byte-identical results.
 * GTNX_INVALID_ARGUMENT on top of gtnx_batch_ctc_beam_decode's, before a device is asked for: a null, destroyed or
 * foreign lm_graph, an lm_weight or insertion_bonus that is not finite; with the device: more than 2^19 labels, a
 * graph that was uploaded to another device. Nothing is written by a refused call. */
gtnx_status_t gtnx_batch_ctc_beam_decode_graph(gtnx_batch_t ems, const int* frames, int blank, int beam_size,
                                               int cutoff_top_n, int nbest, gtnx_lm_graph_t lm_graph, float lm_weight,
                                               float insertion_bonus, void* tokens_device, int64_t row_stride,
                                               void* lengths_device, void* scores_device,
                                               void* am_scores_device /* may be null */);
/* calls that have launched so far (process-wide) / utterances they decoded */
gtnx_status_t gtnx_batch_ctc_beam_stats(int64_t* calls, int64_t* utterances);
/* Levenshtein distance of all B * N pairs (hyp[b, k], ref[b]) of token rows that live on the device, results left on
 * the device: what examples/edit_distance.cpp computes as -viterbiScore(compose(hyp, compose(edits, ref))), without the
 * edits graph of alphabet^2 arcs.  Unit costs for substitution, insertion and deletion; tokens are compared with ==
 * only, any int32 is a token and there is no alphabet size.
 * hyp_device: int32, B * N rows of width L, hyp_stride (>= L) elements apart; hyp_lengths_device: int32 [B][N], dense;
 * ref_device: int32, B rows of width U, ref_stride (>= U) apart; ref_lengths_device: int32 [B], dense.  The lengths are
 * DEVICE memory (what gtnx_batch_linear_decode / gtnx_batch_ctc_beam_decode wrote): the host never sees them.  The
 * kernel clamps a length to 0 .. L (0 .. U), a negative one counts as 0, and elements at or past the clamped length
 * are never read -- a beam-search slot without a hypothesis (length 0, tokens -1) scores ref's length.
 * dist_device: int32 [B][N].  ops_device: int32 [B][N][3] = (substitutions, deletions, insertions), or null to skip
 * it; a deletion is a reference token without a hypothesis counterpart, an insertion the converse.  The counts are
 * those of ONE alignment: with D[i][j] the distance of ref[:i] and hyp[:j], walk back from (len_ref, len_hyp) and take
 * at every cell the first move that attains D[i][j] of: diagonal (a match where the tokens are equal, else a
 * substitution), up (a deletion), left (an insertion).  S + D + I == dist.  With ops null nothing is stored for the walk.
 * GTNX_INVALID_ARGUMENT before a device is asked for: a null input or dist pointer, negative B, N, L or U, a negative
 * stride or one shorter than its width, L > 65536, U > 4096 (the limits of the implementation: the carries of a row of
 * columns and the reference live in LDS, a lane owns one block of 64 reference tokens), B * N beyond an int.  B * N == 0
 * returns without touching a device.  With the device: an output the engine's current device may not write.
 * One launch on the engine's stream without ops (edit_distance.hip).  With ops the walk keeps 16 bytes * L *
 * ceil(U / 64) per pair in scratch from the stream-ordered pool, at most 256 MiB per launch: beyond that the pairs run
 * in slices of launches (the environment variable GTNX_EDIT_DISTANCE_SCRATCH_BYTES, read per call, lowers the cap: a
 * debug switch for tests).  Nothing is copied back, the call does not wait, nothing but dist and ops is written. */
gtnx_status_t gtnx_batch_edit_distance(const void* hyp_device, int64_t hyp_stride, const void* hyp_lengths_device,
                                       const void* ref_device, int64_t ref_stride, const void* ref_lengths_device,
                                       int B, int N, int L, int U, void* dist_device, void* ops_device);
/* calls that have launched so far (process-wide) / pairs they computed */
gtnx_status_t gtnx_batch_edit_distance_stats(int64_t* calls, int64_t* pairs);
/* The exact log score of all n * N hypotheses that live on the device under the n emission slabs of `ems` (a
 * gtnx_batch_linear / _rows batch, [n][M][C]), results left on the device: for pair (b, k)
 *   len = clamp(lengths[b][k], 0, L) (a negative length counts as 0), y = tokens[b][k][0 .. len), T_b = frames[b],
 *   scores[b][k] = forwardScore(ctcGraph(y, blank) o linearGraph(emissions_b[0 .. T_b)))
 * the log-sum over all alignments of the summed emissions; no normaliser is subtracted, so the CTC loss of y is
 * forwardScore(emissions_b) - scores[b][k], and an unpruned gtnx_batch_ctc_beam_decode gives the same number.  ctcGraph
 * is the acceptor of benchmarks/ctc.cpp:40-58: 2 len + 1 nodes, a skip arc only between different neighbouring labels,
 * the last two nodes accept; a token equal to `blank` is a label like any other.
 * tokens_device: int32, n * N rows of width L, row_stride (>= L) elements apart; lengths_device: int32 [n][N], dense --
 * DEVICE memory, what gtnx_batch_ctc_beam_decode wrote: the host never sees them.  frames: HOST, [n], T_b in 0 .. M, or
 * null (the rows the batch carries).  max_length (1 .. 4096) is the caller's bound on len; it, not L, sizes LDS and
 * scratch.  scores_device: float32 [n][N].
 * The score is -inf -- never NaN, and without a gradient -- when no alignment fits (len + repeats > T_b), every path
 * crosses a -inf emission, len > max_length, a token inside the length lies outside 0 .. C - 1 (checked by the kernel:
 * such an element never becomes an address), or T_b == 0.  Elements at or past a length and emission rows at or past
 * T_b are never read.  A beam-search slot without a hypothesis (length 0, tokens -1) scores as the empty sequence,
 * all blanks: a finite number -- mask such slots with the beam's own -inf.
 * GTNX_INVALID_ARGUMENT before a device is asked for: a null batch, tokens, lengths or scores pointer, negative N, L,
 * row_stride or blank, row_stride < L, max_length outside 1 .. 4096.  n * N == 0 returns without touching a device.
 * With the device: not a gtnx_batch_linear / _rows batch, a frame count outside 0 .. M, blank >= C, an output the
 * engine's current device may not write.
 * One launch on the engine's stream (ctc_score.hip), one workgroup per pair, no scratch; nothing is copied back, the
 * call does not wait, nothing but scores is written. */
gtnx_status_t gtnx_batch_ctc_score(gtnx_batch_t ems, const int* frames, int blank, const void* tokens_device,
                                   int64_t row_stride, const void* lengths_device, int N, int L, int max_length,
                                   void* scores_device);
/* The gradient of those scores: grad[b][t][c] = sum over k of weights[b][k] * d scores[b][k] / d emissions[b][t][c], for
 * caller-supplied weights_device (float32 [n][N], device memory) -- what the backward of any N-best objective needs,
 * the hypotheses weighted separately.  The inputs are those of gtnx_batch_ctc_score, with the same meaning and the same
 * refusals (weights and grad in the place of scores).  grad_device: float32 [n][M][C]; EVERY element is written: zeros
 * where nothing lands, rows at or past T_b included.  A pair whose score is -inf or whose weight is exactly 0 adds
 * nothing (0 * NaN never appears); a non-finite weight on a finite score is the caller's.
 * The call is stateless: it recomputes the alpha rows into scratch from the stream-ordered pool, max_b T_b * (2 *
 * max_length + 1) floats per pair, at most 256 MiB per pair of launches; beyond that the pairs run in slices, bit-equal
 * to the unsliced run (the environment variable GTNX_CTC_SCORE_SCRATCH_BYTES, read per call, lowers the cap: a debug
 * switch for tests); a single pair above the cap runs alone with scratch of its own size.  The sums are taken in one
 * fixed order by plain loads and stores -- within a pair and frame the states of one label ascending, the pairs of an
 * utterance in k order by one workgroup -- so the gradient has the same bits run to run; there are no floating-point
 * atomics.  n * N == 0 returns without touching a device AND WITHOUT WRITING grad. */
gtnx_status_t gtnx_batch_ctc_score_grad(gtnx_batch_t ems, const int* frames, int blank, const void* tokens_device,
                                        int64_t row_stride, const void* lengths_device, int N, int L, int max_length,
                                        const void* weights_device, void* grad_device);
/* calls of either kind that have launched so far (process-wide) / pairs they took */
gtnx_status_t gtnx_batch_ctc_score_stats(int64_t* calls, int64_t* pairs);
/* The exact CTC log score of ONE ACYCLIC TOKEN LATTICE PER UTTERANCE -- several word-piece decompositions of a
 * transcript, alternative pronunciations, optional tokens, weighted or not -- under the n emission slabs of a
 * gtnx_batch_linear / _rows batch, lattices read where they lie on the device, scores left there:
 *   scores[b] = log sum over the lattice's paths p of exp(w(p) + ctc_score(emissions_b[0 .. T_b), labels(p))),
 * every decomposition and every alignment at once, nothing subtracted.  Utterance b's lattice has K = num_nodes[b]
 * nodes (node 0 starts, node K - 1 accepts) and the arcs arcs[b][a] = (src, dst, label), a < clamp(num_arcs[b], 0, A),
 * with 0 <= src < dst < K, sorted by dst (non-decreasing) within the utterance; arc_weights[b][a] is added once per use
 * of the arc.  Equivalently scores[b] = forwardScore(G_b o emissions_b) for the CTC alignment graph G_b of the lattice:
 * one blank state per node, one token state per arc, self-loops on both, blank(src) -> token(a), token(a) -> blank(dst),
 * token(a') -> token(a) when dst(a') == src(a) and the labels differ, the arc's weight on every transition that enters
 * token(a); paths start in blank(0) before frame 0 (so frame 0 is spent in blank(0) or in a token that leaves node 0,
 * which pays its weight there) and end in blank(K - 1) or a token that enters node K - 1.  Two lattice paths that spell the same labels both count; a label equal to `blank` is a label like any other.
 * arcs_device: int32, n rows of A arcs, row_stride (>= 3 A) elements apart; num_arcs_device, num_nodes_device: int32 [n];
 * arc_weights_device: float32 [n][A] or null (all zeros) -- all DEVICE memory, none is downloaded.  frames: HOST, [n],
 * T_b in 0 .. M, or null.  max_states (1 .. 4096) is the caller's bound on K + arcs; it sizes LDS and scratch.
 * scores_device: float32 [n].  Float32, in this order (alpha' the next frame's row):
 *   token a: x = logadd(alpha[a], alpha[blank src] + w_a); for a' entering src, ascending, label(a') != label(a):
 *            x = logadd(x, alpha[a'] + w_a); alpha'[a] = x + e(t, label a)
 *   blank n: x = alpha[n]; for a' entering n, ascending: x = logadd(x, alpha[a']); alpha'[n] = x + e(t, blank)
 *   score = logadd over blank(K - 1), then the arcs entering K - 1 ascending.
 * The score is -inf -- never NaN, and without a gradient -- when T_b == 0, K < 1, K + arcs > max_states, an arc has
 * src < 0, src >= dst or dst >= K, an arc is out of dst order, a label lies outside 0 .. C - 1, a weight is +inf or NaN,
 * or no alignment fits.  A -inf weight forbids its arc.  Nodes that cannot be reached and arcs that lead nowhere are
 * legal and add nothing.  Every arc field is checked by the kernel before it becomes an address; nothing at or past
 * num_arcs[b], a frame count or a row's width is read.
 * GTNX_INVALID_ARGUMENT before a device is asked for: a null batch, arcs, num_arcs, num_nodes or scores pointer,
 * negative A or blank, row_stride < 3 A, max_states outside 1 .. 4096.  A batch without an utterance returns without
 * touching a device.  With the device: not a gtnx_batch_linear / _rows batch, a frame count outside 0 .. M, blank >= C,
 * an output the engine's current device may not write.
 * One launch on the engine's stream (ctc_lattice.hip), one workgroup per utterance, no scratch; nothing is copied back
 * and the call does not wait. */
gtnx_status_t gtnx_batch_ctc_lattice_score(gtnx_batch_t ems, const int* frames, int blank, const void* arcs_device,
                                           int64_t row_stride, const void* num_arcs_device,
                                           const void* num_nodes_device, const void* arc_weights_device, int A,
                                           int max_states, void* scores_device);
/* The gradients of those scores for caller-supplied weights_device (float32 [n], device memory; grad_out under
 * autograd).  grad_device: float32 [n][M][C] = weights[b] * d scores[b] / d emissions[b]; EVERY element is written: zeros
 * where nothing lands, rows at or past T_b included.  arc_grad_device: float32 [n][A] or null = weights[b] * d scores[b] /
 * d arc_weights[b][a], weights[b] times the posterior probability that the arc is used; entries at or past num_arcs[b]
 * are written as 0.  An utterance whose score is -inf or whose weight is exactly 0 gets zeros in both.  The inputs are
 * those of gtnx_batch_ctc_lattice_score with the same meaning and refusals (weights and grad in the place of scores).
 * The call is stateless: it recomputes the alpha rows into scratch from the stream-ordered pool, max_b T_b * max_states
 * floats per utterance, at most 256 MiB per pair of launches; beyond that the utterances run in slices, bit-equal to the
 * unsliced run (GTNX_CTC_LATTICE_SCRATCH_BYTES, read per call, lowers the cap: a debug switch for tests).  The sums are
 * taken in one fixed order by plain stores -- the blank states by lane, wave tree and waves ascending, the tokens of one
 * label ascending by arc index, the frames of an arc descending -- so both gradients have the same bits run to run;
 * there are no floating-point atomics. */
gtnx_status_t gtnx_batch_ctc_lattice_score_grad(gtnx_batch_t ems, const int* frames, int blank, const void* arcs_device,
                                                int64_t row_stride, const void* num_arcs_device,
                                                const void* num_nodes_device, const void* arc_weights_device, int A,
                                                int max_states, const void* weights_device, void* grad_device,
                                                void* arc_grad_device);
/* calls of either kind that have launched so far (process-wide) / utterances they took */
gtnx_status_t gtnx_batch_ctc_lattice_score_stats(int64_t* calls, int64_t* utterances);
/* The best (lattice path, alignment) pair of those lattices: WHICH decomposition or pronunciation the model chose and
 * WHEN each of its tokens was spoken, for every utterance in one call, results left on the device.
 * The lattice arguments, blank, frames and max_states are those of gtnx_batch_ctc_lattice_score with the same meaning,
 * the same state space (state n < K the blank of node n, state K + a the token of arc a) and the same rules about what
 * is invalid.  Float32 max-plus, the forward recurrence's candidates in its order with max for logadd:
 *   frame 0: alpha[blank 0] = e(0, blank); alpha[a] = w_a + e(0, label a) for src a == 0; -inf elsewhere
 *   token a: alpha[a] | alpha[blank src] + w_a | alpha[a'] + w_a for a' entering src, ascending, label(a') != label(a);
 *            x = their maximum; alpha'[a] = x == -inf ? -inf : x + e(t, label a)
 *   blank n: alpha[n] | alpha[a'] for a' entering n, ascending; alpha'[n] likewise with e(t, blank)
 *   end:     alpha[blank(K - 1)] | alpha[a'] for a' entering K - 1, ascending; the score is their maximum
 * An addition with a -inf operand gives -inf.  Of the candidates that reach the maximum the FIRST in that order wins (a
 * later one replaces it only if strictly greater), a -inf candidate is never chosen and a state whose maximum is -inf is
 * dead: this project's own rule (the reference has no canonical alignment graph of a lattice).  Every output is
 * reproducible bit for bit; a chain lattice without weights has the score bits of gtnx_batch_ctc_token_align.
 *   scores_device       float32 [n]: the best w(p) + alignment score, -inf without a path
 *   path_len_device     int32 [n]: the arcs on the best lattice path (0 .. K - 1), 0 without a path
 *   path_arcs_device,   int32, n rows of width P (>= 1), out_stride (>= P) elements apart: the arc indices in path order,
 *   path_tokens_device, their labels, the first frame of each and one past its last (blank frames belong to no arc); -1
 *   starts_device,      at and past path_len and in every entry of an utterance without a path.  A path longer than P
 *   ends_device         keeps its true path_len and writes its first P entries.  path_tokens + path_len have the layout
 *                       gtnx_batch_ctc_score, gtnx_batch_edit_distance and gtnx_batch_ctc_token_align take
 *   token_scores_device float32, same layout, or null: the sum of e(t, label) over the arc's frames, added in ascending
 *                       frame order from the first frame's value; -inf where starts is -1
 *   frame_arcs_device   int32, n rows of width M, frame_stride (>= M) apart, or null: the arc index of every frame, -1 on
 *                       blank frames, from T_b on and in every entry of an utterance without a path
 * Every element of every row is written over the widths P and M, nothing beyond them.  An utterance has no path exactly
 * where gtnx_batch_ctc_lattice_score gives -inf: T_b == 0, an invalid or too large lattice, a +inf or NaN weight, no
 * alignment fits or survives -inf emissions.  A one-node lattice has the empty path: a finite score (the blank
 * emissions summed), rows of -1.  Every arc field is checked before it becomes an address; nothing at or past
 * num_arcs[b], T_b or a width is read; the inputs are only read.  NaN emissions give unspecified values and no access
 * outside the utterance's own rows.
 * GTNX_INVALID_ARGUMENT before a device is asked for: what gtnx_batch_ctc_lattice_score refuses there, a null scores,
 * path_len, path_arcs, path_tokens, starts or ends pointer, P < 1, out_stride < P.  A batch without an utterance returns
 * without touching a device.  With the device: not a gtnx_batch_linear / _rows batch, a frame count outside 0 .. M,
 * blank >= C, frame_stride < M with frame arcs, an output the engine's current device may not write.  A refused call
 * writes nothing.
 * One workgroup per utterance (ctc_lattice_align.hip).  The back-pointers take 16 bits per state and frame in scratch
 * from the stream-ordered pool, 2 * max_states * max_b T_b bytes per utterance, at most 256 MiB per launch; beyond that
 * the utterances run in slices with the same bits (GTNX_CTC_LATTICE_ALIGN_SCRATCH_BYTES, read per call, lowers the cap: a
 * debug switch for tests); a single utterance above the cap runs alone.  Nothing is copied back, the call does not
 * wait. */
gtnx_status_t gtnx_batch_ctc_lattice_align(gtnx_batch_t ems, const int* frames, int blank, const void* arcs_device,
                                           int64_t row_stride, const void* num_arcs_device,
                                           const void* num_nodes_device, const void* arc_weights_device, int A,
                                           int max_states, void* scores_device, void* path_len_device,
                                           void* path_arcs_device, void* path_tokens_device, void* starts_device,
                                           void* ends_device, void* token_scores_device, int P, int64_t out_stride,
                                           void* frame_arcs_device, int64_t frame_stride);
/* calls that have launched so far (process-wide) / utterances they took */
gtnx_status_t gtnx_batch_ctc_lattice_align_stats(int64_t* calls, int64_t* utterances);
/* The best alignment of those hypotheses: WHEN each token was spoken and how well the frames support it, for all n * N
 * pairs in one call, results left on the device.  The inputs are those of gtnx_batch_ctc_score with the same meaning:
 * pair (b, k) is y = tokens[b][k][0 .. len), len = clamp(lengths[b][k], 0, L), under emissions_b[0 .. T_b).  The states
 * are those of ctcGraph(y, blank): s = 0 .. 2 len, even states carry `blank`, state 2 i + 1 carries y[i]; a frame enters
 * s from s and s - 1, and from s - 2 for an odd s > 1 whose token differs from the one before; paths start in state 0
 * before frame 0 and end in state 2 len or 2 len - 1 behind frame T_b - 1.  A token equal to `blank` is a label like
 * any other.  Float32 max-plus: a candidate is alpha[source] + e(t, label(s)), one addition; the new value is the exact
 * maximum.  Of the candidates that reach it the one whose source has the smallest rank wins, the rank order of the
 * states being, with U = len, S = 2 U + 1 and p leading strict ascents y[0] < .. < y[p],
 *   0 | (2i, 2i-1) for i = 1..p | S-1 | for i = U-1 down to p+1: (2i, 2i+1) if y[i] != y[i-1] else (2i+1, 2i) | 2p+1
 * and of two equal end states the smaller wins: the choice of viterbiPath (shortest.cpp:190-272) whenever every token
 * is above `blank`, and that of gtnx_batch_viterbi_align.  Every output is reproducible bit for bit.
 *   scores_device       float32 [n][N]: the path's score, -inf without a path
 *   starts_device,      int32, n * N rows of width L, out_stride (>= L) elements apart: the first frame of token i and
 *   ends_device         one past its last frame (blank frames belong to no token); -1 for i >= len and in every entry
 *                       of a pair without a path
 *   token_scores_device float32, same layout, or null: the sum of e(t, y[i]) over the token's frames, added in
 *                       ascending frame order from the first frame's value; -inf where starts is -1.  With normalised
 *                       emissions exp(token_scores / (ends - starts)) is the usual confidence; nothing is subtracted
 *   frame_tokens_device int32, n * N rows of width M, frame_stride (>= M) apart, or null: the token index of every
 *                       frame, -1 on blank frames, from T_b on and in every entry of a pair without a path
 * Every element of every row is written over the widths L and M, nothing beyond them.  A pair has no path where
 * gtnx_batch_ctc_score gives -inf: len + repeats > T_b, every path crosses a -inf emission, len > max_length, a token
 * inside the length outside 0 .. C - 1 (checked before it becomes an address), T_b == 0.  A beam slot without a
 * hypothesis (length 0) aligns as the empty sequence: a finite score, rows of -1.  Elements at or past a length and
 * emission rows at or past T_b are never read; the inputs are only read.  NaN emissions give unspecified values and no
 * access outside the pair's own rows.
 * GTNX_INVALID_ARGUMENT before a device is asked for: a null batch, tokens, lengths, scores, starts or ends pointer,
 * negative N, L, stride or blank, row_stride < L, out_stride < L, max_length outside 1 .. 4096.  n * N == 0 returns
 * without touching a device.  With the device: not a gtnx_batch_linear / _rows batch, a frame count outside 0 .. M,
 * blank >= C, frame_stride < M with frame tokens, an output the engine's current device may not write.  A refused call
 * writes nothing.
 * One workgroup per pair (ctc_token_align.hip).  The back-pointers take 2 bits per state and frame in scratch from the
 * stream-ordered pool, ceil(max_b T_b / 16) * (2 max_length + 1) words per pair, at most 256 MiB per launch; beyond
 * that the pairs run in slices with the same bits (GTNX_CTC_TOKEN_ALIGN_SCRATCH_BYTES, read per call, lowers the cap: a
 * debug switch for tests); a single pair above the cap runs alone.  Nothing is copied back, the call does not wait. */
gtnx_status_t gtnx_batch_ctc_token_align(gtnx_batch_t ems, const int* frames, int blank, const void* tokens_device,
                                         int64_t row_stride, const void* lengths_device, int N, int L, int max_length,
                                         void* scores_device, void* starts_device, void* ends_device,
                                         void* token_scores_device, int64_t out_stride, void* frame_tokens_device,
                                         int64_t frame_stride);
/* calls that have launched so far (process-wide) / pairs they aligned */
gtnx_status_t gtnx_batch_ctc_token_align_stats(int64_t* calls, int64_t* pairs);
/* The ASG force-align term of n * N device-resident hypotheses under the n emission slabs of a gtnx_batch_linear / _rows
 * batch, left on the device (DESIGN section 25 holds the contract):
 *   scores[b][k] = forwardScore(emissions_b[0 .. T_b) o (forceAlign(tokens[b][k][0 .. len)) o transitions)),
 * len = clamp(lengths[b][k], 0, L), log semiring, nothing subtracted -- so that the ASG loss of y is
 * forwardScore(emissions o transitions) minus this score.  tokens_device, row_stride, lengths_device, N, L, frames and
 * max_length are those of gtnx_batch_ctc_score; tokens are labels only (ASG has no blank) and equal neighbours are
 * legal, as in forceAlign.  table_device: float32 [C + C * C] in the arc order of asgTransitions -- entry y is
 * start[y], entry C + i * C + j is transitions[i][j], label j followed by label i -- the table
 * gtnx_batch_ctc_beam_decode_lm takes.  The positions are i = 0 .. len - 1, float32:
 *   alpha_0[0] = start[y_0] + e(0, y_0), every other alpha_0[i] = -inf;
 *   alpha_t[i] = logadd(alpha_{t-1}[i] + tr[y_i][y_i], alpha_{t-1}[i-1] + tr[y_i][y_{i-1}]) + e(t, y_i);
 *   score = alpha_{T_b - 1}[len - 1].
 * The score is -inf -- never NaN, and without a gradient -- when len == 0, T_b < len (T_b == 0 included), len >
 * max_length, a token inside the length lies outside 0 .. C - 1 (checked by the kernel before it becomes an address),
 * or every alignment crosses a -inf emission or table entry.  Elements at or past a length and emission rows at or
 * past T_b are never read.
 * GTNX_INVALID_ARGUMENT before a device is asked for: a null batch, table, tokens, lengths or scores pointer, negative
 * N, L or row_stride, row_stride < L, max_length outside 1 .. 4096.  n * N == 0 returns without touching a device.
 * With the device: not a gtnx_batch_linear / _rows batch, a frame count outside 0 .. M, more than 16384 labels (the
 * table gradient keeps a row of C floats in LDS), table_device anything but memory allocated on the engine's current
 * device (the kernel gathers from it: host memory is refused with one GPU as well), an output the engine's current
 * device may not write.
 * One launch on the engine's stream (asg_score.hip), one workgroup per pair, no scratch; nothing is copied back, the
 * call does not wait, nothing but scores is written. */
gtnx_status_t gtnx_batch_asg_score(gtnx_batch_t ems, const int* frames, const void* table_device,
                                   const void* tokens_device, int64_t row_stride, const void* lengths_device, int N,
                                   int L, int max_length, void* scores_device);
/* The gradients of those scores under caller-supplied weights_device (float32 [n][N], device memory), in one stateless
 * call.  The inputs are those of gtnx_batch_asg_score with the same refusals.
 *   grad_emissions_device (or null) float32 [n][M][C]: sum over k of weights[b][k] * d scores[b][k] / d emissions[b];
 *     EVERY element is written: zeros where nothing lands, rows at or past T_b included.
 *   grad_table_device (or null) float32 [C + C * C]: sum over all pairs of weights * d scores / d table in the table's
 *     own order; EVERY entry is written.
 * Not both null.  A pair whose score is -inf or whose weight is exactly 0 adds nothing.
 * The alpha rows are recomputed into scratch from the stream-ordered pool, max_b T_b * max_length floats per pair, at
 * most 256 MiB per slice of launches; beyond that the pairs run in slices, bit-equal to the unsliced run (the
 * environment variable GTNX_ASG_SCORE_SCRATCH_BYTES, read per call, lowers the cap: a debug switch for tests); a
 * single pair above the cap runs alone with scratch of its own size.  With a table gradient every pair also leaves 2 *
 * min(L, max_length) floats of occupancy sums in scratch, reduced by one launch behind the last slice: workgroup i
 * owns row i of the transitions, walks the pairs and positions in ascending order and adds one value at a time.  The
 * emission gradient is added by one workgroup per (utterance, tile of rows), which walks the utterance's pairs in k
 * order.  The sums are taken in one fixed order by plain loads and stores, so both gradients have the same bits run to
 * run; there are no floating-point atomics.  n * N == 0 returns without touching a device AND WITHOUT WRITING either gradient. */
gtnx_status_t gtnx_batch_asg_score_grad(gtnx_batch_t ems, const int* frames, const void* table_device,
                                        const void* tokens_device, int64_t row_stride, const void* lengths_device,
                                        int N, int L, int max_length, const void* weights_device,
                                        void* grad_emissions_device, void* grad_table_device);
/* calls of either kind that have launched so far (process-wide) / pairs they took */
gtnx_status_t gtnx_batch_asg_score_stats(int64_t* calls, int64_t* pairs);
/* The exact ASG log score of ONE ACYCLIC TOKEN LATTICE PER UTTERANCE -- gtnx_batch_ctc_lattice_score's lattices under
 * gtnx_batch_asg_score's criterion:
 *   scores[b] = log sum over the lattice's paths p of exp(w(p) + asg_score(emissions_b[0 .. T_b), table, labels(p))),
 * every decomposition and every alignment at once, nothing subtracted.  table_device: float32 [C + C * C], entry c =
 * start[c], entry C + i * C + j = transitions[i][j] (label j followed by label i).  The lattice arguments are those of
 * gtnx_batch_ctc_lattice_score with the same meaning: arcs (src, dst, label) with 0 <= src < dst < num_nodes, dst-sorted,
 * node 0 starts, the last node accepts, arc_weights added once per use of the arc, -inf forbids it.  The states are the
 * arcs: one token state per arc, NO blank states, equal neighbouring labels are legal.  Float32, in this order:
 *   frame 0: alpha[a] = (w_a + table[lab a]) + e(0, lab a) for src a == 0, -inf otherwise
 *   frame t: x = alpha[a] + table[C + lab a * C + lab a]; for a' entering src a, ascending:
 *            x = logadd(x, alpha[a'] + (w_a + table[C + lab a * C + lab a'])); alpha'[a] = x + e(t, lab a)
 *   score = logadd over the arcs entering the last node, ascending.
 * max_states (1 .. 4096) is the caller's bound on nodes + arcs, exactly as for the CTC call, so the same lattices and
 * the same argument serve both criteria.  max_edges (1 .. 2^21) is the caller's bound on E_b = the sum over the arcs of
 * the in-degree of their src; the kernel counts E_b when it stages the lattice (the gradient call sizes its scratch by
 * the bound without a download).  The score is -inf -- never NaN, and without a gradient -- when T_b == 0, num_nodes <
 * 1, nodes + clamp(num_arcs) > max_states, E_b > max_edges, any arc field gtnx_batch_ctc_lattice_score refuses, a weight
 * that is +inf or NaN, no alignment fits (a one-node lattice has none: ASG has no empty alignment), or every alignment
 * passes a -inf emission, start or transition entry.  Every arc field is checked before it becomes an address or an
 * index; nothing at or past num_arcs[b] is read.  At most 16384 labels; table indices are computed in 64 bits.
 * GTNX_INVALID_ARGUMENT before a device is asked for: a null batch, table, arcs, num_arcs, num_nodes or scores pointer,
 * negative A, row_stride < 3 A, max_states outside 1 .. 4096, max_edges outside 1 .. 2^21.  A batch without an utterance
 * returns without touching a device.  With the device: not a gtnx_batch_linear / _rows batch, a frame count outside
 * 0 .. M, more than 16384 labels, a table that is not device memory, an output the current device may not write.
 * One launch on the engine's stream (asg_lattice.hip), one workgroup per utterance, no scratch, no copy back, no wait. */
gtnx_status_t gtnx_batch_asg_lattice_score(gtnx_batch_t ems, const int* frames, const void* table_device,
                                           const void* arcs_device, int64_t row_stride, const void* num_arcs_device,
                                           const void* num_nodes_device, const void* arc_weights_device, int A,
                                           int max_states, int max_edges, void* scores_device);
/* The gradients of those scores for caller-supplied weights_device (float32 [n]; grad_out under autograd).  Each output
 * may be null, not all three.  grad_emissions_device: float32 [n][M][C] = weights[b] * d scores[b] / d emissions[b];
 * grad_table_device: float32 [C + C * C] = sum over b of weights[b] * d scores[b] / d table; arc_grad_device: float32
 * [n][A] = weights[b] * the posterior probability that the arc is used.  EVERY element of an output is written: zeros
 * where nothing lands, rows at or past T_b and arcs at or past num_arcs[b] included.  An utterance whose score is -inf
 * or whose weight is exactly 0 adds nothing.  Stateless: alpha is recomputed into scratch from the stream-ordered pool
 * (max_b T_b * max_states floats per utterance; with a table or arc gradient max_edges floats per utterance on top, one
 * cell per edge), at most 256 MiB per launch group; beyond that the utterances run in slices, bit-equal to the unsliced
 * run (GTNX_ASG_LATTICE_SCRATCH_BYTES, read per call, lowers the cap: a debug switch for tests).  Every sum has one
 * order -- a label's arcs ascending, an arc's frames descending, an edge's frames descending in its own cell, a table
 * row's utterances, arcs and edges ascending, one value at a time -- and every store is a plain store: the same bits run
 * to run; there are no floating-point atomics. */
gtnx_status_t gtnx_batch_asg_lattice_score_grad(gtnx_batch_t ems, const int* frames, const void* table_device,
                                                const void* arcs_device, int64_t row_stride,
                                                const void* num_arcs_device, const void* num_nodes_device,
                                                const void* arc_weights_device, int A, int max_states, int max_edges,
                                                const void* weights_device, void* grad_emissions_device,
                                                void* grad_table_device, void* arc_grad_device);
/* calls of either kind that have launched so far (process-wide) / utterances they took */
gtnx_status_t gtnx_batch_asg_lattice_score_stats(int64_t* calls, int64_t* utterances);
/* The best ASG alignment of those hypotheses: WHEN each token was spoken and how well the frames support it, for all
 * n * N pairs in one call, results left on the device (DESIGN section 28 holds the contract).  The inputs are those of
 * gtnx_batch_asg_score with the same meaning: pair (b, k) is y = tokens[b][k][0 .. len), len = clamp(lengths[b][k], 0,
 * L), under emissions_b[0 .. T_b); table_device is float32 [C + C * C], entry y is start[y], entry C + i * C + j is
 * transitions[i][j], label j followed by label i; its indices are computed in 64 bits and the call has no cap on C of
 * its own.  Position i = 0 .. len - 1 means the first i + 1 labels are consumed; a frame enters i from i (self) and
 * from i - 1 (step); paths start in position 0 at frame 0 and end in position len - 1 behind frame T_b - 1.  Equal
 * neighbouring tokens are legal, there is no blank.  Float32 max-plus with the association of
 * gtnx_batch_viterbi_align's ASG launch, so that the scores are bit-equal to it where both apply: with w_self[i] =
 * tr[y_i][y_i], w_step[i] = tr[y_i][y_{i-1}] and w_step[0] = start[y_0],
 *   alpha_0[0] = 0.0f + (w_step[0] + e(0, y_0)), every other alpha_0[i] = -inf;
 *   c0 = alpha_{t-1}[i] + (w_self[i] + e(t, y_i)), c1 = alpha_{t-1}[i-1] + (w_step[i] + e(t, y_i));
 *   alpha_t[i] = max(c0, c1), exact; of two equal candidates THE STEP WINS (c1 >= c0), the choice of viterbiPath on
 *   this lattice.  Every output is reproducible bit for bit.
 *   scores_device       float32 [n][N]: alpha_{T_b - 1}[len - 1], -inf without a path
 *   starts_device,      int32, n * N rows of width L, out_stride (>= L) elements apart: the first frame of token i and
 *   ends_device         one past its last frame; with a path starts[0] == 0, ends[i] == starts[i + 1], ends[len - 1] ==
 *                       T_b; -1 for i >= len and in every entry of a pair without a path
 *   token_scores_device float32, same layout, or null: the sum of e(t, y[i]) over the token's frames, added in
 *                       ascending frame order from the first frame's value, emissions only; -inf where starts is -1
 *   frame_tokens_device int32, n * N rows of width M, frame_stride (>= M) apart, or null: the token index of every
 *                       frame, never -1 inside a path; -1 from T_b on and in every entry of a pair without a path
 * Every element of every row is written over the widths L and M, nothing beyond them.  A pair has no path exactly where
 * gtnx_batch_asg_score gives -inf: len == 0 (a beam slot without a hypothesis: rows of -1 and -inf), T_b < len, len >
 * max_length, a token inside the length outside 0 .. C - 1 (checked before it becomes an address), a -inf emission or
 * table entry on every alignment.  Elements at or past a length and emission rows at or past T_b are never read; the
 * inputs are only read.  NaN or +inf inputs give unspecified values and no access outside the pair's own rows.
 * GTNX_INVALID_ARGUMENT before a device is asked for: a null table, scores, starts or ends pointer, a negative
 * out_stride or frame_stride, out_stride < L, then what gtnx_batch_asg_score refuses about the batch, tokens, lengths,
 * N, L, row_stride and max_length (1 .. 4096).  n * N == 0 returns without touching a device.  With the device: not a
 * gtnx_batch_linear / _rows batch, a frame count outside 0 .. M, frame_stride < M with frame tokens, table_device
 * anything but memory allocated on the engine's current device, an output the engine's current device may not write.
 * A refused call writes nothing.
 * One workgroup per pair (asg_token_align.hip).  The back-pointers take 1 bit per position and frame in scratch from
 * the stream-ordered pool, ceil(max_b T_b / 32) * max_length words per pair, at most 256 MiB per launch; beyond that
 * the pairs run in slices with the same bits (GTNX_ASG_TOKEN_ALIGN_SCRATCH_BYTES, read per call, lowers the cap: a
 * debug switch for tests); a single pair above the cap runs alone.  Nothing is copied back, the call does not wait. */
gtnx_status_t gtnx_batch_asg_token_align(gtnx_batch_t ems, const int* frames, const void* table_device,
                                         const void* tokens_device, int64_t row_stride, const void* lengths_device,
                                         int N, int L, int max_length, void* scores_device, void* starts_device,
                                         void* ends_device, void* token_scores_device, int64_t out_stride,
                                         void* frame_tokens_device, int64_t frame_stride);
/* calls that have launched so far (process-wide) / pairs they aligned */
gtnx_status_t gtnx_batch_asg_token_align_stats(int64_t* calls, int64_t* pairs);
/* ASG prefix beam search with N-best output over the n emission slabs of a gtnx_batch_linear / _rows batch
 * ([n][M][C]), results left on the device.  The hypotheses are the label sequences WITHOUT EQUAL
 * NEIGHBOURS -- what gtnx_batch_viterbi_decode's collapsed rows can hold -- each summed over all of its alignments
 * under emissions o transitions.  Every frame labelling collapses to exactly one such sequence, so the hypotheses
 * partition the paths: unpruned, a hypothesis's score is gtnx_batch_asg_score of its tokens, and the log-sum over all
 * hypotheses is forwardScore(emissions o transitions).
 * table_device: DEVICE float32 [C + C * C] in the arc order of gtn::criteria::asgTransitions: table[c] is start[c],
 * table[C + i * C + j] is transitions[i][j], the score of label j followed by label i -- the table
 * gtnx_batch_asg_score takes.  frames: HOST, [n], T_b in 0 .. M, or null (the rows the batch carries).
 * Per utterance, float32 throughout, with x = emissions[b][t]:
 *   token set   S_t = the cutoff_top_n (1 .. 32) best labels of row t: value descending, of equal values the smaller
 *               label; NaN and -inf are never chosen; no blank is appended.  S_t restricts EVERY use of frame t, stays
 *               as well as extensions: with an unbounded list the result is the exact N-best of the lattice restricted
 *               to S_t per frame.
 *   state       at most beam_size (1 .. 64) distinct prefixes, each with ONE score a(p): the log-sum of the alignments
 *               of frames 0 .. t to p that end in last(p).  Before frame 0: the empty prefix with score 0.  It has no
 *               stay, so it is gone after frame 0.
 *   frame t     with l = last(p): the stay (p not empty, l in S_t) scores (a(p) + tr[l][l]) + x[l]; the extension by c
 *               in S_t, c != l, scores s = (a(p) + w) + x[c], w = start[c] for the empty prefix and tr[c][l] otherwise.
 *               A w that is -inf, +inf or NaN drops its candidate, so a -inf entry forbids a bigram or a first label;
 *               a candidate whose value is not above -inf is dropped.  An extension that spells a prefix q of the list
 *               is no candidate: its s is log-added into q's stay value (from -inf if q has no stay), and the merged q
 *               competes as a stay.  Identity is exact, by the labels: a prefix that left the list and was created
 *               again is still recognised as the parent of its child that stayed.
 *   order       total descending, then stays before extensions, then the parent's rank ascending, then the label
 *               ascending; the first beam_size with a total above -inf form the new list.
 *   arithmetic  the sums in exactly the order written; log-add(a, b) = b if a = -inf, a if b = -inf, else m +
 *               log1p(exp(n - m)), m the larger, n the smaller.
 * tokens_device: int32 [n][nbest] rows of width M, row_stride (>= M) elements apart: the labels of hypothesis r of
 * utterance b, -1 from its length on up to column M; lengths_device: int32 [n][nbest]; scores_device: float32
 * [n][nbest].  A slot without a hypothesis (T_b == 0, a frame with nothing above -inf, fewer hypotheses than nbest) gets
 * -1, 0, -inf.  Rows at or past T_b are never read: what they hold never changes a bit of any output.  No global or
 * floating-point atomics: the same bits run to run.
 * GTNX_INVALID_ARGUMENT, each with a text that begins "[gtnx_batch_asg_beam_decode]", and nothing is written.  Before a
 * device is asked for: a null batch, a null table, a null output pointer, a negative row_stride, beam_size outside
 * 1 .. 64, cutoff_top_n outside 1 .. 32, nbest outside 1 .. beam_size.  n == 0 then returns without touching a device.
 * With the device: not a gtnx_batch_linear / _rows batch (there is no other route), a frame count outside 0 .. M or
 * above the rows the batch carries, row_stride < M, M * beam_size beyond an int, more than 2^19 labels (a candidate's
 * sort key keeps its label in 19 bits; such a table has no device to live on), table_device anything but memory
 * allocated on the engine's current device (the kernel gathers from it: host memory is refused with one GPU as well),
 * an output the engine's current device may not write.
 * Two launches on the engine's stream (asg_beam.hip): the token sets of all rows, then one workgroup per utterance.
 * Scratch from the stream-ordered pool: 8 * cutoff_top_n + 4 bytes per row and 8 * (M * beam_size + 1) bytes per
 * utterance.  Nothing is copied back, the call does not wait. */
gtnx_status_t gtnx_batch_asg_beam_decode(gtnx_batch_t ems, const int* frames, const void* table_device, int beam_size,
                                         int cutoff_top_n, int nbest, void* tokens_device, int64_t row_stride,
                                         void* lengths_device, void* scores_device);
/* gtnx_batch_asg_beam_decode with a compiled LM graph (gtnx_lm_graph_create; its walk semantics are stated there) fused
 * into the ranking -- a lexicon, a grammar or an n-gram model beside the criterion's own transitions, which stay what
 * they are: table_device is still the acoustic model's table.  DESIGN section 31 holds the contract:
 *   state       every prefix also carries L (float32) and its LM state; the empty prefix has L = 0 and the graph's start
 *               state.
 *   extension   of prefix p by c in S_t, c != last(p): (wt, next) = the walk of (state(p), c);
 *               inc = lm_weight * wt + insertion_bonus (the product rounded, then the sum; never fused).  The acoustic
 *               score is unchanged, s = (a(p) + w) + x[c]; L' = L(p) + inc, state' = next, total = s + L'.  Dropped
 *               when the walk forbids c or inc is not finite, and for every reason it is dropped without a graph.
 *   stay        unchanged, the graph is not consulted: total = stay + L(p); L and the state are copied.
 *   merging     acoustic and unchanged: an extension that spells a prefix q of the list is log-added into q's stay and
 *               struck.  The graph is deterministic, so q has that extension's L and state already.
 *   order       by total descending, then as without a graph.  The token sets and their pruning stay acoustic.  A total
 *               is not examined beyond that: a candidate is dropped by its acoustic score and its inc alone.
 * Labels of the graph at or above C are never walked, accept flags are ignored, and (state, c) with c == last(p) is
 * never walked: a sequence with equal neighbours is no hypothesis.
 * scores_device: acoustic + L (one float32 add); am_scores_device (float32 [n][nbest], may be null): the acoustic
 * score alone -- unpruned, gtnx_batch_asg_score of those tokens.  A slot without a hypothesis gets -1, 0, -inf, -inf.
 * With lm_weight = 0, insertion_bonus = 0 and a graph that permits every label with a finite weight, tokens, lengths
 * and scores are the bytes of gtnx_batch_asg_beam_decode, and am_scores equals scores.
 * GTNX_INVALID_ARGUMENT, each with a text that begins "[gtnx_batch_asg_beam_decode_graph]", and nothing is written:
 * everything gtnx_batch_asg_beam_decode refuses, and before a device is asked for: a null, destroyed or foreign
 * lm_graph, an lm_weight or insertion_bonus that is not finite; with the device: an am_scores_device that is not
 * memory allocated on the engine's current device (host memory is refused with one GPU as well), a graph that was
 * uploaded to another device.  The first decode with a graph uploads it (16 bytes per arc, 32 per state) and waits for
 * that copy, once.  Counted by gtnx_batch_asg_beam_stats. */
gtnx_status_t gtnx_batch_asg_beam_decode_graph(gtnx_batch_t ems, const int* frames, const void* table_device,
                                               int beam_size, int cutoff_top_n, int nbest, gtnx_lm_graph_t lm_graph,
                                               float lm_weight, float insertion_bonus, void* tokens_device,
                                               int64_t row_stride, void* lengths_device, void* scores_device,
                                               void* am_scores_device /* may be null */);
/* calls that have launched so far (process-wide) / utterances they decoded */
gtnx_status_t gtnx_batch_asg_beam_stats(int64_t* calls, int64_t* utterances);
/* num_samples alignments of every chain of a batch drawn from the posterior of the ASG model emissions o transitions,
 * plus the merge of equal neighbours, results left on the device (DESIGN section 34 has the whole contract).  ASG frames
 * are not independent: the sample is exact by forward filtering, backward sampling.
 *   Model: table_device is float32 [C + C * C] on the device in the arc order of asgTransitions -- table[c] the start
 *   score of label c, table[C + i * C + j] the score of moving from label j to label i -- the table of
 *   gtnx_batch_asg_score.  s(y) = table[y0] + x[b,0,y0] + sum_{t>=1} (table[C + y_t * C + y_{t-1}] + x[b,t,y_t]), and
 *   alignment y of utterance b is drawn with probability exp(s(y) / temperature - logZ_b).
 *   Mass: only finite entries carry mass.  A -inf, +inf or NaN emission or table entry makes every alignment through it
 *   impossible, and it is never drawn.  An utterance without an alignment of finite score, or with T_b == 0, has no
 *   path: every sample of it gets -1 rows, length 0, logq = -inf, and its logz is -inf.  No output is ever NaN.
 *   Filter: alpha_0[i] = (table[i] + x[0,i]) / temperature, alpha_t[i] = x[t,i] / temperature + logsumexp_j(table[C +
 *   i * C + j] / temperature + alpha_{t-1}[j]), kept per frame as a float32 plane relative to a float64 running
 *   reference; logZ_b = logsumexp_i alpha_{T_b-1}[i].
 *   Draw: backward, one uniform per (b, k, t).  Frame T_b - 1 has masses exp(alpha[j] - ref), frame t below it, given
 *   i = y_{t+1}, masses exp(alpha_t[j] + table[C + i * C + j] / temperature - ref).  Inverse CDF in label order: the
 *   smallest j whose cumulative mass over 0 .. j exceeds u * total (the total as the sampler summed it); if rounding
 *   leaves none, the last label with mass.  A label without mass is never returned.
 *   Randomness is counter-based: Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (t, b, k >> 2, 1)
 *   (gtnx_batch_ctc_sample has 0 in the last word); sample k uses output word k & 3, u = (2 * (word >> 9) + 1) * 2^-24.
 *   The same seed gives the same bytes whatever the strides, the slicing, the frame counts of the other utterances or
 *   the contents of pad rows, and the first N samples of a call with more are those of a call with N.
 * tokens_device: int32 [n][num_samples][row_stride], row_stride >= M: the alignment with equal neighbours merged (ASG
 * has no blank), -1 from its length to M -- the layout gtnx_batch_asg_beam_decode writes; lengths_device: int32
 * [n][num_samples]; logq_device (may be null): float32 [n][num_samples], the sum of the drawn conditionals' logs
 * log(mass / total), added in draw order (frame T_b - 1 first) from 0 in float32 -- in exact arithmetic s(y) /
 * temperature - logZ_b; labels_device (may be null): int32 [n][num_samples][row_stride], the frame labels, -1 from T_b
 * to M; logz_device (may be null): float32 [n], logZ_b -- at temperature 1 the full-connect score
 * forwardScore(emissions_b[:T_b] o transitions).
 * frames (host, [n], or null): T_b; null means the rows the batch carries.  Rows from T_b on are never read.
 * GTNX_INVALID_ARGUMENT before a device is asked for: a null batch, table, tokens or lengths pointer, a negative
 * stride, num_samples outside 1 .. 1024, a temperature that is not finite and > 0, a number of labels outside 1 .. 1024
 * (the filter is O(T C^2) per utterance and the draw keeps a row in the registers of one wave).  With the device: ems
 * is not a gtnx_batch_linear / _rows batch (there is no other route), a count outside 0 .. M or above the rows the batch
 * carries, row_stride < M, n * num_samples beyond an int, a table or outputs that are not memory of the engine's current
 * device.  A refused call writes nothing.
 * Launches on the engine's stream (asg_sample.hip): filter, draw and collapse per slice, one prep launch before them
 * above 128 labels.  The planes (4 M C bytes per utterance) and the label and term of every (b, k, t) live in scratch
 * from the stream-ordered pool, at most 256 MiB per slice: beyond that the utterances run in slices with the same bytes
 * (GTNX_ASG_SAMPLE_SCRATCH_BYTES, read per call, lowers the cap: a debug switch for tests).  Nothing is copied back and
 * the call does not wait for the device. */
gtnx_status_t gtnx_batch_asg_sample(gtnx_batch_t ems, const int* frames, const void* table_device, int num_samples,
                                    uint64_t seed, float temperature, void* tokens_device, int64_t row_stride,
                                    void* lengths_device, void* logq_device /* may be null */,
                                    void* labels_device /* may be null */, void* logz_device /* may be null */);
/* calls that have launched so far (process-wide) / utterances they sampled */
gtnx_status_t gtnx_batch_asg_sample_stats(int64_t* calls, int64_t* utterances);
/* rows M and labels C of the slabs of a gtnx_batch_linear / _rows batch; -1, -1 for any other batch */
gtnx_status_t gtnx_batch_linear_shape(gtnx_batch_t ems, int* rows, int* labels);
gtnx_status_t gtnx_batch_backward(gtnx_batch_t a, int retain_graph);                  /* autograd.cpp:17-67 */
gtnx_status_t gtnx_batch_items(gtnx_batch_t a, float* out);                           /* graph.h:143, n floats */
gtnx_status_t gtnx_batch_items_device(gtnx_batch_t a, void* device_out);
/* as gtnx_grads_bind_device_n / gtnx_grads_device_n, for the elements of a batch */
gtnx_status_t gtnx_batch_grads_bind_device(gtnx_batch_t a, void* device_out, const int64_t* offsets);
gtnx_status_t gtnx_batch_grads_device(gtnx_batch_t a, void* device_out, const int64_t* offsets);

/* ------------------------------------------------------------------ autograd
 * gtn/autograd.h:27,37 */
gtnx_status_t gtnx_backward(gtnx_graph_t g, int retain_graph);
gtnx_status_t gtnx_backward_with_grad(gtnx_graph_t g, gtnx_graph_t grad, int retain_graph);
gtnx_status_t gtnx_backward_n(const gtnx_graph_t* g, int n, int retain_graph);

/* ------------------------------------------------------------------ utils
 * gtn/utils.h:23-60 (test fixtures of the parity suite; host-side) */
gtnx_status_t gtnx_equal(gtnx_graph_t a, gtnx_graph_t b, int* out);
gtnx_status_t gtnx_isomorphic(gtnx_graph_t a, gtnx_graph_t b, int* out);

/* ------------------------------------------------------------------ formats
 * gtn/utils.h:115-150, utils.cpp:152-225: the binary graph format -- int32 {numNodes, numArcs, numStart, numAccept},
 * the start nodes, the accept nodes, {src, dst, ilabel, olabel} per arc, float32 weights.  `data` is the whole
 * file image: the arc table and the weights go to the device in ONE copy and are split into the graph's SoA
 * arrays there (adjacency lists built on the device as well); node and arc ids as load() numbers them. */
gtnx_status_t gtnx_graph_load_buffer(const void* data, size_t bytes, gtnx_graph_t* out);

/* ------------------------------------------------------------------ several GPUs, one process
 * The path shards by utterance (parallelMap has no cross-task communication, parallel/parallel_map.h:167-179): a host
 * that drives the GPUs of a node gives each device its own thread (gtnx_set_device; gtn::parallelMapSharded) and no
 * data-path collective is needed.  What is gathered afterwards goes over RCCL (xGMI), one communicator per device,
 * enqueued on each device's engine stream so that it orders with the kernels producing its inputs:
 *   all_gather   the per-utterance losses: device k contributes `count` floats at send[k] (ITS memory) and receives
 *                all n * count at recv[k], blocks in the order of `devices`
 *   all_reduce   the gradient of a graph every utterance shares (ASG transitions, criterion_test.cpp:289-305: the sum
 *                over utterances): bufs[k] (device k's partial sum, `count` floats) becomes the total, in place
 * librccl.so is looked up at first use; a communicator over ONE device needs none (gather = copy, reduce = nothing). */
typedef struct gtnx_comm_s* gtnx_comm_t;
gtnx_status_t gtnx_comm_create(const int* devices, int n, gtnx_comm_t* out);
gtnx_status_t gtnx_comm_destroy(gtnx_comm_t c);
gtnx_status_t gtnx_comm_size(gtnx_comm_t c, int* n);
gtnx_status_t gtnx_comm_all_gather_f32(gtnx_comm_t c, const void* const* send, void* const* recv, int64_t count);
gtnx_status_t gtnx_comm_all_reduce_sum_f32(gtnx_comm_t c, void* const* bufs, int64_t count);

/* ------------------------------------------------------------------ profiling
 * hipEvent timing of the engine's own kernel launches on the launch stream
 * (what bench.py's roofline leg reads).  name is a kernel family, e.g.
 * "forward_score", "compose", "forward_score_grad", "linear_forward". */
gtnx_status_t gtnx_prof_enable(int on);
gtnx_status_t gtnx_prof_reset(void);
gtnx_status_t gtnx_prof_get(const char* name, double* total_ms, int64_t* launches,
                            double* algorithmic_bytes);
/* Diagnostics: viterbiPath of SYMBOLIC products with a dense partner (max-plus walk) -- how many best paths ran through
 * a state with two exactly equal finite candidates since the process started (`seen`), and how many of those kept the
 * first maximum in in-row order because the product was too large to build and replay the reference's queue on
 * (`unresolved`; shortest.cpp:215-218, INTEGRATION.md "Where results can differ" 3). */
gtnx_status_t gtnx_debug_viterbi_ties(int64_t* seen, int64_t* unresolved);
/* Diagnostics (host only, no GPU needed): how exact ties in products of an emission chain with `g` are decided without
 * building the lattice when g is exactly a CTC target acceptor (benchmarks/ctc.cpp:40-58) with label-sorted out-lists:
 * queue_rank[n] = position of node n in the reference's queue within every layer of the lattice (viterbiPath keeps the
 * arc relaxed first, shortest.cpp:208-224), creation_rank[n] = its position in compose's creation order (in-list and
 * accept-list order: viterbiScore's gradient, shortest.cpp:118-127, :148-160); numNodes() ints each.  *applies = 0:
 * g is not such a graph (nothing written; tied utterances then take the built lattice). */
gtnx_status_t gtnx_debug_tie_ranks(gtnx_graph_t g, int* queue_rank, int* creation_rank, int* applies);
/* names, '\n'-separated, of the families seen since the last reset */
gtnx_status_t gtnx_prof_names(char* buf, size_t cap);
/* Diagnostics: which kernel family would score the SYMBOLIC chain product `g` (a compose / intersect result kept
 * symbolic, gtnx_compose_mode) -- forwardScore (tropical = 0) or viterbiScore / viterbiPath (tropical = 1).  The
 * decision table is gtn_amd/csrc/ops_symbolic.cpp; *route is an index into "band", "pair", "dense_mfma", "dense",
 * "maxplus", "walk" (gtnx_debug_route_name), or -1 when `g` is not a symbolic product.  No reference analogue. */
gtnx_status_t gtnx_debug_symbolic_route(gtnx_graph_t g, int tropical, int* route);
gtnx_status_t gtnx_debug_route_name(int route, char* buf, size_t cap);
/* Diagnostics (host only, no GPU needed): which kernel of gtn_amd/csrc/shortest.hip the forwardScore / viterbiScore /
 * viterbiPath sweeps of BUILT graphs and their gradients were given to.  Cell `cell` of *n_cells: its name
 * ("fwd/generic/log/g8", "fwd/narrow/log/inw", "fwd/deep", "bwd/generic/tropical/g64", "bwd/narrow/fused", ...:
 * direction / family / semiring or mode / lanes per node) into buf, and the number of launches it took since the
 * process started into *launches.  A cell outside [0, *n_cells) gives an empty name and 0.  Any pointer may be NULL.
 * No reference analogue. */
gtnx_status_t gtnx_debug_shortest_routes(int cell, char* buf, size_t cap, int64_t* launches, int* n_cells);
/* Diagnostics (host only, no GPU needed): the way compose / intersect took (gtn_amd/csrc/ops_compose.cpp), counted per
 * PRODUCT -- not per launch -- since the process started.  Cell `cell` of *n_cells: its name into buf and its count into
 * *count.  The cells: the kernel of a product's first run ("fast256", "fast512", "general/lds", "general/hbm",
 * "wide_chain", "pairs"); the hand-backs a kernel asked for ("redo/fast->wide_chain", "redo/fast->pairs",
 * "redo/fast->general", "redo/wide_chain->general"); the bitmap layout of a chain product whose first run was the FAST
 * variant ("bitmap/classic", "bitmap/window_full", "bitmap/window_partial"); and attributes of the finished product:
 * "sizes/deferred" | "sizes/read", "arrays/skipped" | "arrays/full", "layered" | "not_layered", "transpose" (it needed
 * the transpose passes), for products the FAST variant finished "g1_cache/on" | "g1_cache/off" and, chain products
 * only, "replicate/inline" | "replicate/grid"; "symbolic": the product stayed lazy and nothing was built.  A call that
 * throws counts nothing.  A cell outside [0, *n_cells) gives an empty name and 0.  Any pointer may be NULL.  No
 * reference analogue. */
gtnx_status_t gtnx_debug_compose_routes(int cell, char* buf, size_t cap, int64_t* count, int* n_cells);

#ifdef __cplusplus
}
#endif
#endif /* GTN_AMD_H */
