// lm_graph.h -- a deterministic acceptor with back-off (failure) arcs, compiled for the two prefix beam searches
// (DESIGN section 30 holds the contract, section 31 the ASG search's; lm_walk.h walks the same words on the device, for
// ctc_beam.hip and asg_beam.hip alike).
//
// The compiled form is ONE array of 16-byte words, so that every probe of a walk is the same load:
//   state s, words [2 s] and [2 s + 1]:  { begin, count, eps_dst, eps_weight bits }  { first label, dense, 0, 0 }
//            begin:   the word index of the state's first labelled arc (arcs of a state are contiguous, sorted by label)
//            count:   how many labelled arcs it has
//            eps_dst: where its epsilon arc leads, -1 without one; eps_weight: that arc's weight
//            dense:   1 when the labels are first, first + 1, ..., first + count - 1 -- the arc of label c is then word
//                     begin + (c - first), found with one load
//   arc,     word [2 S + j]:             { label, dst, weight bits, 0 }
// A lookup loads the state's two words together, then bisects the arcs (one word per probe; the probe that finds the
// label has the destination and the weight with it).
//
// Walk semantics (failure arcs, what ARPA back-off means -- NOT what compose does with epsilon): from state s with label
// c, an arc labelled c adds its weight and leads to its destination; otherwise the epsilon arc adds its weight and the
// walk repeats from its destination; without either c is forbidden from s.  The weight is the float32 sum of the walked
// weights in walk order, starting from the first one.
//
// A snapshot: the arcs and the weights as they are when it is compiled.  No autograd.  Accept flags and output labels
// are ignored.  Compiling and walking are host work and need no device; the words are uploaded by the first decode.
#pragma once
#include <memory>
#include <mutex>
#include <vector>

#include "graph.h"
#include "kernels.h"

namespace gtnx {

constexpr int kLmMaxEpsChain = 8;        // epsilon arcs a walk may follow; it visits at most one state more
constexpr int kLmMaxBisect = 32;         // probes of one state's arcs
constexpr int64_t kLmMaxNodes = 1 << 24;

struct LmGraph {
  std::vector<gtnx_i4> words;
  int states = 0, start = 0, eps_chain = 0;
  int64_t arcs = 0;  // of the source graph, epsilon arcs included
  // the device copy: made once, by the first decode that uses it, on that decode's device
  std::mutex mu;
  DevMemP dev;
  int device = -1;
};
using LmGraphP = std::shared_ptr<LmGraph>;

// Refuses (GTNX_INVALID_ARGUMENT, nothing repaired): no start node or several, two arcs with one input label out of a
// node, several epsilon arcs out of a node, an epsilon chain that is cyclic or longer than 8 arcs, a label below -1,
// more than 2^24 nodes, a linear graph.  The arcs need not be sorted.
LmGraphP lm_graph_compile(Graph& g);
// false: `label` is forbidden from `state` (weight and next are then -inf and -1).  A found walk may still have a
// weight that is not finite: the search drops such an extension.
bool lm_graph_walk(const LmGraph& lm, int state, int label, float* weight, int* next);
// the words on the calling thread's device (uploaded on first use; a graph that lives on another device is refused,
// under the name `who` of the entry that asked)
const gtnx_i4* lm_graph_device(LmGraph& lm, const char* who);

// handles of the C ABI: a registry, so that a destroyed or foreign pointer is refused and not followed
void* lm_graph_register(LmGraphP lm);
LmGraphP lm_graph_lookup(const void* handle);  // null when the handle is not a live one
bool lm_graph_unregister(const void* handle);

}  // namespace gtnx
