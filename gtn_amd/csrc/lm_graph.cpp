// lm_graph.cpp -- compile, walk and upload of the LM graph of the CTC prefix beam search (lm_graph.h has the layout and
// the semantics).  Host code throughout: nothing here asks for a device but lm_graph_device.
#include "lm_graph.h"

#include <algorithm>
#include <cstring>
#include <limits>
#include <numeric>
#include <string>
#include <unordered_map>

namespace gtnx {

namespace {
constexpr const char* kWho = "[gtnx_lm_graph_create] ";

inline int f2i(float f) {
  int i;
  std::memcpy(&i, &f, sizeof(i));
  return i;
}
inline float i2f(int i) {
  float f;
  std::memcpy(&f, &i, sizeof(f));
  return f;
}
inline gtnx_i4 word(int x, int y, int z, int w) {
  gtnx_i4 v;
  v.x = x;
  v.y = y;
  v.z = z;
  v.w = w;
  return v;
}

std::mutex g_reg_mu;
std::unordered_map<const void*, LmGraphP> g_reg;
}  // namespace

LmGraphP lm_graph_compile(Graph& g) {
  Structure& s = *g.s;
  if (s.kind == KIND_LINEAR) throw_invalid(std::string(kWho) + "a linear graph is not a language model: build an explicit acceptor");
  s.ensure_host();
  const int64_t N = s.N, A = s.A;
  if (s.start.size() != 1)
    throw_invalid(std::string(kWho) + (s.start.empty() ? "the graph has no start node" : "the graph has more than one start node"));
  if (N > kLmMaxNodes) throw_invalid(std::string(kWho) + "more than 2^24 nodes");
  if (2 * N + A + 1 > std::numeric_limits<int>::max()) throw_invalid(std::string(kWho) + "too many arcs: the compiled form is indexed by an int");
  const float* wt = A > 0 ? g.weights_host(false) : nullptr;
  for (int64_t a = 0; a < A; ++a)
    if (s.il[size_t(a)] < -1) throw_invalid(std::string(kWho) + "an input label below -1 (arc " + std::to_string(a) + ")");
  // the arcs by (source, input label): the epsilon arc of a node (-1) comes first
  std::vector<int> order(static_cast<size_t>(A));
  std::iota(order.begin(), order.end(), 0);
  std::sort(order.begin(), order.end(), [&](int x, int y) {
    if (s.src[size_t(x)] != s.src[size_t(y)]) return s.src[size_t(x)] < s.src[size_t(y)];
    if (s.il[size_t(x)] != s.il[size_t(y)]) return s.il[size_t(x)] < s.il[size_t(y)];
    return x < y;
  });
  for (int64_t k = 1; k < A; ++k) {
    const int x = order[size_t(k - 1)], y = order[size_t(k)];
    if (s.src[size_t(x)] == s.src[size_t(y)] && s.il[size_t(x)] == s.il[size_t(y)]) {
      if (s.il[size_t(x)] == -1)
        throw_invalid(std::string(kWho) + "more than one epsilon arc out of node " + std::to_string(s.src[size_t(x)]));
      throw_invalid(std::string(kWho) + "two arcs with the same input label " + std::to_string(s.il[size_t(x)]) + " out of node " +
                    std::to_string(s.src[size_t(x)]) + ": the acceptor must be deterministic");
    }
  }
  auto lm = std::make_shared<LmGraph>();
  lm->states = int(N);
  lm->start = s.start[0];
  lm->arcs = A;
  lm->words.assign(size_t(2 * N), word(0, 0, -1, 0));
  lm->words.reserve(size_t(2 * N + A));
  for (int64_t k = 0; k < A;) {
    const int node = s.src[size_t(order[size_t(k)])];
    gtnx_i4& rec = lm->words[size_t(2) * size_t(node)];
    if (s.il[size_t(order[size_t(k)])] == -1) {
      rec.z = s.dst[size_t(order[size_t(k)])];
      rec.w = f2i(wt[order[size_t(k)]]);
      ++k;
    }
    const int begin = int(lm->words.size());
    int count = 0;
    for (; k < A && s.src[size_t(order[size_t(k)])] == node; ++k, ++count) {
      const int a = order[size_t(k)];
      lm->words.push_back(word(s.il[size_t(a)], s.dst[size_t(a)], f2i(wt[a]), 0));
    }
    // (push_back may have moved the words: the record is addressed again)
    gtnx_i4& r = lm->words[size_t(2) * size_t(node)];
    r.x = begin;
    r.y = count;
    if (count > 0) {
      const int first = lm->words[size_t(begin)].x, last = lm->words[size_t(begin) + size_t(count) - 1].x;
      lm->words[size_t(2) * size_t(node) + 1] = word(first, int64_t(last) - first == int64_t(count) - 1 ? 1 : 0, 0, 0);
    }
  }
  // epsilon chains: depth[s] = arcs from s to the first state without an epsilon arc.  A chain is followed until it
  // meets a state that is done or on the chain itself (a cycle)
  std::vector<int> depth(size_t(N), -1);
  std::vector<int> chain;
  std::vector<uint8_t> on(size_t(N), 0);
  for (int64_t s0 = 0; s0 < N; ++s0) {
    chain.clear();
    int u = int(s0);
    while (depth[size_t(u)] < 0) {
      if (on[size_t(u)]) throw_invalid(std::string(kWho) + "an epsilon cycle through node " + std::to_string(u));
      on[size_t(u)] = 1;
      chain.push_back(u);
      const int e = lm->words[size_t(2) * size_t(u)].z;
      if (e < 0) {
        depth[size_t(u)] = 0;
        break;
      }
      u = e;
    }
    for (size_t i = chain.size(); i-- > 0;) {
      const int v = chain[i];
      on[size_t(v)] = 0;
      if (depth[size_t(v)] < 0) depth[size_t(v)] = depth[size_t(lm->words[size_t(2) * size_t(v)].z)] + 1;
      if (depth[size_t(v)] > kLmMaxEpsChain)
        throw_invalid(std::string(kWho) + "an epsilon chain longer than 8 arcs from node " + std::to_string(v));
      lm->eps_chain = std::max(lm->eps_chain, depth[size_t(v)]);
    }
  }
  return lm;
}

bool lm_graph_walk(const LmGraph& lm, int state, int label, float* weight, int* next) {
  if (state < 0 || state >= lm.states) throw_range("[gtnx_lm_graph_walk] state out of range");
  // the device's loops, probe for probe (ctc_beam.hip: lm_walks)
  float sum = 0.0f;
  bool first = true;
  int sn = state;
  if (label >= 0) {
    for (int hop = 0; hop <= kLmMaxEpsChain; ++hop) {
      const gtnx_i4 r0 = lm.words[size_t(2) * size_t(sn)], r1 = lm.words[size_t(2) * size_t(sn) + 1];
      int lo = r0.x, hi = r0.x + r0.y;
      if (r1.y) {  // dense: the only arc it can be
        const int64_t j = int64_t(label) - r1.x;
        if (j >= 0 && j < r0.y) {
          lo = r0.x + int(j);
          hi = lo + 1;
        } else {
          hi = lo;
        }
      }
      for (int step = 0; step < kLmMaxBisect && lo < hi; ++step) {
        const int mid = lo + ((hi - lo) >> 1);
        const gtnx_i4 a = lm.words[size_t(mid)];
        if (a.x == label) {
          const float w = i2f(a.z);
          *weight = first ? w : sum + w;
          *next = a.y;
          return true;
        }
        if (a.x < label) lo = mid + 1;
        else hi = mid;
      }
      if (r0.z < 0) break;
      const float w = i2f(r0.w);
      sum = first ? w : sum + w;
      first = false;
      sn = r0.z;
    }
  }
  *weight = -std::numeric_limits<float>::infinity();
  *next = -1;
  return false;
}

const gtnx_i4* lm_graph_device(LmGraph& lm, const char* who) {
  Runtime& rt = Runtime::get();
  std::lock_guard<std::mutex> lock(lm.mu);
  if (!lm.dev) {
    // (one word more than the form has: the kernel loads the word behind every word it addresses)
    const size_t bytes = sizeof(gtnx_i4) * (lm.words.size() + 1);
    std::vector<gtnx_i4> padded(lm.words);
    padded.push_back(word(0, 0, 0, 0));
    DevMemP d = rt.alloc(bytes);
    rt.h2d(d->ptr, padded.data(), bytes);
    rt.sync();  // once: later decodes may come on another stream, and `padded` goes
    lm.dev = d;
    lm.device = rt.device();
  }
  if (lm.device != rt.device())
    throw_invalid(std::string("[") + who + "] the LM graph was uploaded to device " + std::to_string(lm.device) +
                  ", the calling thread is on device " + std::to_string(rt.device()));
  return lm.dev->as<gtnx_i4>();
}

void* lm_graph_register(LmGraphP lm) {
  std::lock_guard<std::mutex> lock(g_reg_mu);
  const void* h = lm.get();
  g_reg[h] = std::move(lm);
  return const_cast<void*>(h);
}
LmGraphP lm_graph_lookup(const void* handle) {
  std::lock_guard<std::mutex> lock(g_reg_mu);
  auto it = g_reg.find(handle);
  return it == g_reg.end() ? nullptr : it->second;
}
bool lm_graph_unregister(const void* handle) {
  LmGraphP gone;  // (let go of outside the lock)
  {
    std::lock_guard<std::mutex> lock(g_reg_mu);
    auto it = g_reg.find(handle);
    if (it == g_reg.end()) return false;
    gone = std::move(it->second);
    g_reg.erase(it);
  }
  return true;
}

}  // namespace gtnx
