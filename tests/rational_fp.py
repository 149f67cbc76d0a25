"""The yardstick of the device-built rational operations (gtn_amd/csrc/rational.hip, ops_rational.cpp): plain numpy
versions of clone(projection), concat, closure, union and remove(ilabel, olabel), written from the reference's
documented construction (functions.cpp:66-318) -- inputs in order, each graph's arcs followed by the connectors into
it (concat), the new start node first (closure), remove's per-kept-node breadth-first walk in out-list order with the
weights dropped -- plus the adjacency lists in arc-id order, the ordered start / accept lists, the arc offset of every
input (the gradient slice) and a float64 forward / backward over a DAG.

A graph here is a dict of numpy arrays: start, accept (uint8 [N]); src, dst, il, ol (int32 [A]); w (float32 [A]);
results of concat / closure / union also carry "offsets" (int64 [inputs]), a chain of linear() "sorted".  tests/test_rational_cpu.py pins every
function to the unmodified reference; tests/test_rational_gpu.py compares the engine with it.  Everything that can
meet a million arcs is vectorised; only remove's walk over nodes that HAVE a matching out-arc is a Python loop."""
import numpy as np

EPS = -1


def graph(start, accept, src=(), dst=(), il=(), ol=None, w=None):
    src = np.asarray(src, dtype=np.int32).reshape(-1)
    il = np.asarray(il, dtype=np.int32).reshape(-1)
    return {
        "start": np.asarray(start, dtype=np.uint8).reshape(-1), "accept": np.asarray(accept, dtype=np.uint8).reshape(-1),
        "src": src, "dst": np.asarray(dst, dtype=np.int32).reshape(-1), "il": il,
        "ol": il.copy() if ol is None else np.asarray(ol, dtype=np.int32).reshape(-1),
        "w": np.zeros(src.size, np.float32) if w is None else np.asarray(w, dtype=np.float32).reshape(-1),
    }


def norm(d):
    """a tests/graphgen.py dict (lists) as a graph of this module; arc-sorted graphs are not handled here"""
    assert d.get("sort") in (None, "both"), "adjacency of an arc-sorted graph is not in arc-id order"
    return graph(d["start"], d["accept"], d["src"], d["dst"], d["il"], d["ol"], d["w"])


def linear(T, C, w=None):
    """creations.cpp:20-33: T + 1 nodes, node 0 starts, node T accepts (T = 0: nobody accepts), arc t * C + c"""
    t = np.repeat(np.arange(T, dtype=np.int32), C)
    start = np.zeros(T + 1, np.uint8)
    accept = np.zeros(T + 1, np.uint8)
    start[0] = 1
    if T > 0:
        accept[T] = 1
    g = graph(start, accept, t, t + 1, np.tile(np.arange(C, dtype=np.int32), T), None, w)
    g["sorted"] = True  # (markArcSorted on both sides, creations.cpp:30-31: compose picks its matcher by it)
    return g


def N(g):
    return int(g["start"].size)


def A(g):
    return int(g["src"].size)


def start_list(g):
    return np.flatnonzero(g["start"]).astype(np.int32)


def accept_list(g):
    return np.flatnonzero(g["accept"]).astype(np.int32)


def adjacency(g):
    """(out_off, out_list, in_off, in_list): lists in arc-id order (graph.cpp:62-63)"""
    res = []
    for key in ("src", "dst"):
        k = g[key]
        lst = np.argsort(k, kind="stable").astype(np.int32)
        off = np.zeros(N(g) + 1, np.int64)
        np.cumsum(np.bincount(k, minlength=N(g)), out=off[1:])
        res += [off, lst]
    return tuple(res)


def out_lists(g):
    oo, ol, _, _ = adjacency(g)
    return [ol[oo[n]:oo[n + 1]].tolist() for n in range(N(g))]


def in_lists(g):
    _, _, io, il = adjacency(g)
    return [il[io[n]:io[n + 1]].tolist() for n in range(N(g))]


# ---------------------------------------------------------------- clone / concat / closure / union
def clone(g, projection=0):
    """functions.cpp:66-92; projection 1: both labels the input label, 2: both the output label"""
    out = {k: v.copy() for k, v in g.items() if k not in ("offsets", "sorted")}
    if projection == 1:
        out["ol"] = g["il"].copy()
    elif projection == 2:
        out["il"] = g["ol"].copy()
    out["offsets"] = np.zeros(1, np.int64)
    return out


def _cat(parts, dtype):
    parts = [np.asarray(p, dtype=dtype).reshape(-1) for p in parts]
    return np.concatenate(parts) if parts else np.zeros(0, dtype)


def union(gs):
    """functions.cpp:188-223: nodes and arcs of the inputs in order, node ids shifted"""
    noff = np.concatenate([[0], np.cumsum([N(g) for g in gs])]).astype(np.int64)
    aoff = np.concatenate([[0], np.cumsum([A(g) for g in gs])]).astype(np.int64)
    shift = np.repeat(noff[:-1], [A(g) for g in gs]).astype(np.int32)
    out = graph(_cat([g["start"] for g in gs], np.uint8), _cat([g["accept"] for g in gs], np.uint8),
                _cat([g["src"] for g in gs], np.int32) + shift, _cat([g["dst"] for g in gs], np.int32) + shift,
                _cat([g["il"] for g in gs], np.int32), _cat([g["ol"] for g in gs], np.int32),
                _cat([g["w"] for g in gs], np.float32))
    out["offsets"] = aoff[:-1].copy()
    return out


def concat(gs):
    """functions.cpp:97-153: graph i's arcs, then an epsilon arc for every (accept p of graph i - 1, start q of graph
    i) with p the slow index; only the first graph's starts and the last graph's accepts survive"""
    if not gs:
        out = graph([1], [1])
        out["offsets"] = np.zeros(0, np.int64)
        return out
    src, dst, il, ol, w, st, ac, offs = [], [], [], [], [], [], [], []
    noff = a = 0
    for i, g in enumerate(gs):
        st.append(g["start"] if i == 0 else np.zeros(N(g), np.uint8))
        ac.append(g["accept"] if i == len(gs) - 1 else np.zeros(N(g), np.uint8))
        offs.append(a)
        src.append(g["src"] + noff), dst.append(g["dst"] + noff), il.append(g["il"]), ol.append(g["ol"]), w.append(g["w"])
        a += A(g)
        if i > 0:
            p = accept_list(gs[i - 1]) + (noff - N(gs[i - 1]))
            q = start_list(g) + noff
            k = p.size * q.size
            src.append(np.repeat(p, q.size)), dst.append(np.tile(q, p.size))
            il.append(np.full(k, EPS)), ol.append(np.full(k, EPS)), w.append(np.zeros(k))
            a += k
        noff += N(g)
    out = graph(_cat(st, np.uint8), _cat(ac, np.uint8), _cat(src, np.int32), _cat(dst, np.int32), _cat(il, np.int32),
                _cat(ol, np.int32), _cat(w, np.float32))
    out["offsets"] = np.asarray(offs, np.int64)
    return out


def closure(g):
    """functions.cpp:155-186: node 0 is the new start / accept node; the graph's arcs, then 0 -> every old start, then
    every old accept -> 0, all epsilon"""
    s, a = start_list(g) + 1, accept_list(g) + 1
    k = s.size + a.size
    start = np.zeros(N(g) + 1, np.uint8)
    start[0] = 1
    out = graph(start, start.copy(), _cat([g["src"] + 1, np.zeros(s.size), a], np.int32),
                _cat([g["dst"] + 1, s, np.zeros(a.size)], np.int32), _cat([g["il"], np.full(k, EPS)], np.int32),
                _cat([g["ol"], np.full(k, EPS)], np.int32), _cat([g["w"], np.zeros(k)], np.float32))
    out["offsets"] = np.zeros(1, np.int64)
    return out


# ---------------------------------------------------------------- remove
def remove(g, ilabel=EPS, olabel=None):
    """functions.cpp:257-318.  Kept nodes: start nodes and nodes with an in-arc that does not carry the label pair, in
    node order.  From every kept node a breadth-first walk over the matching arcs (queue order, out-lists in arc-id
    order): every other arc met is emitted from the kept node, an accept node met makes it accept.  Weights are 0."""
    olabel = ilabel if olabel is None else olabel
    n = N(g)
    match = (g["il"] == ilabel) & (g["ol"] == olabel)
    keep = g["start"].astype(bool).copy()
    keep[g["dst"][~match]] = True
    new_id = np.cumsum(keep) - 1
    roots = np.flatnonzero(keep)
    oo, ol, _, _ = adjacency(g)
    has_match = np.zeros(n, bool)
    has_match[g["src"][match]] = True
    accept = g["accept"][roots].astype(np.uint8)
    # nodes without a matching out-arc emit their own out-list, in order: one slice each, gathered at once
    if not has_match[roots].any():
        emitted = ol[keep[g["src"][ol]]].astype(np.int64)
        src_new = new_id[g["src"][emitted]]
    else:
        dst, acc_in = g["dst"], g["accept"]
        pieces = []
        for k, r in enumerate(roots.tolist()):
            if not has_match[r]:
                pieces.append(ol[oo[r]:oo[r + 1]])
                continue
            seen, queue, head, mine, acc = {r}, [r], 0, [], False
            while head < len(queue):
                nxt = queue[head]
                head += 1
                acc = acc or bool(acc_in[nxt])
                for arc in ol[oo[nxt]:oo[nxt + 1]].tolist():
                    if match[arc]:
                        dn = int(dst[arc])
                        if dn not in seen:
                            seen.add(dn)
                            queue.append(dn)
                    else:
                        mine.append(arc)  # (emitted from the kept node, whatever node the arc leaves)
            accept[k] = 1 if acc else 0
            pieces.append(mine)
        emitted = _cat(pieces, np.int64)
        src_new = np.repeat(np.arange(roots.size), [len(p) for p in pieces])
    return graph(g["start"][roots], accept, src_new, new_id[g["dst"][emitted]], g["il"][emitted], g["ol"][emitted])


# ---------------------------------------------------------------- float64 forward / backward over a DAG
def _topo(g):
    n = N(g)
    indeg = np.bincount(g["dst"], minlength=n).astype(np.int64)
    outs = out_lists(g)
    order = [i for i in range(n) if indeg[i] == 0]
    head = 0
    while head < len(order):
        u = order[head]
        head += 1
        for a in outs[u]:
            v = int(g["dst"][a])
            indeg[v] -= 1
            if indeg[v] == 0:
                order.append(v)
    assert len(order) == n, "the graph has a cycle"
    return order, outs


def score_and_grad(g, tropical=False):
    """shortestDistance (shortest.cpp) in float64: (score, d score / d arc weight [A]).  Log semiring: the gradient of
    an arc is its posterior; tropical: 1 on the arcs of the best path (ties: the arc met first in in-list order, which
    the callers avoid by using generic weights).  -inf and zeros when no accepting path exists."""
    order, outs = _topo(g)
    n, w = N(g), g["w"].astype(np.float64)
    ins = in_lists(g)
    alpha = np.full(n, -np.inf)
    best = np.full(n, -1, np.int64)
    for u in order:
        terms = [alpha[int(g["src"][a])] + w[a] for a in ins[u]]
        if g["start"][u]:
            terms.append(0.0)
        if not terms:
            continue
        m = max(terms)
        if m == -np.inf:
            continue
        if tropical:
            alpha[u] = m
            k = int(np.argmax(terms))
            best[u] = ins[u][k] if k < len(ins[u]) else -1
        else:
            alpha[u] = m + np.log(sum(np.exp(t - m) for t in terms))
    acc = accept_list(g)
    grad = np.zeros(A(g))
    if acc.size == 0 or not np.isfinite(alpha[acc]).any():
        return -np.inf, grad
    if tropical:
        u = int(acc[int(np.argmax(alpha[acc]))])
        score = alpha[u]
        while best[u] >= 0:
            grad[best[u]] = 1.0
            u = int(g["src"][best[u]])
        return float(score), grad
    m = alpha[acc].max()
    score = m + np.log(np.exp(alpha[acc] - m).sum())
    beta = np.full(n, -np.inf)  # log of d score / d alpha, seeded at the accept nodes
    for u in reversed(order):
        terms = [beta[int(g["dst"][a])] + w[a] for a in outs[u]]
        if g["accept"][u]:
            terms.append(0.0)
        terms = [t for t in terms if t > -np.inf]
        if terms:
            mm = max(terms)
            beta[u] = mm + np.log(sum(np.exp(t - mm) for t in terms))
    with np.errstate(invalid="ignore"):
        e = alpha[g["src"]] + w + beta[g["dst"]] - score
    grad = np.where(np.isfinite(e), np.exp(e), 0.0)
    return float(score), grad
