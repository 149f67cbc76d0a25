"""The yardstick of the built-graph shortest-distance kernels (gtn_amd/csrc/shortest.hip: forwardScore, viterbiScore,
viterbiPath and their gradients on host-built graphs), in plain numpy; nothing of the engine is imported here.

  * seeded generators of TRIM graphs (every node on a start -> accept path, so the reference's queue quirks -- dead ends
    that block its reverse queue, nodes it never reaches -- do not enter): layered DAGs and chains with forward arcs;
  * two host forms of shortest.cpp's recursion, float64 and float32, the same code with another number type.  A case's
    `err` for a quantity is max(|float32 form - float64 form|, 2^-23 * max(1, |float64 value|)): what the number format
    costs on this graph, computed without the device;
  * vetting of tropical / path cases: both forms take the same arc at every node of the best path and the same accept
    node, and the runner-up is at least 64 err away, so a correct float32 kernel cannot legitimately choose otherwise;
  * a replica of the host's dispatch (ops_built.cpp: op_shortest_distance, SdOp::backward, op_viterbi_path;
    shortest.hip: launch_sd_forward / launch_sd_backward / pick_group) over a replica of the level schedule
    (graph.cpp: build_host_schedule), so that every case names the kernel cell it must land in and the CPU suite can
    check that name before a GPU is spent on it;
  * the case lists of tests/test_shortest_cells_gpu.py.

A graph is a tests/graphgen.py dict with numpy arrays; the input label of an arc is its id, so a path's labels name its
arcs.  Node ids are topological (src < dst)."""
import functools

import numpy as np

EPS32 = 2.0 ** -23
VET_GAP = 64.0

# the constants of the dispatch (shortest.hip / ops_built.cpp)
K_RING, K_CA, K_CN = 4096, 2048, 1024  # forward ring, arcs and nodes of a level (kRing, kCA, kCN)
K_DEEP_P = 24576                       # kDeepP


# ---------------------------------------------------------------------------------------------------- generators
def _finish(rng, N, start, accept, src, dst, int_weights, wscale, sort, shuffle_labels=False):
    src, dst = np.asarray(src, np.int32), np.asarray(dst, np.int32)
    perm = rng.permutation(src.size)  # arc ids are not in-row order
    src, dst = src[perm], dst[perm]
    assert (src < dst).all()
    if int_weights:
        w = rng.integers(-2, 2, src.size).astype(np.float32)
    else:
        w = (rng.normal(0.0, 1.0, src.size) * wscale).astype(np.float32)
    il = np.arange(src.size, dtype=np.int32)
    if shuffle_labels:  # labels still name the arcs, but label order is not arc-id order: arc_sort permutes the lists
        il = rng.permutation(src.size).astype(np.int32)
    return {"start": np.asarray(start, np.uint8), "accept": np.asarray(accept, np.uint8), "src": src, "dst": dst,
            "il": il, "ol": il.copy(), "w": w, "sort": sort}


def spread(total, n):
    """n integers, as equal as possible, that sum to total"""
    q, r = divmod(int(total), int(n))
    return [q + (1 if i < r else 0) for i in range(n)]


def layered(seed, widths, indeg, back=1, extra_starts=0, extra_accepts=0, int_weights=False, wscale=1.0, extra=(),
            total_arcs=None, sort=None, shuffle_labels=False):
    """Layered DAG: widths[l] nodes on level l (node ids level by level), level 0 the start nodes, the last level the
    accept nodes.  `indeg`: in-degree of every node of levels >= 1 -- one number, or one per level >= 1 (a number or a
    list per node).  Every node takes its first in-arc from the previous level (which fixes its level), every node of
    the previous level is taken at least once (trim), the other sources are drawn from up to `back` levels back.
    extra_starts / extra_accepts: that many nodes of the middle levels are start / accept as well (such a start node
    keeps its in-arcs).  extra: (src node, dst node) arcs on top.  total_arcs: in-degrees are nudged by one, node after
    node, until the graph has exactly that many arcs.  int_weights: weights in {-2..1} (ties).  shuffle_labels: the labels
    are a seeded permutation of the arc ids (drawn last: structure and weights are those of the unshuffled graph), so
    that sort="i" really reorders every in- and out-list."""
    rng = np.random.default_rng(seed)
    widths = [int(x) for x in widths]
    L = len(widths)
    off = np.concatenate([[0], np.cumsum(widths)]).astype(np.int64)
    N = int(off[-1])
    deg = np.zeros(N, np.int64)
    for l in range(1, L):
        d = indeg if np.isscalar(indeg) else indeg[l - 1]
        deg[off[l]:off[l + 1]] = d
    if total_arcs is not None:
        diff = int(total_arcs) - len(extra) - int(deg.sum())
        nodes = np.arange(off[1], N)
        i = 0
        while diff != 0:
            n = nodes[i % nodes.size]
            i += 1
            if diff < 0 and deg[n] <= 1:
                continue
            deg[n] += 1 if diff > 0 else -1
            diff += -1 if diff > 0 else 1
    src, dst = [], []
    for l in range(1, L):
        prev = np.arange(off[l - 1], off[l])
        nodes = np.arange(off[l], off[l + 1])
        d = deg[nodes]
        S = int(d.sum())
        assert (d >= 1).all() and S >= prev.size, "level %d cannot take every node of level %d" % (l, l - 1)
        slot = np.arange(S) - np.repeat(np.cumsum(d) - d, d)
        srcs = rng.integers(off[max(0, l - back)], off[l], S)
        first = np.flatnonzero(slot == 0)
        srcs[first] = prev[np.arange(nodes.size) % prev.size]
        if prev.size > nodes.size:
            rest = prev[nodes.size:]
            others = np.flatnonzero(slot != 0)[:rest.size]
            assert others.size == rest.size
            srcs[others] = rest
        src.append(srcs)
        dst.append(np.repeat(nodes, d))
    for s, t in extra:
        src.append(np.asarray([s]))
        dst.append(np.asarray([t]))
    start = np.zeros(N, np.uint8)
    accept = np.zeros(N, np.uint8)
    start[:off[1]] = 1
    accept[off[L - 1]:] = 1
    mid = np.arange(off[1], off[L - 1])
    if extra_starts:
        start[rng.choice(mid, extra_starts, replace=False)] = 1
    if extra_accepts:
        accept[rng.choice(mid, extra_accepts, replace=False)] = 1
    g = _finish(rng, N, start, accept, np.concatenate(src), np.concatenate(dst), int_weights, wscale, sort,
                shuffle_labels)
    g["level_off"] = off
    return g


def chain(seed, P, extra, in_hubs=(), out_hubs=(), extra_accepts=0, starts=(0,), wscale=1.0, long_arc=False,
          int_weights=False):
    """0 -> 1 -> ... -> P-1 (a node per dependency level) plus about `extra` random forward arcs; in_hubs / out_hubs:
    (position, degree) pairs -- that node has EXACTLY that in- / out-degree, the chain's arc included; long_arc: one
    arc 0 -> P-1; extra_accepts: that many other nodes accept too; starts: the start nodes (0 must be one; the others
    keep their in-arcs)."""
    rng = np.random.default_rng(seed)
    src, dst = [np.arange(P - 1)], [np.arange(1, P)]
    hin, hout = dict(in_hubs), dict(out_hubs)
    for p, d in hin.items():
        assert 1 <= p < P and d >= 1
        src.append(rng.integers(0, p, d - 1))
        dst.append(np.full(d - 1, p))
    for p, d in hout.items():
        assert 0 <= p < P - 1 and d >= 1
        t = rng.integers(p + 1, P, d - 1)
        for _ in range(100):
            bad = np.isin(t, list(hin))
            if not bad.any():
                break
            t[bad] = rng.integers(p + 1, P, int(bad.sum()))
        assert not np.isin(t, list(hin)).any()
        src.append(np.full(d - 1, p))
        dst.append(t)
    if extra:
        s = rng.integers(0, P - 1, extra)
        t = s + 1 + (rng.random(extra) * (P - 1 - s)).astype(np.int64)
        keep = ~np.isin(t, list(hin)) & ~np.isin(s, list(hout))
        src.append(s[keep])
        dst.append(t[keep])
    if long_arc:
        assert (P - 1) not in hin and 0 not in hout
        src.append(np.asarray([0]))
        dst.append(np.asarray([P - 1]))
    start = np.zeros(P, np.uint8)
    accept = np.zeros(P, np.uint8)
    start[list(starts)] = 1
    assert start[0]
    accept[P - 1] = 1
    if extra_accepts:
        accept[rng.choice(np.arange(1, P - 1), extra_accepts, replace=False)] = 1
    return _finish(rng, P, start, accept, np.concatenate(src), np.concatenate(dst), int_weights, wscale, None)


def wide_chain(seed, steps, arcs, int_weights=False):
    """benchmarks/functions.cpp's makeLinear in small: `arcs` parallel arcs per step, a node per level"""
    rng = np.random.default_rng(seed)
    src = np.repeat(np.arange(steps), arcs)
    start = np.zeros(steps + 1, np.uint8)
    accept = np.zeros(steps + 1, np.uint8)
    start[0] = accept[steps] = 1
    return _finish(rng, steps + 1, start, accept, src, src + 1, int_weights, 1.0, None)


def with_neg_inf_arc(g, seed=0):
    """-inf on an arc whose destination has another, finite in-arc (so it lies on no best path)"""
    g = dict(g)
    rng = np.random.default_rng(seed)
    deg = np.bincount(g["dst"], minlength=g["start"].size)
    cand = np.flatnonzero(deg[g["dst"]] >= 2)
    w = g["w"].copy()
    w[cand[rng.integers(0, cand.size)]] = -np.inf
    g["w"] = w
    return g


def with_dead_accepts(g, every=3):
    """every `every`-th accept node of the last level gets -inf on all its in-arcs: reachable, but with score -inf"""
    g = dict(g)
    acc = np.flatnonzero(g["accept"])
    dead = acc[acc >= g["level_off"][-2]][::every]
    w = g["w"].copy()
    w[np.isin(g["dst"], dead)] = -np.inf
    g["w"] = w
    g["dead_accepts"] = dead
    return g


def as_lists(g):
    """for tests/oracle_lib.py: plain Python numbers"""
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in g.items() if k in
            ("start", "accept", "src", "dst", "il", "ol", "w", "sort")}


def _csr(key, n):
    lst = np.argsort(key, kind="stable").astype(np.int64)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(key, minlength=n), out=off[1:])
    return off, lst


def is_trim(g):
    """every node lies on a path from a start node to an accept node (structure only)"""
    n = g["start"].size
    src, dst = g["src"], g["dst"]
    fwd = g["start"].astype(bool).copy()
    bwd = g["accept"].astype(bool).copy()
    order = np.argsort(dst, kind="stable")
    for a in order:  # dst ascending = topological: sources are final
        if fwd[src[a]]:
            fwd[dst[a]] = True
    for a in np.argsort(src, kind="stable")[::-1]:
        if bwd[dst[a]]:
            bwd[src[a]] = True
    return bool(fwd.all() and bwd.all()) and n > 0


# ---------------------------------------------------------------------------------------------------- host forms
def sweep(g, dtype, tropical=False, grad=True):
    """shortest.cpp's recursion over the nodes in id order, every operation in `dtype` (np.float64 / np.float32).
    Log semiring: {"alpha", "score", "grad"} with the gradient by the engine's regrouping (node gradients pulled over
    the out-rows, linear domain).  Tropical: {"alpha", "score", "best" (arg-max in-arc per node, -1: the start's own
    0), "acc" (accept node), "gap" (per node: best minus runner-up candidate), "acc_gap", "path" (arc ids, first arc
    first), "grad" (0/1)}."""
    F = dtype
    n = g["start"].size
    src, dst = g["src"].astype(np.int64), g["dst"].astype(np.int64)
    w = g["w"].astype(F)
    in_off, in_list = _csr(dst, n)
    start = g["start"]
    alpha = np.full(n, -np.inf, F)
    best = np.full(n, -1, np.int64)
    gap = np.full(n, np.inf)
    zero = np.zeros(1, F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for v in range(n):
            arcs = in_list[in_off[v]:in_off[v + 1]]
            t = alpha[src[arcs]] + w[arcs]
            if start[v]:
                t = np.concatenate([t, zero])
            if t.size == 0:
                continue
            m = t.max()
            if m == -np.inf:
                continue
            if tropical:
                alpha[v] = m
                k = int(np.argmax(t))
                best[v] = arcs[k] if k < arcs.size else -1
                if t.size > 1:
                    gap[v] = float(m) - float(np.partition(t, -2)[-2])
            else:
                alpha[v] = m + np.log(np.exp(t - m).sum(dtype=F))
        acc = np.flatnonzero(g["accept"])
        a = alpha[acc]
        m = a.max()
        out = {"alpha": alpha}
        if tropical:
            k = int(np.argmax(a))
            out.update(score=F(m), best=best, acc=int(acc[k]), gap=gap,
                       acc_gap=(float(m) - float(np.partition(a, -2)[-2])) if a.size > 1 else np.inf)
            path = []
            u = int(acc[k])
            while m > -np.inf and best[u] >= 0:
                path.append(int(best[u]))
                u = int(src[best[u]])
            out["path"] = path[::-1]
            gr = np.zeros(src.size, F)
            gr[path] = 1
            out["grad"] = gr
            return out
        score = m + np.log(np.exp(a - m).sum(dtype=F)) if m > -np.inf else F(m)
        out["score"] = F(score)
        if not grad:
            return out
        out_off, out_list = _csr(src, n)
        ng = np.zeros(n, F)
        gr = np.zeros(src.size, F)
        denom = np.exp(score - m)
        accept = g["accept"]
        for u in range(n - 1, -1, -1):
            arcs = out_list[out_off[u]:out_off[u + 1]]
            v = dst[arcs]
            gl = ng[v] * np.exp(alpha[u] + w[arcs] - alpha[v])
            gr[arcs] = gl
            s = gl.sum(dtype=F)
            if accept[u]:
                s = s + np.exp(alpha[u] - m) / denom
            ng[u] = s
        out["grad"] = gr
    return out


def err_of(v32, v64):
    v64, v32 = np.asarray(v64, np.float64), np.asarray(v32, np.float64)
    with np.errstate(invalid="ignore"):
        diff = np.where(v32 == v64, 0.0, np.abs(v32 - v64))  # (equal infinities are equal)
        return np.maximum(diff, EPS32 * np.maximum(1.0, np.where(np.isfinite(v64), np.abs(v64), 1.0)))


def yardstick(g, log_grad=True, tropical=True):
    """both host forms of a case: log {"score", "score_err", "grad", "grad_err"}; tropical {"score32", "grad", "path",
    "vet" (None or the reason the case does not vet)}"""
    out = {}
    l64, l32 = sweep(g, np.float64, grad=log_grad), sweep(g, np.float32, grad=log_grad)
    out["score"] = float(l64["score"])
    out["score_err"] = float(err_of(l32["score"], l64["score"]))
    if log_grad:
        out["grad"] = l64["grad"]
        out["grad_err"] = err_of(l32["grad"], l64["grad"])
    if tropical:
        t64, t32 = sweep(g, np.float64, True), sweep(g, np.float32, True)
        out["trop_score32"] = np.float32(t32["score"])
        out["trop_grad"] = t64["grad"].astype(np.float32)
        out["trop_path"] = t64["path"]
        out["vet"] = _vet(g, t64, t32)
    return out


def _vet(g, t64, t32):
    if t64["path"] != t32["path"] or t64["acc"] != t32["acc"]:
        return "the two host forms take different paths"
    e = err_of(t32["alpha"], t64["alpha"])
    nodes = [t64["acc"]] + [int(g["src"][a]) for a in t64["path"]]
    for v in nodes:
        if not t64["gap"][v] >= VET_GAP * e[v]:
            return "node %d: runner-up %.3g away, err %.3g" % (v, t64["gap"][v], e[v])
    if not t64["acc_gap"] >= VET_GAP * e[t64["acc"]]:
        return "accept reduction: runner-up %.3g away" % t64["acc_gap"]
    return None


def in_lists_as_built(g):
    """per node, the in-arcs in the order the graph's in-list has once it is built: arc-id order, or -- sort "i" --
    by input label (graph.cpp arcSort; labels here are distinct, so the order is total)"""
    n = g["start"].size
    key = g["dst"].astype(np.int64) * (g["src"].size + 1) + (g["il"] if g.get("sort") == "i" else np.arange(g["src"].size))
    lst = np.argsort(key, kind="stable")
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(g["dst"], minlength=n), out=off[1:])
    return [lst[off[v]:off[v + 1]] for v in range(n)]


def tie_census(g):
    """(nodes with two equal best finite candidates, those of them on the best path, accept nodes that share the best
    score, tied nodes whose FIRST best candidate in in-list order is not the best candidate with the smallest arc id)
    of an integer-weight case, in float64 -- exact for integers.  Where the last count is zero, ranking ties by in-row
    slot and ranking them by arc id cannot be told apart."""
    t = sweep(g, np.float64, True)
    acc = np.flatnonzero(g["accept"])
    a = t["alpha"][acc]
    on_path = [t["acc"]] + [int(g["src"][k]) for k in t["path"]]
    rows = in_lists_as_built(g)
    w = g["w"].astype(np.float64)
    differ = 0
    for v in np.flatnonzero(t["gap"] == 0):
        arcs = rows[v]
        c = t["alpha"][g["src"][arcs]] + w[arcs]
        best = arcs[c == t["alpha"][v]]
        if best.size >= 2 and best[0] != best.min():
            differ += 1
    return int((t["gap"] == 0).sum()), int((t["gap"][on_path] == 0).sum()), int((a == a.max()).sum()), differ


# ---------------------------------------------------------------------------------------------------- dispatch replica
class Sched:
    pass


def sched_stats(g):
    """graph.cpp: build_host_schedule in small -- the reference's FIFO order gives the positions, the dependency depth
    the levels; a trim graph schedules every node and writes every out-arc"""
    if "_sched" in g:  # (kept on the graph; weights do not enter)
        return g["_sched"]
    n = int(g["start"].size)
    src, dst = g["src"].tolist(), g["dst"].tolist()
    out_off, out_list = _csr(g["src"], n)
    out_off, out_list = out_off.tolist(), out_list.tolist()
    deg = np.bincount(g["dst"], minlength=n).tolist()
    level = [0] * n
    order = [v for v in np.flatnonzero(g["start"]).tolist() if deg[v] == 0]
    head = 0
    while head < len(order):
        u = order[head]
        head += 1
        lu = level[u] + 1
        for k in range(out_off[u], out_off[u + 1]):
            d = dst[out_list[k]]
            if level[d] < lu:
                level[d] = lu
            deg[d] -= 1
            if deg[d] == 0:
                order.append(d)
    assert len(order) == n, "not every node is scheduled: the graph is not trim"
    pos = np.empty(n, np.int64)
    pos[order] = np.arange(n)
    lv = np.asarray(level)[order]
    assert (np.diff(lv) >= 0).all()
    s = Sched()
    s.N, s.A, s.P, s.L = n, len(src), n, int(lv[-1]) + 1
    level_off = np.searchsorted(lv, np.arange(s.L + 1))
    s.max_width = int(np.diff(level_off).max())
    indeg_p = np.bincount(g["dst"], minlength=n)[order]
    row_off = np.concatenate([[0], np.cumsum(indeg_p)])
    s.max_level_arcs = int(np.diff(row_off[level_off]).max())
    # per level: end position minus the smallest source position of its in-arcs
    dl = np.asarray(level)[g["dst"]]
    mn = np.full(s.L, n, np.int64)
    np.minimum.at(mn, dl, pos[g["src"]])
    mn = np.minimum(mn, level_off[:-1])
    s.max_reach = int((level_off[1:] - mn).max())
    s.n_in = s.n_out = s.A
    g["_sched"] = s
    return s


def pick_group(x16):
    return 256 if x16 >= 192 * 16 else 64 if x16 >= 24 * 16 else 8 if x16 >= 4 * 16 else 1


def _narrow_fwd(ss):
    ok = all(s.max_level_arcs <= K_CA and s.max_width <= K_CN and s.max_reach <= K_RING and s.A <= 16 * s.N for s in ss)
    return ok and sum(s.L for s in ss) >= 32 * len(ss)


def _deep(ss, no_deep):
    return (not no_deep) and all(64 <= s.P <= K_DEEP_P and 4 * s.L >= s.P and s.A <= 64 * s.P for s in ss)


def predict(gs, what, no_deep=False):
    """the cell a batch of host-built graphs lands in; what: "fwd_log", "fwd_trop", "path", "bwd_log", "bwd_trop".
    (Host-built schedules carry neither row-ordered weights nor identity out-rows: the narrow kernel is the plain log
    forward one only, and no backward is narrow.)"""
    ss = [sched_stats(g) for g in gs]
    g = pick_group((sum(s.n_in for s in ss) * 16) // sum(s.P for s in ss))
    if what == "fwd_log":
        if _narrow_fwd(ss):
            return "fwd/narrow/log"
        return "fwd/deep" if _deep(ss, no_deep) else "fwd/generic/log/g%d" % g
    if what == "bwd_log":
        return "bwd/deep" if _deep(ss, no_deep) else "bwd/generic/log/g%d" % g
    return {"fwd_trop": "fwd/generic/tropical/g%d", "path": "fwd/generic/path/g%d", "bwd_trop": "bwd/generic/tropical/g%d"}[what] % g


def generic_cells(G):
    return {"fwd_log": "fwd/generic/log/g%d" % G, "bwd_log": "bwd/generic/log/g%d" % G,
            "fwd_trop": "fwd/generic/tropical/g%d" % G, "bwd_trop": "bwd/generic/tropical/g%d" % G,
            "path": "fwd/generic/path/g%d" % G}


# ---------------------------------------------------------------------------------------------------- the case lists
# name -> (builder, cells).  Builders are seeded; a seed that does not vet is replaced by the next one by hand, the
# shape stays (tests/test_shortest_cells_cpu.py keeps every case vetted).
def _g1():
    return layered(101, [37] * 9, 2, back=3)


def _g8(total):
    return lambda: layered(111, [37] * 5, 5, back=2, total_arcs=total)


def _g64_pair(total, seed=121):
    return lambda: layered(seed, [37] * 5, 30, back=2, total_arcs=total)


def _g64():
    return layered(131, [5] * 7, [24, 65, 191, 24, 65, 191], back=2)


def _g256_pair(total):
    return lambda: layered(141, [5] * 4, 256, back=2, total_arcs=total)


def _g256(width):
    return lambda: layered(150 + width, [width] * 9, [192, 257, 300, 513, 513, 300, 257, 192], back=2)


_ONCE = {1: ([37] * 4, 2), 8: ([37] * 4, 6), 64: ([5] * 4, 40), 256: ([3] * 4, 260)}


def _accepts300(G):
    # a last level of 300 accept nodes, every third of them with score -inf
    widths, d = _ONCE[G]
    last = max(d, -(-widths[-1] // 300) + 1)
    return lambda: with_dead_accepts(layered(160 + G, widths + [300], [d] * (len(widths) - 1) + [last], back=2))


def _accepts300_live(G):
    # the same shape with every accept node reachable: the log gradient over n_accept > 256
    widths, d = _ONCE[G]
    last = max(d, -(-widths[-1] // 300) + 1)
    return lambda: layered(160 + G, widths + [300], [d] * (len(widths) - 1) + [last], back=2)


def _starts(G):
    widths, d = _ONCE[G]
    return lambda: layered(170 + G, widths + [widths[0]], d, back=2, extra_starts=2, extra_accepts=2)


def _neg_arc(G):
    widths, d = _ONCE[G]
    return lambda: with_neg_inf_arc(layered(180 + G, widths + [widths[0]], d, back=2), seed=G)


GENERIC = {
    "g1/9x37": (_g1, 1),
    "g8/5x37/x16=64": (_g8(740), 8),
    "g8/5x37/x16=63": (_g8(739), 1),
    "g64/5x37/x16=384": (_g64_pair(4440), 64),
    "g64/5x37/x16=383": (_g64_pair(4439), 8),
    "g64/7x5/deg24-65-191": (_g64, 64),
    "g256/4x5/x16=3072": (_g256_pair(3840), 256),
    "g256/4x5/x16=3071": (_g256_pair(3839), 64),
    "g256/9x1": (_g256(1), 256),
    "g256/9x2": (_g256(2), 256),
    "g256/9x3": (_g256(3), 256),
}
for _G in (1, 8, 64, 256):
    GENERIC["g%d/300-accepts" % _G] = (_accepts300(_G), _G)
    GENERIC["g%d/300-live-accepts" % _G] = (_accepts300_live(_G), _G)
    GENERIC["g%d/starts-with-in-arcs" % _G] = (_starts(_G), _G)
    GENERIC["g%d/neg-inf-arc" % _G] = (_neg_arc(_G), _G)

# integer weights: ties at nodes and at the accept reduction; judged with == against the oracle
TIES = {}
for _G, (_w, _d) in ((8, (37, 6)), (64, (5, 40)), (256, (3, 260))):
    for _sort in (None, "i"):
        TIES["g%d/%s" % (_G, "sorted" if _sort else "unsorted")] = (
            (lambda w=_w, d=_d, G=_G, srt=_sort: layered(190 + G, [w] * 5, d, back=2, int_weights=True, sort=srt,
                                                           shuffle_labels=srt is not None)), _G)

# deep family: name -> (builder, whether it qualifies for the one-wave kernels); the generic cell it takes under
# GTNX_NO_DEEP=1, or when it does not qualify, is in expected_cells()
DEEP = {
    "deep/P=64": (lambda: chain(201, 64, 20 * 64), True),
    "deep/P=65": (lambda: chain(202, 65, 20 * 65), True),
    "deep/P=130": (lambda: chain(203, 130, 20 * 130), True),
    "deep/P=63": (lambda: chain(204, 63, 20 * 63), False),
    "deep/P=24576": (lambda: chain(205, 24576, 24576), True),
    "deep/P=24577": (lambda: chain(206, 24577, 24577), False),
    "deep/in-hub-64": (lambda: chain(207, 4300, 4300, in_hubs=[(2150, 64)], long_arc=True), True),
    "deep/in-hub-65": (lambda: chain(208, 4300, 4300, in_hubs=[(2150, 65)], long_arc=True), True),
    "deep/in-hub-2048": (lambda: chain(209, 4300, 4300, in_hubs=[(2150, 2048)], long_arc=True), True),
    "deep/in-hub-2049": (lambda: chain(210, 4300, 4300, in_hubs=[(2150, 2049)], long_arc=True), True),
    "deep/in-hubs-2x1100": (lambda: chain(211, 4300, 4300, in_hubs=[(2150, 1100), (2151, 1100)], long_arc=True), True),
    "deep/out-hub-64": (lambda: chain(212, 4300, 4300, out_hubs=[(2150, 64)], long_arc=True), True),
    "deep/out-hub-65": (lambda: chain(213, 4300, 4300, out_hubs=[(2150, 65)], long_arc=True), True),
    "deep/out-hub-2048": (lambda: chain(214, 4300, 4300, out_hubs=[(2150, 2048)], long_arc=True), True),
    "deep/out-hub-2049": (lambda: chain(215, 4300, 4300, out_hubs=[(2150, 2049)], long_arc=True), True),
    "deep/out-hubs-2x1100": (lambda: chain(216, 4300, 4300, out_hubs=[(2150, 1100), (2151, 1100)], long_arc=True), True),
    "deep/130-accepts-3-starts": (lambda: chain(217, 4300, 4300, extra_accepts=129, starts=(0, 1, 2150), long_arc=True), True),
    "deep/weights-x30": (lambda: chain(218, 4300, 4300, wscale=30.0, long_arc=True), True),
}


def _edge_levels(n):
    return lambda: layered(301, [5] * n, 2)


def _edge_width(w):
    return lambda: layered(302, [5] * 15 + [w, 5] + [5] * 15, [2] * 14 + [1, -(-w // 5)] + [2] * 15)


def _edge_level_arcs(total):
    d = spread(total, 512)
    return lambda: layered(303, [5] * 15 + [512, 5] + [5] * 15, [2] * 14 + [d, 103] + [2] * 15)


def _edge_reach(reach):
    # level 5 ends at position `reach`, and one of its nodes takes an arc from node 0 (position 0)
    k = reach // 1000
    w = reach - 5 - 1000 * k
    widths = [5] + [1000] * k + [w] + [5] * 30
    return lambda: layered(304, widths, [2] * k + [-(-1000 // w) + 1, -(-w // 5) + 1] + [2] * 29, extra=[(0, 5 + 1000 * k)])


def _edge_a16n(over):
    return lambda: layered(305, [8] * 32, 16, total_arcs=16 * 256 + over)


# host-built narrow eligibility: the pair on either side of every rule
NARROW = {
    "narrow/levels=32": _edge_levels(32), "narrow/levels=31": _edge_levels(31),
    "narrow/width=1024": _edge_width(1024), "narrow/width=1025": _edge_width(1025),
    "narrow/level-arcs=2048": _edge_level_arcs(2048), "narrow/level-arcs=2049": _edge_level_arcs(2049),
    "narrow/reach=4096": _edge_reach(4096), "narrow/reach=4097": _edge_reach(4097),
    "narrow/reach=2048": _edge_reach(2048), "narrow/reach=2049": _edge_reach(2049),
    "narrow/A=16N": _edge_a16n(0), "narrow/A=16N+1": _edge_a16n(1),
}
NARROW_CELLS = {
    "narrow/levels=32": ("fwd/narrow/log", "bwd/generic/log/g1"), "narrow/levels=31": ("fwd/generic/log/g1", "bwd/generic/log/g1"),
    "narrow/width=1024": ("fwd/narrow/log", "bwd/generic/log/g1"), "narrow/width=1025": ("fwd/generic/log/g1", "bwd/generic/log/g1"),
    "narrow/level-arcs=2048": ("fwd/narrow/log", "bwd/generic/log/g8"), "narrow/level-arcs=2049": ("fwd/generic/log/g8", "bwd/generic/log/g8"),
    "narrow/reach=4096": ("fwd/narrow/log", "bwd/generic/log/g1"), "narrow/reach=4097": ("fwd/generic/log/g1", "bwd/generic/log/g1"),
    # (kRingB = 2048 bounds the BACKWARD ring, which needs identity out-rows: a host-built graph never has them, so
    #  both sides of this pair take the ring forward and the generic kernel backward)
    "narrow/reach=2048": ("fwd/narrow/log", "bwd/generic/log/g1"), "narrow/reach=2049": ("fwd/narrow/log", "bwd/generic/log/g1"),
    "narrow/A=16N": ("fwd/narrow/log", "bwd/generic/log/g8"), "narrow/A=16N+1": ("fwd/generic/log/g8", "bwd/generic/log/g8"),
}


def _batch_row_among_thin():
    return [wide_chain(401, 12, 300)] + [layered(410 + i, [37] * 9, 2, back=3) for i in range(20)]


def _batch_thin_among_rows():
    return [wide_chain(430 + i, 8, 400) for i in range(20)] + [layered(451, [37] * 3, 2)]


def _batch_deep_and_small():
    return [chain(461, 130, 20 * 130), chain(462, 40, 20 * 40)]


def _batch_narrow_and_not():
    return [layered(471, [5] * 32, 2), layered(472, [5] * 31, 2), layered(473, [5] * 20, 2)]


# name -> (builder of the list, G the batch totals give; every batch here ends on the generic family)
BATCHES = {
    "batch/300-arc-row-among-20-thin": (_batch_row_among_thin, 1),
    "batch/thin-among-20-wide-rows": (_batch_thin_among_rows, 256),
    "batch/deep-and-P<64": (_batch_deep_and_small, 8),
    "batch/narrow-and-not": (_batch_narrow_and_not, 1),
}


@functools.lru_cache(maxsize=None)
def build(name):
    for table in (GENERIC, TIES, DEEP, BATCHES):
        if name in table:
            return table[name][0]()
    return NARROW[name]()


@functools.lru_cache(maxsize=None)
def case_yardstick(name, index=None):
    g = build(name)
    if index is not None:
        g = g[index]
    dead = "dead_accepts" in g
    return yardstick(g, log_grad=not dead, tropical=not (name in DEEP or name in NARROW))


def expected_cells(name, no_deep=False):
    """what -> cell name, as the case list states it"""
    if name in GENERIC or name in TIES:
        return generic_cells((GENERIC.get(name) or TIES[name])[1])
    if name in DEEP:
        if DEEP[name][1] and not no_deep:
            return {"fwd_log": "fwd/deep", "bwd_log": "bwd/deep"}
        G = 8 if name in ("deep/P=64", "deep/P=65", "deep/P=130", "deep/P=63") else 1
        return {"fwd_log": "fwd/generic/log/g%d" % G, "bwd_log": "bwd/generic/log/g%d" % G}
    if name in NARROW:
        return dict(zip(("fwd_log", "bwd_log"), NARROW_CELLS[name]))
    return generic_cells(BATCHES[name][1])
