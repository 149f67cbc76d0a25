"""The case list of tests/test_rational_cpu.py (yardstick against the unmodified reference and against the fixture
tests/golden/rational.json) and tests/test_rational_gpu.py (engine against the yardstick): both files import CASES,
TIE_CASES and SCORE_CASES from here, so no GPU case lacks a CPU pin.

A case is a function of an `ops` object -- FpOps (tests/rational_fp.py) or ApiOps (gtn_amd or the reference-backed
mirror) -- that builds its graphs through `ops` only and returns {"results": {name: graph}, "probes": {name: graph}} and,
where an empty probe would prove nothing, "nonempty": the probes that must have arcs.
A result is what a device builder returned; a probe is what a second device operation made of a result BEFORE anything
pulled that result to the host, which is the only way the result's adjacency lists, start / accept lists, counts and
epsilon flag can be seen as they are on the device.  Every graph is deterministic from a seed."""
import os

import numpy as np

import graphgen as gg
import rational_fp as fp

ABSENT = 10 ** 6  # a label no graph carries: remove(g, ABSENT) rewrites g in out-list order, node by node


# ---------------------------------------------------------------- the two back ends
class FpOps:
    """the yardstick"""
    is_fp = True

    def __init__(self):
        self.leaves = []

    def leaf(self, g, calc_grad=True):
        return g

    def linear(self, T, C, w=None):
        return fp.linear(T, C, w)

    def clone(self, g, projection=0):
        return fp.clone(g, projection)

    def concat(self, gs):
        return fp.concat(list(gs))

    def closure(self, g):
        return fp.closure(g)

    def union(self, gs):
        return fp.union(list(gs))

    def remove(self, g, ilabel=fp.EPS, olabel=None):
        return fp.remove(g, ilabel, olabel)

    def compose(self, a, b):
        """the repository's plain C oracle (oracle/gtn_oracle.c), whose node / arc order is the reference's"""
        return fp.norm(ograph(a).compose(ograph(b)).to_dict())

    def save_load(self, g):
        return {k: v.copy() for k, v in g.items() if k not in ("offsets", "sorted")}

    def viterbi_path(self, g):
        return None  # (exact ties: the expected arcs are the reference's recorded ones, tests/golden/rational.json)

    def pull(self, g):
        return g


class ApiOps:
    """gtn_amd, or the reference behind the same Python surface (tests/refbackend/gtn_ref.py)"""
    is_fp = False

    def __init__(self, api, tmp_dir):
        self.api = api
        self.tmp = str(tmp_dir)
        self.leaves = []  # (handle, yardstick graph): the inputs, compared again after the case ran
        self.saved = 0

    def leaf(self, g, calc_grad=True):
        h = to_api(self.api, g, calc_grad)
        self.leaves.append((h, g))
        return h

    def linear(self, T, C, w=None):
        h = self.api.linear_graph(T, C)
        if w is not None and T * C:
            h.set_weights(np.asarray(w, np.float32))
        self.leaves.append((h, fp.linear(T, C, w)))
        return h

    def clone(self, g, projection=0):
        return self.api.clone(g, projection)

    def concat(self, gs):
        return self.api.concat(list(gs))

    def closure(self, g):
        return self.api.closure(g)

    def union(self, gs):
        return self.api.union(list(gs))

    def remove(self, g, ilabel=fp.EPS, olabel=None):
        return self.api.remove(g, ilabel, ilabel if olabel is None else olabel)

    def compose(self, a, b):
        return self.api.compose(a, b)

    def save_load(self, g):
        self.saved += 1
        path = os.path.join(self.tmp, "g%d.bin" % self.saved)
        self.api.save(path, g)
        return self.api.load(path)

    def viterbi_path(self, g):
        return self.api.viterbi_path(g)

    def pull(self, g):
        return from_api(g)


def to_api(api, g, calc_grad=True):
    h = api.Graph(calc_grad)
    if fp.N(g):
        h.add_nodes(g["start"], g["accept"])
    if fp.A(g):
        h.add_arcs(g["src"], g["dst"], g["il"], g["ol"], g["w"])
    return h


def from_api(h):
    s, d, il, ol, w = h.arcs()
    n = h.num_nodes()
    start, accept = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    st, ac = np.asarray(h.start(), np.int64), np.asarray(h.accept(), np.int64)
    assert (np.diff(st) > 0).all() and (np.diff(ac) > 0).all(), "start / accept lists are in node order"
    assert st.size == h.num_start() and ac.size == h.num_accept()
    start[st] = 1
    accept[ac] = 1
    return fp.graph(start, accept, s, d, il, ol, w)


def as_lists(g):
    return {"start": g["start"].tolist(), "accept": g["accept"].tolist(), "src": g["src"].tolist(),
            "dst": g["dst"].tolist(), "il": g["il"].tolist(), "ol": g["ol"].tolist(),
            "w": [float(x) for x in g["w"]], "sort": None}


def ograph(g):
    """the graph in the plain C oracle, a chain marked arc-sorted as linearGraph marks it"""
    from oracle_lib import OGraph, lib
    o = OGraph.from_dict(as_lists(g))
    if g.get("sorted"):
        lib().og_mark_sorted(o.h, 0)
        lib().og_mark_sorted(o.h, 1)
    return o


def same(got, want):
    """None, or what differs first; every comparison is == (weights included: they are copies, or zeros)"""
    for key in ("start", "accept", "src", "dst", "il", "ol", "w"):
        a, b = np.asarray(got[key]), np.asarray(want[key])
        if a.shape != b.shape:
            return "%s: %d entries, expected %d" % (key, a.size, b.size)
        if not np.array_equal(a, b):
            i = int(np.flatnonzero(a != b)[0])
            return "%s[%d] = %r, expected %r" % (key, i, a[i].item(), b[i].item())
    return None


# ---------------------------------------------------------------- generators
def rand_graph(seed, n, a, nlabels=4, eps=0.0, acceptor=False, p_start=0.2, p_accept=0.2, dag=False, int_w=False):
    """n nodes, a arcs in random arc-id order; dag: src < dst; int_w: weights in {0, 1, 2} (exact ties)"""
    rng = np.random.default_rng(seed)
    start = (rng.random(n) < p_start).astype(np.uint8)
    accept = (rng.random(n) < p_accept).astype(np.uint8)
    if n == 0 or (dag and n < 2):
        a = 0
    src = rng.integers(0, max(n - 1, 1) if dag else max(n, 1), a)
    dst = rng.integers(src + 1, n) if dag else rng.integers(0, max(n, 1), a)
    il = rng.integers(0, nlabels, a)
    ol = il.copy() if acceptor else rng.integers(0, nlabels, a)
    if eps > 0:
        il = np.where(rng.random(a) < eps, fp.EPS, il)
        ol = il.copy() if acceptor else np.where(rng.random(a) < eps, fp.EPS, ol)
    w = rng.integers(0, 3, a).astype(np.float32) if int_w else rng.normal(0, 1, a).astype(np.float32)
    return fp.graph(start, accept, src, dst, il, ol, w)


def flags_at(g, starts=(), accepts=(), clear=True):
    """the graph with exactly these start / accept nodes (those inside it)"""
    g = dict(g)
    n = fp.N(g)
    for key, ids in (("start", starts), ("accept", accepts)):
        f = np.zeros(n, np.uint8) if clear else g[key].copy()
        ids = np.asarray([i for i in ids if 0 <= i < n], np.int64)
        f[ids] = 1
        g[key] = f
    return g


def split(g_total_flags, sizes, seed, arcs_per_node=1.5, **kw):
    """graphs of the given sizes whose UNION has the start / accept nodes of g_total_flags = (starts, accepts)"""
    starts, accepts = g_total_flags
    out, off = [], 0
    for k, n in enumerate(sizes):
        g = rand_graph(seed + k, n, int(n * arcs_per_node), **kw)
        out.append(flags_at(g, [s - off for s in starts], [a - off for a in accepts]))
        off += n
    return out


SMALL_Y = rand_graph(900, 3, 4, p_start=0.0, p_accept=0.0)
SMALL_Y = flags_at(SMALL_Y, [0, 2], [1])
SMALL_Z = fp.graph([1, 0, 0], [0, 0, 0], [0, 1], [1, 2], [1, 2])  # (a DAG where nothing accepts: the tie cases)


def _lists_case(total, starts, accepts, seed):
    def case(ops):
        sizes = (total // 2, total // 3, total - total // 2 - total // 3)
        parts = [ops.leaf(g) for g in split((starts, accepts), sizes, seed)]
        x = ops.union(parts)
        y = ops.leaf(SMALL_Y)
        return {"results": {"union": x}, "probes": {"closure": ops.closure(x), "concat": ops.concat([x, y]),
                                                     "concat_before": ops.concat([y, x])}}
    return case


EDGE = (1022, 1023, 1024, 2048)
CASES = {}
for _n in (1023, 1024, 1025, 2049):
    CASES["lists_N%d" % _n] = _lists_case(_n, (0,) + EDGE, (5,) + EDGE, 10 + _n)
CASES["lists_many_starts"] = _lists_case(2049, [n for n in range(2049) if n % 4], (3, 1024, 2047), 31)
CASES["lists_no_accept"] = _lists_case(1025, (0, 1023, 1024), (), 32)
CASES["lists_start_and_accept"] = _lists_case(2049, (1024,), (1024,), 33)


# ---- connectors
def _with_counts(seed, n, a, n_start, n_accept, **kw):
    """n_start start nodes and n_accept accept nodes at seeded places (they may overlap)"""
    rng = np.random.default_rng(seed + 7)
    g = rand_graph(seed, n, a, **kw)
    return flags_at(g, rng.permutation(n)[:n_start].tolist(), rng.permutation(n)[:n_accept].tolist())


EMPTY = fp.graph([], [])
C1 = _with_counts(40, 30, 50, 3, 20)    # 20 accepts
C2 = _with_counts(41, 25, 40, 15, 15)   # x 15 starts = 300 connectors; 15 accepts
C3 = _with_counts(42, 30, 45, 20, 4)    # x 20 starts = 300 connectors
C_NOACC = _with_counts(43, 12, 20, 2, 0)


def _concat_case(parts):
    def case(ops):
        hs = [ops.leaf(g) for g in parts]
        r = ops.concat(hs)
        return {"results": {"concat": r}, "probes": {"remove_eps": ops.remove(r), "closure": ops.closure(r)}}
    return case


CASES["conn_concat3"] = _concat_case([C1, C2, C3])
CASES["conn_no_accept"] = _concat_case([C_NOACC, C2, C3])
CASES["conn_empty_middle"] = _concat_case([C1, EMPTY, C3])
CASES["conn_empty_first"] = _concat_case([EMPTY, C2, C3])
CASES["conn_empty_last"] = _concat_case([C1, C2, EMPTY])
CASES["conn_single"] = _concat_case([C2])
CASES["conn_none"] = _concat_case([])


def _concat_self(ops):
    g = ops.leaf(C2)
    r = ops.concat([g, g])
    return {"results": {"concat": r}, "probes": {"remove_eps": ops.remove(r)}}


CASES["conn_self"] = _concat_self


def _closure_case(g0):
    def case(ops):
        r = ops.closure(ops.leaf(g0))
        return {"results": {"closure": r}, "probes": {"remove_eps": ops.remove(r), "closure": ops.closure(r)}}
    return case


CASES["closure_150"] = _closure_case(_with_counts(44, 400, 600, 150, 150))
CASES["closure_empty"] = _closure_case(EMPTY)


# ---- implicit chains as inputs
def _chain_case(T, C):
    def case(ops):
        rng = np.random.default_rng(50 + T)
        w1, w2 = rng.normal(0, 1, T * C).astype(np.float32), rng.normal(0, 1, T * C).astype(np.float32)
        a, b = ops.linear(T, C, w1), ops.linear(T, C, w2)
        g = ops.leaf(C_NOACC if T == 0 else C2)
        res = {"clone": ops.clone(a), "project_input": ops.clone(a, 1), "project_output": ops.clone(a, 2),
               "closure": ops.closure(a), "union_mixed": ops.union([a, g, b]), "union_chains": ops.union([a, b]),
               "concat_mixed": ops.concat([g, a, g]), "concat_chains": ops.concat([a, b, a])}
        return {"results": res, "probes": {"remove_eps_concat_mixed": ops.remove(res["concat_mixed"]),
                                           "remove_eps_concat_chains": ops.remove(res["concat_chains"]),
                                           "closure_union_mixed": ops.closure(res["union_mixed"]),
                                           "remove_eps_closure": ops.remove(res["closure"])}}
    return case


for _t, _c in ((1, 1), (3, 5), (0, 4)):
    CASES["chain_%dx%d" % (_t, _c)] = _chain_case(_t, _c)


def _chain_remove(ops):
    r = ops.remove(ops.linear(5, 3), 1)
    return {"results": {"remove": r}, "probes": {"closure": ops.closure(r)}}


CASES["chain_remove"] = _chain_remove


# ---- projections of a transducer with epsilons on one side only
def _projection_case(side):
    def case(ops):
        g = flags_at(rand_graph(60 + side, 8, 22, nlabels=3), [0, 3], [5, 7])
        rng = np.random.default_rng(61)
        hit = rng.random(22) < 0.3
        g["il" if side == 0 else "ol"] = np.where(hit, fp.EPS, g["il" if side == 0 else "ol"]).astype(np.int32)
        t = ops.leaf(g)
        chain = ops.linear(3, 3, rng.normal(0, 1, 9).astype(np.float32))
        pi, po = ops.clone(t, 1), ops.clone(t, 2)
        return {"results": {"project_input": pi, "project_output": po},
                "probes": {"compose_pi_chain": ops.compose(pi, chain), "compose_chain_po": ops.compose(chain, po),
                           "compose_po_chain": ops.compose(po, chain), "compose_chain_pi": ops.compose(chain, pi)},
                "nonempty": ["compose_pi_chain", "compose_chain_po", "compose_po_chain", "compose_chain_pi"]}
    return case


CASES["project_eps_in"] = _projection_case(0)
CASES["project_eps_out"] = _projection_case(1)


# ---- sort width and stability (the tie probes of these graphs: TIE_CASES)
def _sort_graphs(total):
    """two DAGs with integer weights whose union has `total` nodes, with arcs from and into the last node"""
    na = total - 100
    ga = rand_graph(70 + total, na, 2 * na, dag=True, int_w=True, nlabels=1000, p_start=0.02, p_accept=0.0)
    gb = rand_graph(71 + total, 100, 300, dag=True, int_w=True, nlabels=1000, p_start=0.1, p_accept=0.1)
    gb["dst"][::7] = 99      # into the last node ...
    gb["src"][::7] = np.minimum(gb["src"][::7], 98)
    gb["accept"][99] = 1
    ga["accept"][na - 1] = 1
    ga["dst"][::5] = na - 1
    ga["src"][::5] = np.minimum(ga["src"][::5], na - 2)
    for g in (ga, gb):  # shortestDistance wants every node without in-arcs to be a start node (shortest.cpp)
        g["start"][np.bincount(g["dst"], minlength=fp.N(g)) == 0] = 1
    return ga, gb


def _sort_loops(g, seed):
    """the same graph with a tenth of its arcs turned round (cycles) and a self-loop on the last node"""
    g = dict(g)
    rng = np.random.default_rng(seed)
    flip = rng.random(fp.A(g)) < 0.1
    src, dst = np.where(flip, g["dst"], g["src"]), np.where(flip, g["src"], g["dst"])
    src[0] = dst[0] = fp.N(g) - 1   # from and into the last node
    src[1] = fp.N(g) - 1
    g["src"], g["dst"] = src.astype(np.int32), dst.astype(np.int32)
    return g


def _sort_case(total):
    def case(ops):
        ga, gb = _sort_graphs(total)
        r = ops.union([ops.leaf(ga), ops.leaf(_sort_loops(gb, total))])
        return {"results": {"union": r}, "probes": {"remove_absent": ops.remove(r, ABSENT)}}
    return case


for _n in (256, 257, 65536, 65537):
    CASES["sort_N%d" % _n] = _sort_case(_n)


def hub_graph(loops, seed=80):
    """node 100 with 5000 in-arcs from the nodes below it and 5000 out-arcs to the nodes above it, arc ids shuffled;
    every arc has its own label; loops: self-loops on the hub and elsewhere"""
    rng = np.random.default_rng(seed)
    src = np.concatenate([rng.integers(0, 100, 5000), np.full(5000, 100)])
    dst = np.concatenate([np.full(5000, 100), rng.integers(101, 201, 5000)])
    if loops:
        src = np.concatenate([src, [100] * 10, [3, 150, 200]])
        dst = np.concatenate([dst, [100] * 10, [3, 150, 200]])
    perm = rng.permutation(src.size)
    start, accept = np.zeros(201, np.uint8), np.zeros(201, np.uint8)
    start[:100] = 1
    accept[101:] = 1
    return fp.graph(start, accept, src[perm], dst[perm], np.arange(src.size))  # (weights 0: every path ties)


def _hub_case(ops):
    r = ops.union([ops.leaf(SMALL_Y), ops.leaf(hub_graph(True))])
    return {"results": {"union": r}, "probes": {"remove_absent": ops.remove(r, ABSENT)}}


CASES["sort_hub"] = _hub_case


# ---- grid stride: more arcs than one pass of 4096 x 256 lanes
def _stride_case(ops):
    rng = np.random.default_rng(90)
    chain = ops.linear(4100, 256, rng.normal(0, 1, 4100 * 256).astype(np.float32))
    u = ops.union([chain, ops.leaf(rand_graph(91, 5, 9))])
    return {"results": {"union": u}, "probes": {"remove_absent": ops.remove(u, ABSENT), "save_load": ops.save_load(u)}}


CASES["grid_stride"] = _stride_case


# ---- many inputs
def _many_parts(ops, count, seed):
    rng = np.random.default_rng(seed)
    pool = [ops.leaf(rand_graph(seed + k, int(rng.integers(1, 7)), int(rng.integers(0, 9)), p_start=0.4, p_accept=0.4))
            for k in range(12)]
    pool += [ops.leaf(EMPTY), ops.linear(2, 3, rng.normal(0, 1, 6).astype(np.float32)), ops.linear(1, 1), ops.linear(0, 2)]
    return [pool[int(i)] for i in rng.integers(0, len(pool), count)]


def _many_case(ops):
    parts = _many_parts(ops, 300, 100)
    u, c = ops.union(parts), ops.concat(parts)
    return {"results": {"union": u, "concat": c}, "probes": {"closure_union": ops.closure(u), "remove_eps_concat": ops.remove(c)}}


CASES["many_300"] = _many_case


def _grid_y_case(ops):
    """more inputs than the grid's y dimension holds (65535): the segment dimension runs in slices, and concat's
    look-back at the previous input crosses the slice edges"""
    pool = []
    for k in range(5):
        pool.append(ops.leaf(fp.graph([1, 0], [0, 1], [0], [1], [k], [k + 10], [0.5 * k])))
    parts = [pool[(i * 7) % 5] for i in range(65537)]
    u, c = ops.union(parts), ops.concat(parts)
    return {"results": {"union": u, "concat": c}, "probes": {"remove_absent_union": ops.remove(u, ABSENT),
                                                             "closure_concat": ops.closure(c)}}


CASES["grid_y_65537"] = _grid_y_case


# ---- binary loader: below 4096 arcs the host route, from 4096 the device route
def _load_case(n, a, seed):
    def case(ops):
        g = ops.leaf(rand_graph(seed, n, a, eps=0.05, p_start=0.01, p_accept=0.01))
        h = ops.save_load(g)
        return {"results": {"loaded": h}, "probes": {"remove_absent": ops.remove(h, ABSENT), "closure": ops.closure(h)}}
    return case


CASES["load_4095"] = _load_case(300, 4095, 110)
CASES["load_4096"] = _load_case(300, 4096, 110)
CASES["load_sparse"] = _load_case(6000, 4096, 111)


# ---- remove: the walk's semantics, all small
def _g(n, starts, accepts, arcs):
    """arcs: (src, dst, ilabel[, olabel])"""
    s = np.zeros(n, np.uint8)
    a = np.zeros(n, np.uint8)
    s[list(starts)] = 1
    a[list(accepts)] = 1
    return fp.graph(s, a, [x[0] for x in arcs], [x[1] for x in arcs], [x[2] for x in arcs],
                    [x[3] if len(x) > 3 else x[2] for x in arcs])


E = fp.EPS
REMOVE_GRAPHS = {
    "rm_chain_3000": (_g(3002, [0], [3001], [(i, i + 1, E) for i in range(3000)] + [(3000, 3001, 5)]), E, E),
    "rm_cycle": (_g(4, [0], [3], [(0, 1, E), (1, 2, E), (2, 0, E), (1, 3, 1), (2, 3, 2), (0, 0, E)]), E, E),
    "rm_diamond": (_g(5, [0], [4], [(0, 1, E), (0, 2, E), (2, 3, E), (1, 3, E), (3, 4, 1), (1, 4, 2), (3, 4, 3)]), E, E),
    "rm_accept_through_eps": (_g(4, [0], [3], [(0, 1, 1), (1, 2, E), (2, 3, E)]), E, E),
    "rm_eps_only_node_dropped": (_g(4, [0], [3], [(0, 1, E), (1, 3, 2), (0, 2, 1), (2, 1, E)]), E, E),
    "rm_start_with_eps_in": (_g(3, [0, 1], [2], [(0, 1, E), (1, 2, 1), (0, 2, 2)]), E, E),
    "rm_all_match": (_g(3, [0], [2], [(0, 1, E), (1, 2, E), (2, 0, E)]), E, E),
    "rm_no_start_all_match": (_g(3, [], [2], [(0, 1, E), (1, 2, E)]), E, E),
    "rm_label_present": (_g(3, [0], [2], [(0, 1, 7), (1, 2, 7, 8), (1, 2, 8, 7), (0, 2, 9)]), 7, 7),
}


def _remove_case(name):
    def case(ops):
        g, il, ol = REMOVE_GRAPHS[name]
        r = ops.remove(ops.leaf(g), il, ol)
        return {"results": {"remove": r}, "probes": {"closure": ops.closure(r), "remove_again": ops.remove(r, il, ol)}}
    return case


for _name in REMOVE_GRAPHS:
    CASES[_name] = _remove_case(_name)


def _remove_transducer(ops):
    g = rand_graph(120, 6, 14, nlabels=2, p_start=0.4, p_accept=0.4)
    k = np.arange(14, dtype=np.int32)   # labels 2 and 3: the pairs (2, 2), (3, 2), (2, 3), (3, 3) all occur
    g["il"], g["ol"] = 2 + k % 2, 2 + k // 2 % 2
    r = ops.remove(ops.leaf(g), 2, 3)
    return {"results": {"remove": r}, "probes": {"closure": ops.closure(r), "remove_32": ops.remove(r, 3, 2)}}


CASES["rm_transducer_2_3"] = _remove_transducer


def _remove_product(ops):
    """remove on a composition built on the device (its out-lists are not stored as lists there)"""
    a = rand_graph(225, 6, 16, nlabels=2, eps=0.3, p_start=0.4, p_accept=0.4)   # (seeds picked for a product of 18
    b = rand_graph(275, 5, 14, nlabels=2, eps=0.3, p_start=0.4, p_accept=0.4)   # nodes with 20 epsilon:epsilon arcs)
    p = ops.compose(ops.leaf(a), ops.leaf(b))
    r = ops.remove(p)
    return {"results": {"remove": r}, "probes": {"closure": ops.closure(r)}}


CASES["rm_product"] = _remove_product


def _remove_twice(ops):
    g = ops.leaf(rand_graph(123, 12, 40, nlabels=2, eps=0.4, acceptor=True))
    r1 = ops.remove(g)
    r2 = ops.remove(r1)
    return {"results": {"remove": r1, "remove_remove": r2}, "probes": {"closure": ops.closure(r2)}}


CASES["rm_twice"] = _remove_twice


def batch2_graph():
    """6000 nodes, all kept: rows = floor(2^25 / 6000) = 5592 < K, so the walks of nodes 5592.. run in a second batch
    over the scratch rows of nodes 0..407.  Node n has an epsilon arc forwards (inside its block of 6), one backwards
    -- from a node of the second batch straight to the node whose walk used the same row -- and one labelled arc into
    a permutation of the nodes, which keeps every node.  Out-degree <= 3, arc ids shuffled."""
    n = 6000
    rows = (1 << 25) // n
    assert rows == 5592
    ids = np.arange(n)
    fwd = ids[(ids + 1) % 6 != 0]
    back = ids[(ids >= rows) | (ids % 6 != 0)]
    back_to = np.where(back >= rows, back - rows, back - 1)
    src = np.concatenate([fwd, back, ids])
    dst = np.concatenate([fwd + 1, back_to, (ids * 31 + 7) % n])
    lab = np.concatenate([np.full(fwd.size + back.size, E), ids % 11])
    perm = np.random.default_rng(130).permutation(src.size)
    start, accept = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    start[[0, 5999]] = 1
    accept[ids % 9 == 4] = 1
    return fp.graph(start, accept, src[perm], dst[perm], lab[perm])


def _batch2_case(ops):
    r = ops.remove(ops.leaf(batch2_graph()))
    return {"results": {"remove": r}, "probes": {"closure": ops.closure(r)}}


CASES["rm_second_batch"] = _batch2_case


# ---------------------------------------------------------------- exact ties: viterbi_path reads the in-lists
def _tie_concat(ops):
    """every path through concat([g1, g2]) scores 0 and every arc has its own label, so the labels of the best path
    say which connector -- which entry of an in-list -- won"""
    g1 = _g(6, [0], [1, 2, 3, 4], [(0, 4, 13), (0, 2, 11), (0, 1, 10), (0, 3, 12), (0, 5, 14), (5, 3, 15)])
    g2 = _g(5, [0, 1, 2], [3, 4], [(2, 3, 22), (0, 3, 20), (1, 3, 21), (1, 4, 23), (0, 4, 24)])
    return ops.viterbi_path(ops.concat([ops.leaf(g1), ops.leaf(g2)]))


def _tie_hub(ops):
    return ops.viterbi_path(ops.union([ops.leaf(SMALL_Z), ops.leaf(hub_graph(False))]))


def _tie_sort(total):
    def case(ops):
        ga, gb = _sort_graphs(total)
        return ops.viterbi_path(ops.union([ops.leaf(ga), ops.leaf(gb)]))
    return case


TIE_CASES = {"tie_concat": _tie_concat, "tie_hub": _tie_hub}
for _n in (256, 257, 65536, 65537):
    TIE_CASES["tie_sort_N%d" % _n] = _tie_sort(_n)


# ---------------------------------------------------------------- scores and gradients
def _dag(seed, n, n_start, n_accept, nlabels=3):
    g = fp.norm(gg.random_dag(np.random.default_rng(seed), n, avg_deg=2.5, nlabels=nlabels, n_start=n_start,
                              n_accept=n_accept))
    # the reference's backward sweep starts at the accept nodes and waits for every out-arc of a node (shortest.cpp:
    # 41-80): a dead end that does not accept would hold its predecessors' gradients at zero there.  None here:
    rng = np.random.default_rng(seed + 1000)
    dead = [k for k in range(n) if not g["accept"][k] and not (g["src"] == k).any()]
    extra = [(k, int(rng.integers(k + 1, n)), int(rng.integers(0, nlabels)), float(np.float32(rng.normal()))) for k in dead]
    g = fp.graph(g["start"], g["accept"], np.append(g["src"], [e[0] for e in extra]),
                 np.append(g["dst"], [e[1] for e in extra]), np.append(g["il"], [e[2] for e in extra]), None,
                 np.append(g["w"], [e[3] for e in extra]))
    return g


# name -> (kind, input graphs, calc_grad per input)
SCORE_CASES = {
    "score_concat3": ("concat", [_dag(140, 9, 2, 3), _dag(141, 8, 3, 2), _dag(142, 10, 2, 2)], [True, False, True]),
    "score_union": ("union", [_dag(143, 9, 2, 3), _dag(144, 7, 3, 2), _dag(145, 8, 2, 2)], [True, True, True]),
    # g has no node that is both start and accept, so closure(g) composed with a chain has no epsilon cycle
    "score_closure_chain": ("closure_chain", [_dag(146, 7, 2, 2), fp.linear(4, 3, np.random.default_rng(147).normal(
        0, 1, 12))], [True, True]),
}


# a retained tape run twice: the second run seeds the score's gradient again (1, then 2 in all); every level below
# adds what its parent holds by then to what it got in the first run: 1 + 2 = 3 for the scored graph, 1 + 3 = 4 for
# its inputs, 1 + 4 = 5 one level further down (addGrad accumulates, graph.cpp:91-129).  Factor per input:
TWICE = {"concat": [4.0, 4.0, 4.0], "union": [4.0, 4.0, 4.0], "closure_chain": [5.0, 4.0]}


def score_yardstick(name, tropical):
    """(score, [gradient of every input]) in float64 on the yardstick's graph, sliced by the yardstick's offsets"""
    kind, gs, _ = SCORE_CASES[name]
    if kind in ("concat", "union"):
        r = fp.concat(gs) if kind == "concat" else fp.union(gs)
        score, grad = fp.score_and_grad(r, tropical)
        return score, [grad[o:o + fp.A(g)] for o, g in zip(r["offsets"].tolist(), gs)]
    cl = fp.closure(gs[0])
    prod = ograph(cl).compose(ograph(gs[1]))
    info = prod.grad_info()
    score, grad = fp.score_and_grad(fp.norm(prod.to_dict()), tropical)
    g_cl, g_chain = np.zeros(fp.A(cl)), np.zeros(fp.A(gs[1]))
    for col, acc in ((0, g_cl), (1, g_chain)):
        ok = info[:, col] >= 0
        np.add.at(acc, info[ok, col], grad[ok])
    o = int(cl["offsets"][0])
    return score, [g_cl[o:o + fp.A(gs[0])], g_chain]


def score_api(api, name, tropical, twice=False):
    """the same through an API: (score, gradients; None where calc_grad is off)"""
    kind, gs, cg = SCORE_CASES[name]
    hs = [to_api(api, g, c) for g, c in zip(gs, cg)]
    if kind == "concat":
        r = api.concat(hs)
    elif kind == "union":
        r = api.union(hs)
    else:
        r = api.compose(api.closure(hs[0]), hs[1])
    sc = api.viterbi_score(r) if tropical else api.forward_score(r)
    api.backward(sc, True)
    if twice:
        api.backward(sc, True)
    return sc.item(), [h.grad().weights_to_numpy() if c else None for h, c in zip(hs, cg)], hs
