"""ASG scores of token lattices and their gradients (TEST INFRASTRUCTURE ONLY).

Three things live here, shared by test_asg_lattice_cpu.py and test_asg_lattice_gpu.py:
  * the float64 yardstick: a dynamic program over the arcs of a lattice (one token state per arc, no blank) -- score,
    d score / d emissions by alpha-beta, d score / d arc weights as the arcs' posteriors, d score / d table as the
    occupancies of the start entries, the self-loops and the edges;
  * a float32 transcription of gtn_amd/csrc/asg_lattice.hip: the same recurrences with float32 arithmetic in the
    kernel's order (an arc's predecessors and successors one after the other, a label's arcs along its chain, an arc's and
    an edge's frames descending, a table row's utterances, arcs and edges ascending), so that the float32 error of the
    METHOD can be measured against the gates before a GPU is involved;
  * the generated cases, computed once per process and left unchanged.
The lattice builders are tests/ctc_lattice_fp.py's, the table layout and the gates tests/asg_score_fp.py's.
The contract: -inf when T_b == 0, num_nodes < 1, nodes + arcs > max_states, more edges than max_edges
(an edge is a pair of arcs a' -> a with dst a' == src a), an arc with src < 0, src >= dst or dst >= num_nodes, an arc out
of dst order, a label outside 0 .. C - 1, a weight that is +inf or NaN, or no alignment (a one-node lattice has none); a
-inf score or a weight g of exactly 0 gives zero gradients.
"""
import collections
import functools

import numpy as np

import ctc_lattice_fp as cfp
from asg_score_fp import (NEG, SCORE_GATE, GRAD_GATE, TABLE_GATE, CONFIGS, config, table_of, logadd32, score_ok,
                          score_err, grad_err, table_err, model_of)
from ctc_lattice_fp import (lattice_of, paths_of, sort_by_dst, chain_lattice, random_lattice, lattice_of_states, sausage,
                            pack, gout_of, decomposition, the_pieces)

__all__ = ["NEG", "SCORE_GATE", "GRAD_GATE", "TABLE_GATE", "CONFIGS", "config", "table_of", "score_ok", "score_err",
           "grad_err", "table_err", "lattice_of", "paths_of", "chain_lattice", "pack", "the_pieces"]

MAX_STATES, MAX_EDGES = 4096, 1 << 21


def default_max_edges(max_states):
    return min(8 * max_states, MAX_EDGES)


# ---- the edges of a lattice, CSR-wise ----
Edges = collections.namedtuple("Edges", "A lo deg off E to frm osort olo odeg final")


def edges_of(src, dst, K):
    """arc a's incoming edges are the arcs lo[a] .. lo[a] + deg[a] (those entering src a), numbered off[a] ..; `to` and
    `frm` per edge; the arcs leaving node n are osort[olo[n] .. olo[n] + odeg[n]] (ascending); `final` enter K - 1"""
    A = src.size
    nodes = np.arange(K)
    nlo, nhi = np.searchsorted(dst, nodes, "left"), np.searchsorted(dst, nodes, "right")
    lo = nlo[src] if A else np.zeros(0, np.int64)
    deg = (nhi[src] - nlo[src]) if A else np.zeros(0, np.int64)
    off = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    E = int(off[-1])
    to = np.repeat(np.arange(A), deg)
    frm = lo[to] + (np.arange(E) - off[to]) if E else np.zeros(0, np.int64)
    osort = np.argsort(src, kind="stable")
    olo = np.searchsorted(src[osort], nodes, "left")
    odeg = np.searchsorted(src[osort], nodes, "right") - olo
    return Edges(A, lo, deg, off[:-1], E, to, frm, osort, olo, odeg, np.arange(nlo[K - 1], nhi[K - 1]))


def edge_count(src, dst, K):
    nodes = np.arange(K)
    indeg = np.searchsorted(dst, nodes, "right") - np.searchsorted(dst, nodes, "left")
    return int(indeg[src].sum()) if src.size else 0


def lattice_for(case, b):
    """(src, dst, lab, w, K) of utterance b, or None where the lattice alone makes the score -inf"""
    C = case.em.shape[2]
    lat = lattice_of(case.arcs[b], case.num_arcs[b], case.num_nodes[b], None if case.weights is None else case.weights[b],
                     C, case.max_states)
    if lat is None or edge_count(lat[0], lat[1], lat[4]) > max_edges_of(case):
        return None
    return lat


# ---- float64 ----
def _reduceat(values, starts, has, fill):
    """logaddexp over the runs that begin at starts[has] (the runs of the others are empty)"""
    out = np.full(has.size, fill)
    if values.size and has.any():
        out[has] = np.logaddexp.reduceat(values, starts[has])
    return out


def lattice_fp64(em, trans, start, src, dst, lab, w, K):
    """(score, d / d em [T, C], d / d w [A], d / d table [C + C * C]) of one lattice under em [T, C], float64; the
    gradients are None when the score is -inf"""
    x = np.asarray(em, dtype=np.float64)
    T, C = x.shape
    A = src.size
    if T == 0 or A == 0:
        return NEG, None, None, None
    tr, st, w = np.asarray(trans, np.float64), np.asarray(start, np.float64), np.asarray(w, np.float64)
    g = edges_of(src, dst, K)
    wself = tr[lab, lab]
    ew = w[g.to] + tr[lab[g.to], lab[g.frm]]
    first = src == 0
    has_in = g.deg > 0
    alpha = np.full((T, A), NEG)
    with np.errstate(invalid="ignore"):
        alpha[0, first] = (w[first] + st[lab[first]]) + x[0, lab[first]]
        for t in range(1, T):
            inn = _reduceat(alpha[t - 1][g.frm] + ew, g.off, has_in, NEG)
            alpha[t] = np.logaddexp(alpha[t - 1] + wself, inn) + x[t, lab]
            alpha[t][np.isnan(alpha[t])] = NEG
        z = float(np.logaddexp.reduce(alpha[T - 1, g.final])) if g.final.size else NEG
    if not np.isfinite(z):
        return NEG, None, None, None
    # the edges by the arc they leave: beta gathers over them
    by_frm = np.argsort(g.frm, kind="stable")
    fstart = np.searchsorted(g.frm[by_frm], np.arange(A))
    has_out = np.bincount(g.frm, minlength=A) > 0
    beta = np.full((T, A), NEG)
    beta[T - 1, g.final] = 0.0
    p_edge, p_self = np.zeros(g.E), np.zeros(A)
    with np.errstate(invalid="ignore"):
        for t in range(T - 1, 0, -1):
            m = beta[t] + x[t, lab]
            out = _reduceat((ew + m[g.to])[by_frm], fstart, has_out, NEG)
            v = np.logaddexp(m + wself, out)
            beta[t - 1] = np.where(np.isnan(v), NEG, v)
            p_edge += np.nan_to_num(np.exp(alpha[t - 1][g.frm] + ew + m[g.to] - z), nan=0.0)
            p_self += np.nan_to_num(np.exp(alpha[t - 1] + wself + m - z), nan=0.0)
        occ = np.nan_to_num(np.exp(alpha + beta - z), nan=0.0)
    p_start = np.where(first, occ[0], 0.0)
    grad = np.zeros((T, C))
    for t in range(T):
        grad[t] = np.bincount(lab, weights=occ[t], minlength=C)
    garc = p_start + np.bincount(g.to, weights=p_edge, minlength=A)
    gtable = np.zeros(C + C * C)
    np.add.at(gtable, lab, p_start)
    np.add.at(gtable, C + lab * C + lab, p_self)
    np.add.at(gtable, C + lab[g.to] * C + lab[g.frm], p_edge)
    return z, grad, garc, gtable


# ---- float32, as the kernel does it ----
def _rounds(count):
    """round k holds the items whose count is above k"""
    for k in range(int(count.max(initial=0))):
        yield k, np.nonzero(count > k)[0]


def lattice_f32(em, table, src, dst, lab, w, K, gw, gtable=None, want_grad=True):
    """(score, gw * d score / d em [T, C], gw * d score / d w [A]) in float32, the kernel's recurrences in its order;
    with `gtable` ([C + C * C], float32) the utterance's table sums are added into it in the table kernel's order"""
    x = np.asarray(em, dtype=np.float32)
    T, C = x.shape
    A = src.size
    g = edges_of(src, dst, K)
    table = np.asarray(table, dtype=np.float32)
    w32 = np.asarray(w, dtype=np.float32)
    zero, neg = np.float32(0), np.float32(NEG)
    with np.errstate(invalid="ignore"):
        wself = table[C + lab * C + lab]
        ew = (w32[g.to] + table[C + lab[g.to] * C + lab[g.frm]]).astype(np.float32)
        first = src == 0
        wstart = np.where(first, w32 + table[lab], neg).astype(np.float32)
        in_rounds = [(sel, g.lo[sel] + k, g.off[sel] + k) for k, sel in _rounds(g.deg)]
        alpha = np.full((T, A), NEG, dtype=np.float32)
        alpha[0] = np.where(first, wstart + x[0, lab], neg)
        for t in range(1, T):
            prev = alpha[t - 1]
            v = prev + wself
            for sel, frm, e in in_rounds:
                v[sel] = logadd32(v[sel], prev[frm] + ew[e])
            alpha[t] = v + x[t, lab]
    score = neg
    for q in g.final:
        score = logadd32(score, alpha[T - 1, q])
    score = np.float32(score)
    if not want_grad or not score > NEG or gw == 0:
        return score, None, None
    gw = np.float32(gw)
    # the arcs leaving the node an arc enters, ascending: round k is the k-th of them
    out_rounds = []
    for k, sel in _rounds(g.odeg[dst]):
        nxt = g.osort[g.olo[dst[sel]] + k]
        out_rounds.append((sel, nxt, table[C + lab[nxt] * C + lab[sel]]))
    # the chains of equal labels, ascending arc index
    chains = collections.OrderedDict()
    for i, v in enumerate(lab.tolist()):
        chains.setdefault(v, []).append(i)
    lists = list(chains.values())
    heads = np.array([c[0] for c in lists], dtype=np.int64)
    head_lab = np.array(list(chains.keys()), dtype=np.int64)
    longest = max(len(c) for c in lists)
    padded = np.full((len(lists), longest), -1, dtype=np.int64)
    for h, c in enumerate(lists):
        padded[h, :len(c)] = c
    chain_rounds = [(np.nonzero(padded[:, r] >= 0)[0], padded[padded[:, r] >= 0, r]) for r in range(1, longest)]
    beta = np.where(dst == K - 1, zero, neg).astype(np.float32)
    grad = np.zeros((T, C), dtype=np.float32)
    cells = np.zeros(g.E, dtype=np.float32)
    sum_self, sum_start = np.zeros(A, dtype=np.float32), np.zeros(A, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T - 1, -1, -1):
            av = alpha[t]
            occ = np.where((av > NEG) & (beta > NEG), np.exp((av + beta) - score, dtype=np.float32), zero)
            mo = (beta + x[t, lab]).astype(np.float32)
            cell = (mo + w32).astype(np.float32)
            live = mo > NEG
            if t == 0:
                xs = wstart + mo
                sum_start = sum_start + np.where(live & (xs > NEG), np.exp(xs - score, dtype=np.float32), zero)
            else:
                ap = alpha[t - 1]
                xs = (ap + wself) + mo
                sum_self = sum_self + np.where(live & (xs > NEG), np.exp(xs - score, dtype=np.float32), zero)
                xe = (ap[g.frm] + ew) + mo[g.to]
                cells = cells + np.where(live[g.to] & (xe > NEG), np.exp(xe - score, dtype=np.float32), zero)
            sums = occ[heads].copy()
            for sel, follower in chain_rounds:
                sums[sel] = sums[sel] + occ[follower]
            grad[t, head_lab] = gw * sums
            nb = mo + wself
            for sel, nxt, tr in out_rounds:
                nb[sel] = logadd32(nb[sel], cell[nxt] + tr)
            beta = nb.astype(np.float32)
    s = sum_start.copy()
    for k, sel in _rounds(g.deg):
        s[sel] = s[sel] + cells[g.off[sel] + k]
    if gtable is not None:
        # a row's order: the arcs ascending, an arc's self sum first, then its edges ascending; the start row: the arcs
        # that leave node 0, ascending (every row has a workgroup of its own; np.add.at adds one element after the other)
        idx = np.empty(A + g.E, dtype=np.int64)
        val = np.empty(A + g.E, dtype=np.float32)
        at_self = np.arange(A) + g.off
        idx[at_self], val[at_self] = C + lab * C + lab, gw * sum_self
        at_edge = np.arange(g.E) + g.to + 1
        idx[at_edge], val[at_edge] = C + lab[g.to] * C + lab[g.frm], gw * cells
        np.add.at(gtable, idx, val)
        np.add.at(gtable, lab[first], (gw * sum_start)[first])
    return score, grad, (gw * s).astype(np.float32)


# ---- a batch, both ways ----
Case = collections.namedtuple("Case", "em trans start arcs num_arcs num_nodes weights frames max_states max_edges gout")
Result = collections.namedtuple("Result", "scores grad garc gtable scores32 grad32 garc32 gtable32")


def max_edges_of(case):
    return case.max_edges if case.max_edges is not None else default_max_edges(case.max_states)


def evaluate(case, f32=True):
    em = case.em
    B, T, C = em.shape
    A = case.arcs.shape[1]
    table = table_of(case.start, case.trans)
    scores = np.full(B, NEG)
    grad, garc, gtable = np.zeros((B, T, C)), np.zeros((B, A)), np.zeros(C + C * C)
    scores32 = np.full(B, NEG, dtype=np.float32)
    grad32, garc32 = np.zeros((B, T, C), dtype=np.float32), np.zeros((B, A), dtype=np.float32)
    gtable32 = np.zeros(C + C * C, dtype=np.float32)
    for b in range(B):
        Tb = T if case.frames is None else int(case.frames[b])
        lat = lattice_for(case, b)
        if lat is None or Tb == 0 or lat[0].size == 0:
            continue
        src, dst, lab, w, K = lat
        x = em[b, :Tb]
        gw = float(np.float32(case.gout[b]))
        z, ge, ga, gt = lattice_fp64(x, case.trans, case.start, src, dst, lab, w, K)
        scores[b] = z
        if ge is not None and gw != 0:
            grad[b, :Tb] = gw * ge
            garc[b, :src.size] = gw * ga
            gtable += gw * gt
        if f32:
            z32, ge32, ga32 = lattice_f32(x, table, src, dst, lab, w, K, gw, gtable32)
            scores32[b] = z32
            if ge32 is not None:
                grad32[b, :Tb] = ge32
                garc32[b, :src.size] = ga32
    return Result(scores, grad, garc, gtable, scores32, grad32, garc32, gtable32)


# ---- the cases ----
ANY = -1  # ctc_lattice_fp's builders leave out a blank: no label is one


def _model(seed, B, T, C, sigma=0.5):
    return model_of(np.random.default_rng(seed), B, T, C, sigma)


def _edges_in(lats):
    return max(edge_count(*(np.asarray(l[0], np.int64).reshape(-1, 3)[:, i] for i in (0, 1)), l[1]) for l in lats)


def _states_case(max_states, sizes, C, seed, T=14, weights=False):
    """one utterance per size K + A; those above max_states score -inf.  max_edges is the largest edge count of those
    within max_states: the bound itself is legal"""
    rng = np.random.default_rng(seed)
    lats = []
    for S in sizes:
        arcs, K = lattice_of_states(rng, S, C, ANY)
        lats.append((arcs, K, rng.normal(0.0, 1.0, len(arcs)).astype(np.float32) if weights else None))
    arcs, na, nn_, w = pack(lats)
    B = len(sizes)
    em, trans, start = _model(seed + 1, B, T, C)
    cap = max(1, _edges_in([l for l, S in zip(lats, sizes) if S <= max_states]))
    return Case(em, trans, start, arcs, na, nn_, w, None, max_states, cap, gout_of(rng, B))


def _sausage_lattices():
    rng = np.random.default_rng(511)
    lats = []
    for last in (510, 509):
        arcs, K = sausage(rng, 8, [511] * 7 + [last], 5, ANY)
        lats.append((arcs, K, rng.normal(0.0, 1.0, len(arcs)).astype(np.float32)))
    return rng, lats


def _sausage_case():
    """9 nodes, 511 parallel arcs on every segment but the last, which has 510 and 509: 4096 and 4095 states, in-degrees
    of 511, 1 827 336 and 1 826 825 edges under max_edges = 2^21"""
    rng, lats = _sausage_lattices()
    arcs, na, nn_, w = pack(lats)
    em, trans, start = _model(512, 2, 10, 5)
    return Case(em, trans, start, arcs, na, nn_, w, None, 4096, MAX_EDGES, gout_of(rng, 2))


def _sausage_capped_case():
    """the second sausage with max_edges one below its edge count: -inf, beside a chain that scores"""
    rng, lats = _sausage_lattices()
    E = _edges_in(lats[1:])
    chain = chain_lattice([1, 2, 2, 4])
    arcs, na, nn_, w = pack([lats[1], (chain[0], chain[1], None)])
    em, trans, start = _model(513, 2, 10, 5)
    return Case(em, trans, start, arcs, na, nn_, w, None, 4096, E - 1, gout_of(rng, 2))


DEEP_T = 350


def _deep_case():
    """1025 nodes, every arc of span 1, 2 and 3 (3069 arcs): the shortest path has 342 arcs, DEEP_T frames"""
    rng = np.random.default_rng(1025)
    K, C = 1025, 37
    arcs = [(s, s + k, 0) for s in range(K) for k in (1, 2, 3) if s + k < K]
    arcs = sort_by_dst(arcs)[0]
    arcs[:, 2] = rng.integers(0, C, len(arcs))
    arcs_p, na, nn_, w = pack([(arcs, K)])
    em, trans, start = _model(1026, 1, DEEP_T, C, sigma=0.3)
    return Case(em, trans, start, arcs_p, na, nn_, w, None, 4096, None, gout_of(rng, 1))


def _indeg_case(C, T, n_units, longest, seed):
    """word-piece lattices: in-degrees 0 .. longest; learned weights on the pieces; the default max_edges"""
    rng = np.random.default_rng(seed)
    lats = []
    for k in range(3):
        arcs, K = decomposition(range(n_units - k), longest, C, ANY, seed + k)
        lats.append((arcs, K, rng.normal(0.0, 1.0, len(arcs)).astype(np.float32)))
    arcs, na, nn_, w = pack(lats)
    S = int((na + nn_).max())
    em, trans, start = _model(seed, 3, T, C)
    return Case(em, trans, start, arcs, na, nn_, w, None, S, None, gout_of(rng, 3))


def _c1_case():
    """C = 1: every neighbour is equal"""
    rng = np.random.default_rng(2)
    lats = [lattice_of_states(rng, S, 1, ANY) for S in (7, 12, 1)]
    arcs, na, nn_, w = pack(lats)
    em, trans, start = _model(3, 3, 20, 1)
    return Case(em, trans, start, arcs, na, nn_, w, None, 16, None, gout_of(rng, 3))


EDGES = cfp.EDGES[:11] + ("one frame fewer than labels", ) + cfp.EDGES[12:14] + (
    "negative num_arcs: one node, no alignment", "weight -inf on the only path", "-inf start entry on the only path",
    "-inf bigram on the only path", "valid: a -inf bigram on one of two paths", "the one-node lattice")
EDGES_C = 7


def _edges_case():
    """ctc_lattice_fp's edges with ASG's meanings (C = 7, T = 9, max_states = 16; EDGES names them): labels 5 and 6 occur
    in the three utterances about -inf table entries only, start[5] and the bigram 6 -> 5 are -inf; utterance 11, a
    chain of six labels, has five frames"""
    c = cfp._edges_case()
    C, T = EDGES_C, c.em.shape[1]
    rng = np.random.default_rng(98)
    arcs, na, nn_, w, gout = c.arcs.copy(), c.num_arcs.copy(), c.num_nodes.copy(), c.weights.copy(), c.gout
    arcs[6, 2, 2] = C  # ("label == C" for this C)
    extra = [(chain_lattice([5, 1])[0], 3), (chain_lattice([6, 5])[0], 3),
             (np.array([(0, 1, 6), (0, 1, 1), (1, 2, 5)], np.int32), 3), (np.zeros((0, 3), np.int32), 1)]
    ea, ena, enn, _ = pack(extra, width=arcs.shape[1])
    arcs, na, nn_ = np.concatenate([arcs, ea]), np.concatenate([na, ena]), np.concatenate([nn_, enn])
    w = np.concatenate([w, rng.normal(0.0, 1.0, (len(extra), w.shape[1])).astype(np.float32)])
    gout = np.concatenate([gout, gout_of(rng, len(extra))])
    B = len(na)
    assert B == len(EDGES)
    em, trans, start = _model(17, B, T, C)
    start[5] = NEG
    trans[5, 6] = NEG
    frames = tuple(5 if b == 11 else T for b in range(B))
    return Case(em, trans, start, arcs, na, nn_, w, frames, 16, None, gout)


RAGGED_FRAMES = cfp.RAGGED_FRAMES


def _ragged_case(pad=np.nan):
    """ctc_lattice_fp's ragged lattices: frame counts from 0 to T, the pad rows filled with `pad`; utterance 6 has one
    frame fewer than its shortest path"""
    c = cfp._ragged_case()
    B, T, C = c.em.shape
    em, trans, start = _model(9, B, T, C)
    em = em.copy()
    for b, f in enumerate(RAGGED_FRAMES):
        em[b, f:] = pad
    return Case(em, trans, start, c.arcs, c.num_arcs, c.num_nodes, c.weights, RAGGED_FRAMES, 32, None, c.gout)


BUILDERS = {
    "s64": lambda: _states_case(64, (1, 63, 64, 65, 3), 5, 64),           # one wave; 65 states are above max_states
    "s65": lambda: _states_case(65, (65, 64, 1), 5, 65, weights=True),    # the first width above a wave
    "s256": lambda: _states_case(256, (255, 256, 257), 5, 256),
    "s257": lambda: _states_case(257, (257, 255, 258), 37, 257, weights=True),  # three arcs per lane
    "s768": lambda: _states_case(768, (768, 513, 769), 37, 768),
    "s769": lambda: _states_case(769, (769, 770), 37, 769),
    "s1024": lambda: _states_case(1024, (1023, 1024, 1025), 37, 1024, weights=True),
    "s1025": lambda: _states_case(1025, (1025, 1026), 37, 1025),          # two arcs per lane
    "s2048": lambda: _states_case(2048, (2048, 2047, 2049), 37, 2048),
    "s2049": lambda: _states_case(2049, (2049, 2050), 37, 2049, weights=True),  # four arcs per lane
    "sausage": _sausage_case,
    "sausage-capped": _sausage_capped_case,
    "deep": _deep_case,
    "indeg8-c37": lambda: _indeg_case(37, 30, 20, 8, 37),
    "c1": _c1_case,
    "c300": lambda: _indeg_case(300, 40, 24, 4, 300),
    "c301": lambda: _indeg_case(301, 24, 16, 4, 301),                     # no multiple of 4 (300 is one)
    "edges": _edges_case,
    "ragged": _ragged_case,
}
ALL_GPU_CASES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def result(name, f32=True):
    """the Result of a named case, computed once per process and left unchanged"""
    return evaluate(case(name), f32)
