"""CTC scores of token lattices and their gradients (TEST INFRASTRUCTURE ONLY).

Three things live here, shared by test_ctc_lattice_cpu.py and test_ctc_lattice_gpu.py:
  * the float64 yardstick: a dynamic program over the expanded states of a lattice (one blank state per node, one token
    state per arc) -- score, d score / d emissions by alpha-beta, d score / d arc weights as the arcs' posteriors;
  * a float32 transcription of gtn_amd/csrc/ctc_lattice.hip: the same recurrences with float32 arithmetic in the
    kernel's order (a state's predecessors and successors one after the other, the blank states by lane, xor tree and
    waves, a label's tokens along its chain, an arc's frames descending), so that the float32 error of the METHOD can be
    measured against the gate before a GPU is involved;
  * the generated cases, computed once per process and left unchanged.
The contract: -inf when T_b == 0, num_nodes < 1, nodes + arcs > max_states, an arc with src < 0,
src >= dst or dst >= num_nodes, an arc out of dst order, a label outside 0 .. C - 1, a weight that is +inf or NaN, or no
alignment; a -inf score or a weight g of exactly 0 gives zero gradients.
"""
import collections
import functools

import numpy as np

from ctc_score_fp import NEG, SCORE_GATE, GRAD_GATE, logadd32, score_ok, score_err, grad_err, near_path_case, flat_case
from ctc_beam_fp import continuous_case

__all__ = ["NEG", "SCORE_GATE", "GRAD_GATE", "score_ok", "score_err", "grad_err"]


# ---- the lattice the contract reads out of a row ----
def lattice_of(arcs_row, num_arcs, num_nodes, weights_row, C, max_states):
    """(src, dst, lab, w float64, K), or None when the utterance scores -inf by its lattice alone"""
    width = arcs_row.shape[0]
    A = min(max(int(num_arcs), 0), width)
    K = int(num_nodes)
    if K < 1 or K + A > max_states:
        return None
    a = np.asarray(arcs_row[:A], dtype=np.int64).reshape(A, 3)
    src, dst, lab = a[:, 0], a[:, 1], a[:, 2]
    w = np.zeros(A) if weights_row is None else np.asarray(weights_row[:A], dtype=np.float64)
    if ((src < 0) | (src >= dst) | (dst >= K) | (lab < 0) | (lab >= C)).any():
        return None
    if (np.diff(dst) < 0).any() or np.isnan(w).any() or np.isposinf(w).any():
        return None
    return src, dst, lab, w, K


Expanded = collections.namedtuple("Expanded", "K A S lab final f_to f_from f_arc f_rank b_from b_to b_rank lo hi")


def expand(src, dst, lab, K, blank):
    """The transitions of the alignment graph in the kernel's order.  Forward list: the edges INTO a state -- itself
    (rank 0), for a token the blank of its src (rank 1), then the arcs entering the node in ascending order (a token
    skips those of its own label); f_arc is the arc whose weight the edge pays, -1 for none.  Backward list: the edges OUT
    of a state -- itself, for a token the blank of its dst, then the arcs leaving the node in ascending order."""
    A = src.size
    S = K + A
    nodes = np.arange(K)
    lo, hi = np.searchsorted(dst, nodes, "left"), np.searchsorted(dst, nodes, "right")
    osort = np.argsort(src, kind="stable")
    olo, ohi = np.searchsorted(src[osort], nodes, "left"), np.searchsorted(src[osort], nodes, "right")
    q = np.arange(A)
    f = [(np.arange(S), np.arange(S), np.full(S, -1), np.zeros(S, dtype=np.int64)),
         (K + q, src, q, np.ones(A, dtype=np.int64)),
         (dst, K + q, np.full(A, -1), 1 + q - lo[dst])]
    opos = np.empty(A, dtype=np.int64)
    opos[osort] = np.arange(A) - olo[src[osort]]
    b = [(np.arange(S), np.arange(S), np.zeros(S, dtype=np.int64)),
         (K + q, dst, np.ones(A, dtype=np.int64)),
         (src, K + q, 1 + opos)]
    for n in range(K):
        ins, outs = np.arange(lo[n], hi[n]), osort[olo[n]:ohi[n]]
        if not ins.size or not outs.size:
            continue
        differ = lab[outs][:, None] != lab[ins][None, :]  # [out, in]
        oi, ii = np.nonzero(differ)
        f.append((K + outs[oi], K + ins[ii], outs[oi], 2 + (np.cumsum(differ, axis=1) - 1)[oi, ii]))
        b.append((K + ins[ii], K + outs[oi], 2 + (np.cumsum(differ, axis=0) - 1)[oi, ii]))
    f_to, f_from, f_arc, f_rank = (np.concatenate(x).astype(np.int64) for x in zip(*f))
    b_from, b_to, b_rank = (np.concatenate(x).astype(np.int64) for x in zip(*b))
    labs = np.concatenate([np.full(K, blank, dtype=np.int64), lab])
    final = np.concatenate([[K - 1], K + np.arange(lo[K - 1], hi[K - 1])]).astype(np.int64)
    return Expanded(K, A, S, labs, final, f_to, f_from, f_arc, f_rank, b_from, b_to, b_rank, lo, hi)


def _segments(key, n):
    """(order that sorts the edges by key, the start of every key's run): every key 0 .. n - 1 occurs"""
    order = np.argsort(key, kind="stable")
    return order, np.searchsorted(key[order], np.arange(n))


# ---- float64 ----
def lattice_fp64(em, src, dst, lab, w, K, blank):
    """(score, d score / d em [T, C], d score / d w [A]) of one lattice under em [T, C], float64; the gradients are
    None when the score is -inf"""
    x = np.asarray(em, dtype=np.float64)
    T, C = x.shape
    if T == 0:
        return NEG, None, None
    g = expand(src, dst, lab, K, blank)
    fo, fs = _segments(g.f_to, g.S)
    bo, bs = _segments(g.b_from, g.S)
    wp = np.append(np.asarray(w, dtype=np.float64), 0.0)  # (entry A: no weight)
    few = wp[np.where(g.f_arc >= 0, g.f_arc, g.A)][fo]
    ffrom = g.f_from[fo]
    alpha = np.full((T, g.S), NEG)
    alpha[0, 0] = x[0, blank]
    first = np.nonzero(src == 0)[0]
    alpha[0, K + first] = w[first] + x[0, lab[first]]
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            alpha[t] = np.logaddexp.reduceat(alpha[t - 1][ffrom] + few, fs) + x[t, g.lab]
        alpha[np.isnan(alpha)] = NEG
        z = float(np.logaddexp.reduce(alpha[T - 1, g.final]))
    if not np.isfinite(z):
        return NEG, None, None
    # what an edge pays on entering its target: the target's arc weight unless it is the self-loop
    bto = g.b_to[bo]
    bw = wp[np.where((bto >= K) & (bto != g.b_from[bo]), bto - K, g.A)]
    beta = np.full((T, g.S), NEG)
    beta[T - 1, g.final] = 0.0
    grad = np.zeros((T, C))
    garc = np.zeros(g.A)
    enter = g.f_arc[fo] >= 0
    with np.errstate(invalid="ignore"):
        for t in range(T - 1, 0, -1):
            m = beta[t] + x[t, g.lab]
            v = np.logaddexp.reduceat(m[bto] + bw, bs)
            beta[t - 1] = np.where(np.isnan(v), NEG, v)
            p = np.exp(alpha[t - 1][ffrom[enter]] + few[enter] + m[g.f_to[fo][enter]] - z)
            garc += np.bincount(g.f_arc[fo][enter], weights=np.nan_to_num(p, nan=0.0), minlength=g.A)
        occ = np.nan_to_num(np.exp(alpha + beta - z), nan=0.0)
    garc[first] += occ[0, K + first]
    for t in range(T):
        grad[t] = np.bincount(g.lab, weights=occ[t], minlength=C)
    return z, grad, garc


def paths_of(src, dst, K):
    """every path from node 0 to node K - 1 as a list of arc indices"""
    out = [[] for _ in range(K)]
    for a, s in enumerate(src.tolist()):
        out[s].append(a)
    done, stack = [], [(0, [])]
    while stack:
        n, p = stack.pop()
        if n == K - 1:
            done.append(p)
        for a in out[n]:
            stack.append((int(dst[a]), p + [a]))
    return done


# ---- float32, as the kernel does it ----
def config(max_states):
    """(workgroup width, states per lane): ctc_lattice_config of ctc_lattice.hip"""
    for bound, cfg in ((64, (64, 1)), (256, (256, 1)), (768, (256, 3)), (1024, (1024, 1)), (2048, (1024, 2))):
        if max_states <= bound:
            return cfg
    return 1024, 4


def _plus32(x, w):
    with np.errstate(invalid="ignore"):
        return (np.asarray(x, np.float32) + np.asarray(w, np.float32)).astype(np.float32)


class _Rounds:
    """the edges of a list grouped by rank: round r holds the r-th edge of every state that has one"""

    def __init__(self, key, other, rank, extra):
        order = np.lexsort((key, rank))
        self.key, self.other, self.extra = key[order], other[order], extra[order]
        self.bounds = np.searchsorted(rank[order], np.arange(int(rank.max(initial=-1)) + 2))

    def __iter__(self):
        for r in range(len(self.bounds) - 1):
            sl = slice(self.bounds[r], self.bounds[r + 1])
            yield self.key[sl], self.other[sl], self.extra[sl]


def lattice_f32(em, src, dst, lab, w, K, blank, max_states, gw, want_grad=True):
    """(score, gw * d score / d em [T, C], gw * d score / d w [A]) in float32, the kernel's recurrences in its order"""
    x = np.asarray(em, dtype=np.float32)
    T, C = x.shape
    g = expand(src, dst, lab, K, blank)
    S, A = g.S, g.A
    w32 = np.asarray(w, dtype=np.float32)
    few = np.append(w32, np.float32(0))[np.where(g.f_arc >= 0, g.f_arc, A)]  # (entry A: no weight)
    fwd = _Rounds(g.f_to, g.f_from, g.f_rank, few)
    first = np.nonzero(src == 0)[0]
    alpha = np.full((T, S), NEG, dtype=np.float32)
    alpha[0, 0] = x[0, blank]
    alpha[0, K + first] = _plus32(x[0, lab[first]], w32[first])
    for t in range(1, T):
        v = np.full(S, NEG, dtype=np.float32)
        for to, frm, ew in fwd:
            v[to] = logadd32(v[to], _plus32(alpha[t - 1][frm], ew))
        with np.errstate(invalid="ignore"):
            alpha[t] = np.where(v == NEG, np.float32(NEG), v + x[t, g.lab])
    score = np.float32(NEG)
    for s in g.final:
        score = logadd32(score, alpha[T - 1, s])
    score = np.float32(score)
    if not want_grad or not score > NEG or gw == 0:
        return score, None, None
    WG, PER = config(max_states)
    NW = WG // 64
    gw = np.float32(gw)
    # a successor's cell: a token's holds its weight on top
    bself = g.b_to == g.b_from
    bwd = _Rounds(g.b_from, g.b_to, g.b_rank, bself)
    ent_edges = g.f_rank >= 1
    ent = _Rounds(g.f_to[ent_edges], g.f_from[ent_edges], g.f_rank[ent_edges] - 1, few[ent_edges])
    # the chains of equal labels, ascending arc index
    chains = collections.OrderedDict()
    for i, v in enumerate(lab.tolist()):
        chains.setdefault(v, []).append(i)
    lists = list(chains.values())
    heads = np.array([c[0] for c in lists], dtype=np.int64)
    head_lab = np.array(list(chains.keys()), dtype=np.int64)
    rounds = []
    for r in range(1, max((len(c) for c in lists), default=0)):
        sel = [h for h, c in enumerate(lists) if len(c) > r]
        rounds.append((np.array(sel, dtype=np.int64), np.array([lists[h][r] for h in sel], dtype=np.int64)))
    blank_head = np.nonzero(head_lab == blank)[0]
    lane_idx = np.arange(64)
    wtok = np.concatenate([np.zeros(K, dtype=np.float32), w32])
    beta = np.full(S, NEG, dtype=np.float32)
    beta[g.final] = 0.0
    grad = np.zeros((T, C), dtype=np.float32)
    wacc = np.zeros(A, dtype=np.float32)
    for t in range(T - 1, -1, -1):
        av = alpha[t]
        with np.errstate(invalid="ignore", over="ignore"):
            occ = np.where((av > NEG) & (beta > NEG), np.exp((av + beta) - score, dtype=np.float32), np.float32(0))
            mo = np.where(beta == NEG, np.float32(NEG), beta + x[t, g.lab]).astype(np.float32)
        cell = _plus32(mo, wtok)
        # the blank states: by lane (ascending state), the xor tree of the wave, the waves ascending
        lanes = np.zeros(PER * WG, dtype=np.float32)
        lanes[:K] = occ[:K]
        lanes = lanes.reshape(PER, WG)
        ev = np.zeros(WG, dtype=np.float32)
        for j in range(PER):
            ev = ev + lanes[j]
        v = ev.reshape(NW, 64)
        for off in (32, 16, 8, 4, 2, 1):
            v = v + v[:, lane_idx ^ off]
        evs = v[0, 0]
        for q in range(1, NW):
            evs = np.float32(evs + v[q, 0])
        go = occ[K:]
        if A:
            sums = go[heads].copy()
            if blank_head.size:
                sums[blank_head] = evs + sums[blank_head]
            for sel, follower in rounds:
                sums[sel] = sums[sel] + go[follower]
            grad[t, head_lab] = gw * sums
        if not blank_head.size:
            grad[t, blank] = gw * evs
        # how the frame enters an arc
        if A:
            e = np.full(S, NEG, dtype=np.float32)
            if t == 0:
                e[K + first] = w32[first]
            else:
                for to, frm, ew in ent:
                    e[to] = logadd32(e[to], _plus32(alpha[t - 1][frm], ew))
            et, mt = e[K:], mo[K:]
            with np.errstate(invalid="ignore", over="ignore"):
                wacc = wacc + np.where((et > NEG) & (mt > NEG), np.exp((et + mt) - score, dtype=np.float32), np.float32(0))
        if t == 0:
            break
        nb = np.full(S, NEG, dtype=np.float32)
        for frm, to, is_self in bwd:
            nb[frm] = logadd32(nb[frm], np.where(is_self, mo[to], cell[to]))
        beta = nb
    return score, grad, (gw * wacc).astype(np.float32)


# ---- a batch, both ways ----
Case = collections.namedtuple("Case", "em arcs num_arcs num_nodes weights blank frames max_states gout")
Result = collections.namedtuple("Result", "scores grad garc scores32 grad32 garc32")


def evaluate(case, f32=True):
    em = case.em
    B, T, C = em.shape
    A = case.arcs.shape[1]
    scores = np.full(B, NEG)
    grad, garc = np.zeros((B, T, C)), np.zeros((B, A))
    scores32 = np.full(B, NEG, dtype=np.float32)
    grad32, garc32 = np.zeros((B, T, C), dtype=np.float32), np.zeros((B, A), dtype=np.float32)
    for b in range(B):
        Tb = T if case.frames is None else int(case.frames[b])
        lat = lattice_of(case.arcs[b], case.num_arcs[b], case.num_nodes[b],
                         None if case.weights is None else case.weights[b], C, case.max_states)
        if lat is None or Tb == 0:
            continue
        src, dst, lab, w, K = lat
        x = em[b, :Tb]
        gw = float(np.float32(case.gout[b]))
        z, ge, ga = lattice_fp64(x, src, dst, lab, w, K, case.blank)
        scores[b] = z
        if ge is not None and gw != 0:
            grad[b, :Tb] = gw * ge
            garc[b, :src.size] = gw * ga
        if f32:
            z32, ge32, ga32 = lattice_f32(x, src, dst, lab, w, K, case.blank, case.max_states, gw)
            scores32[b] = z32
            if ge32 is not None:
                grad32[b, :Tb] = ge32
                garc32[b, :src.size] = ga32
    return Result(scores, grad, garc, scores32, grad32, garc32)


# ---- lattices ----
def sort_by_dst(arcs, weights=None):
    arcs = np.asarray(arcs, dtype=np.int32).reshape(-1, 3)
    order = np.argsort(arcs[:, 1], kind="stable")
    return (arcs[order], None if weights is None else np.asarray(weights, np.float32)[order])


def chain_lattice(y):
    y = np.asarray(y, dtype=np.int32)
    n = np.arange(y.size, dtype=np.int32)
    return np.stack([n, n + 1, y], axis=1).reshape(-1, 3), y.size + 1


def random_lattice(rng, K, A, C, blank, max_span=4):
    """K nodes, A >= K - 1 arcs: the chain 0 -> 1 -> .. -> K - 1 and A - K + 1 more of span 1 .. max_span; labels other
    than blank, no two neighbours of the chain alike"""
    labels = np.array([c for c in range(C) if c != blank])
    arcs = []
    prev = -1
    for n in range(K - 1):
        v = labels[rng.integers(labels.size)]
        while labels.size > 1 and v == prev:
            v = labels[rng.integers(labels.size)]
        arcs.append((n, n + 1, v))
        prev = v
    for _ in range(A - (K - 1)):
        s = int(rng.integers(0, K - 1))
        d = min(K - 1, s + int(rng.integers(1, max_span + 1)))
        arcs.append((s, d, labels[rng.integers(labels.size)]))
    return sort_by_dst(arcs)[0], K


def lattice_of_states(rng, S, C, blank):
    """a random lattice with K + A == S states; beyond a wave's worth the nodes stay few, so that few frames suffice"""
    if S == 1:
        return np.zeros((0, 3), dtype=np.int32), 1
    K = max(2, min(S // 3, 12))
    return random_lattice(rng, K, S - K, C, blank)


def sausage(rng, segments, widths, C, blank):
    """segments + 1 nodes, widths[i] parallel arcs from node i to node i + 1"""
    labels = np.array([c for c in range(C) if c != blank])
    arcs = [(i, i + 1, labels[rng.integers(labels.size)]) for i in range(segments) for _ in range(widths[i])]
    return sort_by_dst(arcs)[0], segments + 1


def pack(lattices, width=None):
    """(arcs [B, A, 3], num_arcs, num_nodes, weights [B, A] or None) of (arcs, K[, weights]) tuples; rows past the
    counts hold valid-looking arcs of label 0 (they would count if read)"""
    B = len(lattices)
    A = max([1] + [len(l[0]) for l in lattices]) if width is None else width
    arcs = np.zeros((B, A, 3), dtype=np.int32)
    arcs[:, :, 1] = 1
    has_w = any(len(l) > 2 and l[2] is not None for l in lattices)
    weights = np.zeros((B, A), dtype=np.float32) if has_w else None
    num_arcs, num_nodes = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b, l in enumerate(lattices):
        n = len(l[0])
        arcs[b, :n] = l[0]
        num_arcs[b], num_nodes[b] = n, l[1]
        if has_w and len(l) > 2 and l[2] is not None:
            weights[b, :n] = l[2]
    return arcs, num_arcs, num_nodes, weights


def gout_of(rng, B):
    return rng.uniform(-1.0, 1.0, B).astype(np.float32)


def min_frames(src, dst, lab, K):
    """the fewest frames an alignment of the lattice takes: a path's arcs plus a blank between equal neighbours"""
    best = {}
    for a in np.argsort(dst, kind="stable").tolist():
        s = int(src[a])
        cands = [1] if s == 0 else []
        for p, (d, l) in enumerate(zip(dst.tolist(), lab.tolist())):
            if d == s and p in best:
                cands.append(best[p] + (2 if l == lab[a] else 1))
        if cands:
            best[a] = min(cands)
    ends = [best[a] for a in best if dst[a] == K - 1]
    return min(ends) if ends else None


# ---- the cases ----
def _states_case(max_states, sizes, C, blank, seed, T=14, weights=False):
    """one utterance per size K + A; those above max_states score -inf"""
    rng = np.random.default_rng(seed)
    lats = []
    for S in sizes:
        arcs, K = lattice_of_states(rng, S, C, blank)
        w = rng.normal(0.0, 1.0, len(arcs)).astype(np.float32) if weights else None
        lats.append((arcs, K, w))
    arcs, na, nn_, w = pack(lats)
    B = len(sizes)
    return Case(flat_case(seed + 1, B, T, C), arcs, na, nn_, w, blank, None, max_states, gout_of(rng, B))


def _sausage_case():
    """9 nodes, 511 parallel arcs on every segment but the last, which has 510 and 509: 4096 and 4095 states, in-degrees
    of 511 (nine nodes with 511 arcs on all eight segments would be 4097 states, one above the largest max_states)"""
    rng = np.random.default_rng(511)
    C, blank, T = 5, 0, 10
    lats = []
    for last in (510, 509):
        arcs, K = sausage(rng, 8, [511] * 7 + [last], C, blank)
        lats.append((arcs, K, rng.normal(0.0, 1.0, len(arcs)).astype(np.float32)))
    arcs, na, nn_, w = pack(lats)
    return Case(flat_case(512, 2, T, C), arcs, na, nn_, w, blank, None, 4096, gout_of(rng, 2))


def _deep_case():
    """1025 nodes, every arc of span 1, 2 and 3 (3069 arcs), 360 frames peaked along the path of span-3 arcs"""
    rng = np.random.default_rng(1025)
    K, C, blank, T = 1025, 37, 0, 360
    arcs = [(s, s + k, 0) for s in range(K) for k in (1, 2, 3) if s + k < K]
    arcs = sort_by_dst(arcs)[0]
    arcs[:, 2] = rng.integers(1, C, len(arcs))
    path = [a for a in range(len(arcs)) if arcs[a, 0] % 3 == 0 and (arcs[a, 1] - arcs[a, 0] == 3 or arcs[a, 1] == K - 1
                                                                     and arcs[a, 0] == K - 2)]
    for i in range(1, len(path)):
        while arcs[path[i], 2] == arcs[path[i - 1], 2]:
            arcs[path[i], 2] = rng.integers(1, C)
    y = arcs[path, 2]
    em = near_path_case(1026, [y], T, C, blank, peak=10.0)
    arcs_p, na, nn_, w = pack([(arcs, K)])
    return Case(em, arcs_p, na, nn_, w, blank, None, 4096, gout_of(rng, 1))


def the_pieces():
    return {"e": 0, "h": 1, "t": 2, "th": 3, "he": 4, "the": 5}


def decomposition(units, longest, C, blank, seed):
    """every piece of up to `longest` units: the arc (i, j) for 0 < j - i <= longest, labels other than blank"""
    rng = np.random.default_rng(seed)
    n = len(units)
    arcs = [(i, j, 0) for j in range(1, n + 1) for i in range(max(0, j - longest), j)]
    arcs = sort_by_dst(arcs)[0]
    labels = np.array([c for c in range(C) if c != blank])
    arcs[:, 2] = labels[rng.integers(0, labels.size, len(arcs))]
    return arcs, n + 1


def _indeg_case(C, blank, T, n_units, longest, seed):
    """word-piece lattices: in-degrees 0 .. longest; learned weights on the pieces"""
    rng = np.random.default_rng(seed)
    lats = []
    for k in range(3):
        arcs, K = decomposition(range(n_units - k), longest, C, blank, seed + k)
        lats.append((arcs, K, rng.normal(0.0, 1.0, len(arcs)).astype(np.float32)))
    arcs, na, nn_, w = pack(lats)
    S = int((na + nn_).max())
    return Case(continuous_case(seed, 3, T, C), arcs, na, nn_, w, blank, None, S, gout_of(rng, 3))


def _c2_case():
    """C = 2: every token carries the one label, so no token follows a token without a blank between"""
    rng = np.random.default_rng(2)
    lats = [lattice_of_states(rng, S, 2, 0) for S in (7, 12, 1)]
    arcs, na, nn_, w = pack(lats)
    return Case(continuous_case(3, 3, 30, 2), arcs, na, nn_, w, 0, None, 16, gout_of(rng, 3))


EDGES = ("valid: parallel and consecutive equal labels", "num_nodes 0", "src < 0", "src >= dst", "dst >= K",
         "out of dst order", "label == C", "label < 0", "weight +inf", "weight NaN",
         "valid: -inf weight, a label equal to blank, a dead end, an unreachable node", "no alignment fits",
         "above max_states", "num_arcs above the width", "negative num_arcs", "weight -inf on the only path")


def _edges_case():
    """C = 5, blank = 2, T = 9, max_states = 16: the contract's edges one per utterance (EDGES names them)"""
    C, blank, T = 5, 2, 9
    rng = np.random.default_rng(99)
    base = [(0, 1, 1), (0, 1, 1), (0, 1, 3), (1, 2, 1), (1, 2, 4), (0, 2, 0), (2, 3, 4), (2, 3, 4)]
    w0 = rng.normal(0.0, 1.0, len(base)).astype(np.float32)

    def variant(i, *changes):
        a = np.array(base, dtype=np.int32)
        for field, value in zip(changes[0::2], changes[1::2]):
            a[i, field] = value
        return a

    def weighted(i, value):
        w = w0.copy()
        w[i] = value
        return w
    odd = [(0, 1, 1), (0, 2, 2), (1, 2, 3), (1, 3, 4), (0, 5, 1), (4, 5, 3), (2, 5, 0)]  # 3: a dead end; 4: unreachable
    wodd = rng.normal(0.0, 1.0, len(odd)).astype(np.float32)
    wodd[2] = NEG
    long_chain = chain_lattice([1, 1, 1, 1, 1, 3])[0]  # needs 10 frames
    lats = [(np.array(base, np.int32), 4, w0), (np.array(base, np.int32), 0, w0), (variant(3, 0, -1), 4, w0),
            (variant(3, 0, 2), 4, w0), (variant(7, 1, 4), 4, w0), (variant(6, 0, 0, 1, 1), 4, w0), (variant(2, 2, C), 4, w0),
            (variant(2, 2, -1), 4, w0), (np.array(base, np.int32), 4, weighted(1, np.inf)),
            (np.array(base, np.int32), 4, weighted(6, np.nan)), (np.array(odd, np.int32), 6, wodd),
            (long_chain, 7, None), (random_lattice(rng, 5, 12, C, blank)[0], 5, None),
            (np.array(base, np.int32), 4, w0), (np.array(base, np.int32), 1, w0),
            (chain_lattice([1, 3])[0], 3, np.array([0.5, NEG], np.float32))]
    arcs, na, nn_, w = pack(lats, width=12)
    na[13] = 100  # (the width counts: the four rows behind the eight arcs are read -- make them arcs of the lattice)
    arcs[13, 8:] = [(2, 3, 1), (2, 3, 0), (1, 3, 3), (0, 3, 4)]
    na[14] = -3   # (no arc: the one node's blank alone)
    gout = gout_of(rng, len(lats))
    gout[0] = 0.0
    gout[1] = 0.0  # an exact 0 on a finite score and on a -inf one
    return Case(continuous_case(17, len(lats), T, C), arcs, na, nn_, w, blank, None, 16, gout)


RAGGED_FRAMES = (40, 1, 0, 39, 33, 2, 5)


def _ragged_case(pad=np.nan):
    """frame counts from 0 to T, the pad rows filled with `pad`; utterance 6 has one frame fewer than its shortest path"""
    rng = np.random.default_rng(77)
    B, T, C, blank = 7, 40, 5, 4
    em = continuous_case(9, B, T, C).copy()
    for b, f in enumerate(RAGGED_FRAMES):
        em[b, f:] = pad
    lats = [lattice_of_states(rng, S, C, blank) for S in (20, 3, 9, 30, 25, 5)]
    lats[1] = (np.array([(0, 1, 1), (0, 1, 2)], np.int32), 2)  # one frame: one arc fits
    lats[5] = (np.array([(0, 1, 1), (1, 2, 2), (0, 2, 3)], np.int32), 3)
    lats.append(chain_lattice([0, 1, 2, 3, 0, 1]))  # six frames at least
    arcs, na, nn_, w = pack(lats)
    return Case(em, arcs, na, nn_, w, blank, RAGGED_FRAMES, 32, gout_of(rng, B))


def _c256_case():
    return _indeg_case(256, 0, 40, 24, 4, 256)


BUILDERS = {
    "s64": lambda: _states_case(64, (1, 63, 64, 65, 3), 5, 0, 64),          # one wave; 65 states are above max_states
    "s65": lambda: _states_case(65, (65, 64, 1), 5, 0, 65, weights=True),   # the first width above a wave
    "s256": lambda: _states_case(256, (255, 256, 257), 5, 0, 256),
    "s257": lambda: _states_case(257, (257, 255), 37, 36, 257, weights=True),  # three states per lane
    "s768": lambda: _states_case(768, (768, 513), 37, 0, 768),
    "s769": lambda: _states_case(769, (769,), 37, 0, 769),
    "s1024": lambda: _states_case(1024, (1023, 1024, 1025), 37, 0, 1024, weights=True),
    "s1025": lambda: _states_case(1025, (1025,), 37, 0, 1025),              # two states per lane
    "s2048": lambda: _states_case(2048, (2048, 2047), 37, 0, 2048),
    "s2049": lambda: _states_case(2049, (2049,), 37, 0, 2049, weights=True),  # four states per lane
    "sausage": _sausage_case,
    "deep": _deep_case,
    "indeg8-c37": lambda: _indeg_case(37, 0, 30, 20, 8, 37),
    "c2": _c2_case,
    "c256": _c256_case,
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
