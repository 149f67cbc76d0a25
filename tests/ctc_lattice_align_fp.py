"""The yardstick of the batched CTC Viterbi alignment of token lattices (gtnx_batch_ctc_lattice_align,
ctc_lattice_align.hip) and its cases (TEST INFRASTRUCTURE ONLY).

`align_lattice` is a numpy transcription of the contract: the states of ctc_lattice_fp.expand (one
blank state per node, one token state per arc), a state's candidates in the order of `f_rank` -- itself, for a token the
blank of its src, then the arcs that enter the node in ascending order (a token skips those of its own label) -- the exact
maximum, and of the candidates that reach it the FIRST: a later one replaces it only if strictly greater, a -inf candidate
is never chosen.  With dtype float32 every output is the kernel's bit for bit, so the GPU tests compare bits and there is
no tolerance; with float64 the same program is the yardstick the float32 one is measured against.  `rescore64` scores a
returned (path, alignment) on its own in float64 and checks that it is one.  tests/test_ctc_lattice_align_cpu.py pins
this file to an enumeration of the lattice's paths, to the oracle's viterbi score of the alignment graph and to
ctc_token_align_fp on chains."""
import collections
import functools

import numpy as np

from ctc_lattice_fp import (ALL_GPU_CASES, Case, EDGES, RAGGED_FRAMES, case, chain_lattice, decomposition, expand,  # noqa: F401
                            lattice_of, min_frames, pack, paths_of, random_lattice, sausage, sort_by_dst)
from ctc_score_fp import SCORE_GATE  # noqa: F401

NEG = -np.inf

Out = collections.namedtuple("Out", "score path_len path_arcs path_tokens starts ends token_scores frame_arcs")


def no_path(P, M, dtype=np.float32):
    fill = np.full(P, -1, np.int32)
    return Out(dtype(NEG), 0, fill, fill.copy(), fill.copy(), fill.copy(), np.full(P, NEG, dtype), np.full(M, -1, np.int32))


def _plus(x, w):
    """the kernel's plus(): -inf when either operand is"""
    with np.errstate(invalid="ignore"):
        return np.where((x == NEG) | (w == NEG), NEG, x + w).astype(x.dtype)


def align_lattice(em, lat, blank, T, P, dtype=np.float32):
    """one utterance: em [M, C] (rows from T on are not looked at), lat the (src, dst, lab, w, K) of lattice_of or None,
    P the width of the path rows.  Arithmetic in `dtype`."""
    em = np.asarray(em)
    M = em.shape[0]
    T = min(max(int(T), 0), M)
    dead = no_path(P, M, dtype)
    if lat is None or T == 0:
        return dead
    src, dst, lab, w, K = lat
    x = em.astype(dtype)
    w = np.asarray(w).astype(dtype)
    wp = np.append(w, dtype(0))  # (entry -1: no weight)
    g = expand(src, dst, lab, K, blank)
    S = g.S
    # the edges by rank: round r holds the r-th candidate of every state that has one
    order = np.lexsort((g.f_to, g.f_rank))
    to, frm, arc = g.f_to[order], g.f_from[order], g.f_arc[order]
    bounds = np.searchsorted(g.f_rank[order], np.arange(int(g.f_rank.max()) + 2))
    alpha = np.full(S, NEG, dtype=dtype)
    alpha[0] = x[0, blank]
    first = np.nonzero(src == 0)[0]
    alpha[K + first] = _plus(x[0, lab[first]], w[first])
    bp = np.full((T, S), -1, dtype=np.int64)
    for t in range(1, T):
        best = np.full(S, NEG, dtype=dtype)
        for r in range(len(bounds) - 1):
            sl = slice(bounds[r], bounds[r + 1])
            a = arc[sl]
            cand = alpha[frm[sl]]
            pay = a >= 0
            cand = np.where(pay, _plus(cand, wp[a]), cand).astype(dtype)  # (a candidate that pays nothing adds nothing)
            with np.errstate(invalid="ignore"):
                win = cand > best[to[sl]]  # (strictly greater: the first maximum stays; -inf is never chosen)
            best[to[sl][win]] = cand[win]
            bp[t, to[sl][win]] = frm[sl][win]
        with np.errstate(invalid="ignore"):
            alpha = np.where(best == NEG, NEG, best + x[t, g.lab]).astype(dtype)
    score, end = dtype(NEG), -1
    for s in g.final:
        if alpha[s] > score:
            score, end = alpha[s], int(s)
    if not score > NEG:
        return dead
    fa = np.full(M, -1, np.int32)
    s = end
    for t in range(T - 1, -1, -1):
        fa[t] = s - K if s >= K else -1
        if t > 0:
            s = int(bp[t, s])
            assert s >= 0
    assert s == 0 or (s >= K and src[s - K] == 0)
    out = no_path(P, M, dtype)
    on = fa[:T]
    heads = [t for t in range(T) if on[t] >= 0 and (t == 0 or on[t - 1] != on[t])]
    for i, t0 in enumerate(heads[:P]):
        a = int(on[t0])
        t1 = t0
        while t1 < T and on[t1] == a:
            t1 += 1
        out.path_arcs[i], out.path_tokens[i], out.starts[i], out.ends[i] = a, lab[a], t0, t1
        sm = x[t0, lab[a]]
        for t in range(t0 + 1, t1):
            sm = dtype(sm + x[t, lab[a]])
        out.token_scores[i] = sm
    return out._replace(score=dtype(score), path_len=len(heads), frame_arcs=fa)


def rescore64(em, lattice, path_arcs, starts, ends, blank):
    """the float64 score of a returned (path, alignment) under em [T_b, C]: the arcs' weights, the arcs' labels over their
    spans, `blank` on every other frame.  Asserts that it is a path with an alignment: the arcs consecutive from node 0
    to node K - 1, the spans ordered, disjoint and inside [0, T_b), equal neighbouring labels parted by a blank frame."""
    src, dst, lab, w, K = lattice
    x = np.asarray(em, dtype=np.float64)
    T = x.shape[0]
    n = len(path_arcs)
    assert len(starts) == n and len(ends) == n
    node, at = 0, 0
    total = 0.0
    covered = np.zeros(T, dtype=bool)
    for i in range(n):
        a = int(path_arcs[i])
        assert 0 <= a < len(src) and src[a] == node, (i, a)
        node = int(dst[a])
        s, e = int(starts[i]), int(ends[i])
        assert at <= s < e <= T, (i, s, e)
        if i > 0 and lab[a] == lab[int(path_arcs[i - 1])]:
            assert s > at, "equal neighbouring labels need a blank frame between"
        at = e
        covered[s:e] = True
        total += float(w[a]) + float(np.sum(x[s:e, lab[a]]))
    assert node == K - 1
    return total + float(np.sum(x[~covered, blank]))


# ---- a batch ----
Result = collections.namedtuple("Result", "scores path_len path_arcs path_tokens starts ends token_scores frame_arcs")


def default_max_path(c):
    return max(1, min(c.arcs.shape[1], c.max_states))


def evaluate(c, P=None, dtype=np.float32):
    """every output of the call on Case c (ctc_lattice_fp.Case), widths P and M = T"""
    B, M, C = c.em.shape
    P = default_max_path(c) if P is None else P
    out = Result(np.empty(B, dtype), np.empty(B, np.int32), *(np.empty((B, P), np.int32) for _ in range(4)),
                 np.empty((B, P), dtype), np.empty((B, M), np.int32))
    for b in range(B):
        T = M if c.frames is None else int(c.frames[b])
        lat = lattice_of(c.arcs[b], c.num_arcs[b], c.num_nodes[b], None if c.weights is None else c.weights[b], C,
                         c.max_states)
        r = align_lattice(c.em[b], lat, c.blank, T, P, dtype)
        for field, v in zip(out, r):
            field[b] = v
    return out


@functools.lru_cache(maxsize=None)
def result(name):
    """the float32 Result of a named case of ctc_lattice_fp, computed once per process and left unchanged"""
    return evaluate(case(name))


@functools.lru_cache(maxsize=None)
def result64(name):
    return evaluate(case(name), dtype=np.float64)


# ---- tie cases: small lattices under emissions and weights whose sums are exact, so ties are real ----
TIE_C, TIE_BLANK = 4, 0
# (name, arcs (src, dst, label), nodes, integer weights or None)
TIE_LATTICES = [
    ("one node", [], 1, None),
    ("one arc", [(0, 1, 1)], 2, None),
    ("parallel arcs of equal label", [(0, 1, 1), (0, 1, 1), (1, 2, 2), (1, 2, 2)], 3, [0, 0, 1, 1]),
    ("parallel arcs of different labels", [(0, 1, 1), (0, 1, 2), (0, 1, 3), (1, 2, 3), (1, 2, 1)], 3, [1, 1, 0, -1, 0]),
    ("consecutive equal labels", [(0, 1, 1), (1, 2, 1), (1, 2, 2), (2, 3, 1), (2, 3, 2)], 4, [0, 1, 0, 0, 1]),
    ("a label equal to blank", [(0, 1, 0), (0, 1, 2), (1, 2, 0), (1, 2, 2), (0, 2, 1)], 3, [0, 0, 1, 0, 1]),
    ("a dead end", [(0, 1, 1), (0, 2, 2), (1, 3, 2), (1, 4, 1), (0, 4, 2), (2, 3, 3)], 5, [2, 0, 0, -1, 0, 0]),
    ("a -inf weight", [(0, 1, 1), (0, 1, 2), (1, 2, 1), (1, 2, 2)], 3, [0, NEG, 1, NEG]),
    ("a diamond of decompositions", [(0, 1, 2), (0, 2, 1), (1, 2, 1), (0, 3, 2), (1, 3, 1), (2, 3, 2)], 4,
     [0, 1, 1, 2, 1, 0]),
    ("six nodes, spans 1 and 2", [(s, s + k, 1 + (s + k) % 3) for s in range(6) for k in (1, 2) if s + k < 6], 6, None),
]
TIE_EMISSIONS = ("zero", "bits", "small")  # all zero | {0, 1} | {-2 .. 2}
TIE_FRAMES = (1, 2, 3, 5, 9)
TIE_T = max(TIE_FRAMES)


def tie_em(kind, seed, T=TIE_T, C=TIE_C):
    rng = np.random.default_rng(1000 + seed)
    if kind == "zero":
        return np.zeros((T, C), np.float32)
    if kind == "bits":
        return rng.integers(0, 2, (T, C)).astype(np.float32)
    return rng.integers(-2, 3, (T, C)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def tie_cases():
    """[(name, em [TIE_T, C], frames, arcs, K, weights or None)]: every lattice under every kind of emission, frame
    count and weighting (zeros, and the lattice's own small integers)"""
    out = []
    for li, (name, arcs, K, weights) in enumerate(TIE_LATTICES):
        for ki, kind in enumerate(TIE_EMISSIONS):
            for T in TIE_FRAMES:
                for wsel in ((None,) if weights is None else (None, weights)):
                    a, w = sort_by_dst(arcs, wsel)
                    out.append((f"{name} / {kind} / T {T} / {'weights' if wsel else 'no weights'}",
                                tie_em(kind, 31 * li + 7 * ki + T), T, a, K, w))
    return out


@functools.lru_cache(maxsize=None)
def tie_batch():
    """the tie cases as one Case: ragged frame counts, NaN behind them"""
    cases = tie_cases()
    em = np.stack([c[1] for c in cases]).copy()
    frames = tuple(c[2] for c in cases)
    for b, f in enumerate(frames):
        em[b, f:] = np.nan
    arcs, na, nn_, w = pack([(c[3], c[4], c[5]) for c in cases])
    return Case(em, arcs, na, nn_, w, TIE_BLANK, frames, 16, None)


@functools.lru_cache(maxsize=None)
def tie_result():
    return evaluate(tie_batch())
