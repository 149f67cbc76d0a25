"""The yardstick of the batched ASG Viterbi alignment of token lattices (gtnx_batch_asg_lattice_align,
asg_lattice_align.hip) (TEST INFRASTRUCTURE ONLY).  `align_lattice` is a numpy transcription of the contract (DESIGN
section 39): with float32 every output is the kernel's bit for bit, with float64 the same program is measured against an
enumeration of the lattice's paths in tests/test_asg_lattice_align_cpu.py.  The cases are asg_lattice_fp's; the tie
lattices, their emissions and the no-path fills are ctc_lattice_align_fp's."""
import functools

import numpy as np

import asg_lattice_fp as afp
from asg_score_fp import table_of
from ctc_lattice_align_fp import (Result, TIE_C, TIE_FRAMES, TIE_LATTICES, _plus, default_max_path,  # noqa: F401
                                  no_path, tie_em)
from ctc_lattice_fp import pack, sort_by_dst

NEG = -np.inf


def align_lattice(em, table, lat, T, P, dtype=np.float32):
    """one utterance: em [M, C] (rows from T on are not looked at), table [C + C * C], lat the (src, dst, lab, w, K) of
    asg_lattice_fp.lattice_for or None, P the width of the path rows.  Arithmetic in `dtype`."""
    em = np.asarray(em)
    M, C = em.shape
    T = min(max(int(T), 0), M)
    if lat is None or T == 0 or lat[0].size == 0:
        return no_path(P, M, dtype)
    src, dst, lab, w, K = lat
    x, w = em.astype(dtype), np.asarray(w).astype(dtype)
    table = np.asarray(table).astype(dtype)
    tr = table[C:].reshape(C, C)
    wself = tr[lab, lab]
    nodes = np.arange(K)
    lo, hi = np.searchsorted(dst, nodes, "left"), np.searchsorted(dst, nodes, "right")
    # row a: the arcs entering src a (the node they share), ascending, and their edge weights; -inf behind a row's own
    A = src.size
    deg = hi[src] - lo[src]
    col = np.arange(max(int(deg.max()), 1))[None, :]
    own = col < deg[:, None]
    frm = np.where(own, lo[src][:, None] + col, 0)
    ew = np.where(own, _plus(w[:, None], tr[lab[:, None], lab[frm]]), NEG).astype(dtype)
    alpha = np.where(src == 0, _plus(_plus(w, table[lab]), x[0, lab]), NEG).astype(dtype)
    bp = np.full((T, A), -1, np.int64)
    for t in range(1, T):
        cand = np.concatenate([_plus(alpha, wself)[:, None], _plus(alpha[frm], ew)], axis=1)
        k = np.argmax(cand, axis=1)  # (the first maximum)
        best = cand[np.arange(A), k]
        dead = best == NEG
        bp[t] = np.where(dead, -1, np.where(k == 0, np.arange(A), lo[src] + k - 1))
        with np.errstate(invalid="ignore"):
            alpha = np.where(dead, NEG, best + x[t, lab]).astype(dtype)
    final = np.arange(lo[K - 1], hi[K - 1])
    if final.size == 0 or not alpha[final].max() > NEG:
        return no_path(P, M, dtype)
    a = int(final[np.argmax(alpha[final])])
    score = alpha[a]
    fa = np.full(M, -1, np.int32)
    for t in range(T - 1, -1, -1):
        fa[t] = a
        if t > 0:
            a = int(bp[t, a])
    assert a >= 0 and src[a] == 0
    out = no_path(P, M, dtype)
    heads = [t for t in range(T) if t == 0 or fa[t - 1] != fa[t]]
    for i, (t0, t1) in enumerate(zip(heads[:P], (heads + [T])[1:])):
        a = int(fa[t0])
        out.path_arcs[i], out.path_tokens[i], out.starts[i], out.ends[i] = a, lab[a], t0, t1
        sm = x[t0, lab[a]]
        for t in range(t0 + 1, t1):
            sm = dtype(sm + x[t, lab[a]])
        out.token_scores[i] = sm
    return out._replace(score=dtype(score), path_len=len(heads), frame_arcs=fa)


def rescore64(em, table, lat, path_arcs, starts, ends):
    """the float64 score of a returned (path, spans) under em [T_b, C]; asserts that it is a path with an alignment: the
    arcs consecutive from node 0 to node K - 1, the spans tiling [0, T_b)"""
    src, dst, lab, w, K = lat
    x, tb = np.asarray(em, np.float64), np.asarray(table, np.float64)
    T, C = x.shape
    node, at, total, prev = 0, 0, 0.0, None
    for a, s, e in zip(map(int, path_arcs), map(int, starts), map(int, ends)):
        assert 0 <= a < src.size and src[a] == node and s == at and s < e <= T, (a, s, e)
        v = int(lab[a])
        total += float(w[a]) + (tb[v] if prev is None else tb[C + v * C + prev]) + (e - s - 1) * tb[C + v * C + v]
        total += float(np.sum(x[s:e, v]))
        node, at, prev = int(dst[a]), e, v
    assert node == K - 1 and at == T
    return float(total)


def evaluate(c, P=None, dtype=np.float32):
    """every output of the call on Case c (asg_lattice_fp.Case), widths P and M = T, with its fills"""
    B, M, _ = c.em.shape
    P = default_max_path(c) if P is None else P
    table = table_of(c.start, c.trans)
    out = Result(np.empty(B, dtype), np.empty(B, np.int32), *(np.empty((B, P), np.int32) for _ in range(4)),
                 np.empty((B, P), dtype), np.empty((B, M), np.int32))
    for b in range(B):
        T = M if c.frames is None else int(c.frames[b])
        for field, v in zip(out, align_lattice(c.em[b], table, afp.lattice_for(c, b), T, P, dtype)):
            field[b] = v
    return out


@functools.lru_cache(maxsize=None)
def result(name):  # (the float32 Result of a named case, computed once per process and left unchanged)
    return evaluate(afp.case(name))


def tie_table(seed):
    """integer-valued (trans [C, C], start [C]) of small magnitude: every sum is exact, so ties are real"""
    rng = np.random.default_rng(2000 + seed)
    return rng.integers(-1, 2, (TIE_C, TIE_C)).astype(np.float32), rng.integers(-1, 2, TIE_C).astype(np.float32)


@functools.lru_cache(maxsize=None)
def tie_batch():
    """ctc_lattice_align_fp's tie lattices under its small-integer emissions at every frame count, as one Case"""
    cases = [(sort_by_dst(arcs, w), K, T) for _, arcs, K, w in TIE_LATTICES for T in TIE_FRAMES]
    em = np.stack([tie_em("small", b) for b in range(len(cases))])
    for b, c in enumerate(cases):
        em[b, c[2]:] = np.nan
    arcs, na, nn_, w = pack([(a, K, wt) for (a, wt), K, _ in cases])
    return afp.Case(em, *tie_table(0), arcs, na, nn_, w, tuple(c[2] for c in cases), 16, None, None)


def chain_model():
    """(em [1, 40, 6], trans, start, y int32 [11]): a seeded chain on which the best alignment has no tie"""
    rng = np.random.default_rng(7)
    em, trans, start = afp.model_of(rng, 1, 40, 6)
    return em, trans, start, rng.integers(0, 6, 11).astype(np.int32)
