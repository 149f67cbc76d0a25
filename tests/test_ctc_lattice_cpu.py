"""CTC scores of token lattices, the parts that need no GPU.  The float64 yardstick of tests/ctc_lattice_fp.py (which
test_ctc_lattice_gpu.py judges the kernels by) is pinned twice on small lattices: to the enumeration of the lattice's
paths -- logsumexp of w(p) + ctc_score_fp.pair_fp64(em, labels(p)), its gradients the softmax-weighted sums (1e-9) -- and
to the oracle's forwardScore of the alignment graph built arc by arc (1e-4 max(1, |score|), the bound the CPU tests give
that float32 oracle).  A chain lattice is ctc_score, and its loss ctc_loss_fp64 (1e-12).  The float32 transcription of
the kernel stays inside the gate on every case the GPU file runs, the cases sit at the kernel's edges, the builders build
what they say, and the entry points exist in every layer, refuse bad arguments before they ask for a device, and fail
loudly without one."""
import ctypes
import os

import numpy as np
import pytest

import ctc_beam_fp as bfp
import ctc_lattice_fp as fp
import ctc_score_fp as sfp
from conftest import ROOT, has_gpu
from ctc_fp64 import _lse, ctc_loss_fp64
from oracle_lib import OGraph, lib as oracle

NEG = -np.inf

# small lattices: (name, arcs (src, dst, label), nodes, weights or None); labels below C = 3 or 4
A1, A2 = 1, 2
SMALL_LATTICES = [
    ("parallel arcs of equal label", [(0, 1, A1), (0, 1, A1), (1, 2, A2), (0, 2, A2)], 3, [0.3, -0.7, 0.1, 0.4]),
    ("consecutive arcs of equal label", [(0, 1, A1), (1, 2, A1), (1, 2, A2), (2, 3, A1)], 4, None),
    ("a label equal to blank", [(0, 1, 0), (0, 1, 2), (1, 2, 0), (1, 2, 2), (0, 2, 1)], 3, [0.2, 0.0, -0.4, 0.9, -1.0]),
    ("a dead-end arc", [(0, 1, A1), (0, 2, A2), (1, 3, A2), (1, 4, A1), (0, 4, A2)], 5, None),  # nodes 2 and 3 lead nowhere
    ("an unreachable node", [(0, 1, A1), (2, 3, A2), (1, 3, A2), (0, 3, A1)], 4, [0.5, 0.25, -0.5, 0.0]),
    ("a -inf weight", [(0, 1, A1), (0, 1, A2), (1, 2, A1), (1, 2, A2)], 3, [0.1, NEG, -0.2, 0.3]),
    ("the empty lattice", [], 1, None),
    ("a diamond of decompositions", [(0, 1, A2), (0, 2, A1), (1, 2, A1), (0, 3, A2), (1, 3, A1), (2, 3, A2)], 4,
     [0.1, 0.2, -0.3, 0.4, 0.0, -0.6]),
]
SMALL_EMS = [("continuous", 0, 1, 3), ("continuous", 1, 3, 3), ("holes", 2, 4, 3), ("integer", 3, 5, 4),
             ("continuous", 4, 6, 3), ("holes", 5, 6, 4)]


def small_em(kind, seed, T, C):
    make = {"continuous": bfp.continuous_case, "holes": bfp.holes_case, "integer": bfp.integer_case}[kind]
    return make(200 + seed, 1, T, C)[0]


def lattice_arrays(arcs, weights):
    a, w = fp.sort_by_dst(arcs, weights)
    a = a.astype(np.int64)
    return a[:, 0], a[:, 1], a[:, 2], (np.zeros(len(a)) if w is None else w.astype(np.float64))


def by_enumeration(em, src, dst, lab, w, K, blank):
    """(score, d / d em, d / d w) as the sum over the lattice's paths of ctc_score's yardstick"""
    paths = fp.paths_of(src, dst, K)
    assert len(paths) <= 400
    terms = []
    for p in paths:
        z, g = sfp.pair_fp64(em, lab[p], blank)
        terms.append((float(np.sum(w[p])) + z if np.isfinite(z) else NEG, g, p))
    zs = np.array([t[0] for t in terms] or [NEG])
    total = float(_lse(zs)) if np.isfinite(zs).any() else NEG
    if not np.isfinite(total):
        return NEG, None, None
    grad, garc = np.zeros(em.shape), np.zeros(len(src))
    for z, g, p in terms:
        if np.isfinite(z):
            grad += np.exp(z - total) * g
            np.add.at(garc, p, np.exp(z - total))  # (an arc counts once per use)
    return total, grad, garc


@pytest.mark.parametrize("kind,seed,T,C", SMALL_EMS)
@pytest.mark.parametrize("which", range(len(SMALL_LATTICES)))
@pytest.mark.parametrize("blank", ["first", "last"])
def test_yardstick_is_the_enumeration(kind, seed, T, C, which, blank):
    name, arcs, K, weights = SMALL_LATTICES[which]
    em = small_em(kind, seed, T, C)
    src, dst, lab, w = lattice_arrays(arcs, weights)
    if blank == "last":  # (the lattices are written for blank 0: turn the labels round)
        lab = (C - 1) - np.minimum(lab, C - 1)
        blank = C - 1
    else:
        blank = 0
    want = by_enumeration(em, src, dst, lab, w, K, blank)
    got = fp.lattice_fp64(em, src, dst, lab, w, K, blank)
    if np.isfinite(want[0]):
        assert abs(got[0] - want[0]) <= 1e-9, (name, got[0], want[0])
        np.testing.assert_allclose(got[1], want[1], rtol=0, atol=1e-9)
        np.testing.assert_allclose(got[2], want[2], rtol=0, atol=1e-9)
    else:
        assert got[0] == NEG and got[1] is None and got[2] is None, (name, got[0])


@pytest.mark.parametrize("kind,seed,T,C", SMALL_EMS)
@pytest.mark.parametrize("which", range(len(SMALL_LATTICES)))
def test_yardstick_is_the_oracle(kind, seed, T, C, which):
    """forwardScore of the lattice's CTC alignment graph, built arc by arc, intersected with linearGraph(T, C) (float32)"""
    name, arcs, K, weights = SMALL_LATTICES[which]
    em = small_em(kind, seed, T, C)
    src, dst, lab, w = lattice_arrays(arcs, weights)
    w = np.where(np.isfinite(w), w, -1e30)  # (the float32 oracle adds weights: a very low one stands in for -inf)
    for blank in (0, C - 1):
        L = oracle()
        g = OGraph()
        A = len(src)
        # the one start node is blank(0): frame 0 takes its self-loop or an arc into a token that leaves node 0
        for n in range(K):
            L.og_add_node(g.h, int(n == 0), int(n == K - 1))
        for a in range(A):
            L.og_add_node(g.h, 0, int(dst[a] == K - 1))
        for n in range(K):
            L.og_add_arc(g.h, n, n, blank, blank, 0.0)
        for a in range(A):
            s, l, wa = K + a, int(lab[a]), float(w[a])
            L.og_add_arc(g.h, s, s, l, l, 0.0)
            L.og_add_arc(g.h, int(src[a]), s, l, l, wa)
            L.og_add_arc(g.h, s, int(dst[a]), blank, blank, 0.0)
            for a2 in range(A):
                if dst[a2] == src[a] and lab[a2] != lab[a]:
                    L.og_add_arc(g.h, K + a2, s, l, l, wa)
        want = g.compose(OGraph.linear(T, C, em), "intersect").shortest_distance(tropical=False)
        wf = np.where(w < -1e29, NEG, w)
        got = fp.lattice_fp64(em, src, dst, lab, wf, K, blank)[0]
        if want is None or not np.isfinite(want) or want < -1e29:
            assert got == NEG, (name, got, want)
        else:
            assert abs(got - want) <= 1e-4 * max(1.0, abs(want)), (name, blank, got, want)


@pytest.mark.parametrize("kind,seed,T,C", SMALL_EMS + [("continuous", 7, 12, 5)])
def test_a_chain_is_ctc_score_and_its_loss_ctc_loss(kind, seed, T, C):
    em = small_em(kind, seed, T, C)
    rng = np.random.default_rng(seed)
    rows = _lse(em.astype(np.float64), axis=1)
    for n in range(0, T + 1):
        y = rng.integers(1, C, n)
        arcs, K = fp.chain_lattice(y)
        src, dst, lab, w = lattice_arrays(arcs, None)
        z, g, ga = fp.lattice_fp64(em, src, dst, lab, w, K, 0)
        want, gw = sfp.pair_fp64(em, y, 0)
        loss, gloss, _ = ctc_loss_fp64(em, y, 0)
        if np.isfinite(want):
            assert abs(z - want) <= 1e-12 * max(1.0, abs(want)), (n, z, want)
            np.testing.assert_allclose(g, gw, rtol=0, atol=1e-12)
            np.testing.assert_allclose(ga, np.ones(n), rtol=0, atol=1e-9)  # (every arc of a chain is used)
            assert abs((np.sum(rows) - z) - loss) <= 1e-12 * max(1.0, abs(loss)), (n, z, loss)
            np.testing.assert_allclose(np.exp(em.astype(np.float64) - rows[:, None]) - g, gloss, rtol=0, atol=1e-12)
        else:
            assert z == NEG and g is None and not np.isfinite(loss)


def test_every_invalid_lattice_gives_minus_infinity_and_zero_gradients():
    c, r = fp.case("edges"), fp.result("edges")
    fin = np.isfinite(r.scores)
    want = [n.startswith("valid") or n in ("num_arcs above the width", "negative num_arcs") for n in fp.EDGES]
    assert fin.tolist() == want, list(zip(fp.EDGES, r.scores))
    assert np.isneginf(r.scores[~fin]).all() and np.isneginf(r.scores32[~fin]).all()
    for b in np.nonzero(~fin)[0]:
        assert (r.grad[b] == 0).all() and (r.garc[b] == 0).all() and (r.grad32[b] == 0).all() and (r.garc32[b] == 0).all()
    assert (r.grad[0] == 0).all() and (r.garc[0] == 0).all()  # a weight of exactly 0 on a finite score
    # the width counts where num_arcs is above it; a negative count is no arc: the node's blank alone
    assert r.scores[13] != r.scores[0] and np.count_nonzero(r.garc[13]) == 12
    assert r.scores[14] == float(np.sum(c.em[14, :, c.blank].astype(np.float64)))
    assert (r.garc[14] == 0).all() and np.count_nonzero(r.grad[14]) == c.em.shape[1]
    # the forbidden arc, the dead end and the arc out of the unreachable node carry nothing
    # (and neither does arc 0, which leads to them alone)
    assert (r.garc[10, [0, 2, 3, 5]] == 0).all() and np.count_nonzero(r.garc[10]) == 3
    assert np.isfinite(r.grad).all() and np.isfinite(r.garc).all() and not np.isnan(r.scores).any()


def test_frames_equal_slicing_and_pad_rows_have_no_gradient():
    c, r = fp.case("ragged"), fp.result("ragged")
    for b, f in enumerate(fp.RAGGED_FRAMES):
        assert (r.grad[b, f:] == 0).all() and (r.grad32[b, f:] == 0).all()
    assert np.isneginf(r.scores[2]) and np.isneginf(r.scores[6]) and np.isfinite(r.scores[[0, 1, 3, 4, 5]]).all()
    lat = fp.lattice_of(c.arcs[6], c.num_arcs[6], c.num_nodes[6], None, 5, c.max_states)
    assert fp.min_frames(*lat[:3], lat[4]) == fp.RAGGED_FRAMES[6] + 1  # one frame fewer than the shortest path
    assert np.isfinite(r.grad).all() and not np.isnan(r.scores).any()


@pytest.mark.parametrize("name", fp.ALL_GPU_CASES)
def test_the_transcription_stays_inside_the_gate(name):
    """float32 in the kernel's order against float64, on every case the GPU file runs"""
    c, r = fp.case(name), fp.result(name)
    assert np.abs(c.gout).max() <= 1.0
    print(name, "score error", fp.score_err(r.scores32, r.scores), "gradient error", fp.grad_err(r.grad32, r.grad),
          "arc gradient error", fp.grad_err(r.garc32, r.garc))
    assert fp.score_ok(r.scores32, r.scores)
    assert fp.grad_err(r.grad32, r.grad) <= fp.GRAD_GATE
    assert fp.grad_err(r.garc32, r.garc) <= fp.GRAD_GATE
    assert np.isfinite(r.scores).any()  # (a case that scores nothing shows nothing)


def test_the_cases_cover_the_kernels_edges():
    states, configs, indeg, labels, frames = set(), set(), set(), set(), set()
    above = 0
    for name in fp.ALL_GPU_CASES:
        c = fp.case(name)
        B, T, C = c.em.shape
        configs.add(fp.config(c.max_states))
        labels.add(C)
        frames |= set(c.frames if c.frames is not None else [T])
        for b in range(B):
            A = min(max(int(c.num_arcs[b]), 0), c.arcs.shape[1])
            S = int(c.num_nodes[b]) + A
            above += S > c.max_states
            lat = fp.lattice_of(c.arcs[b], c.num_arcs[b], c.num_nodes[b], None, C, c.max_states)
            if lat is not None:
                states.add(S)
                indeg |= set(np.bincount(lat[1], minlength=lat[4]).tolist())
    assert configs == {(64, 1), (256, 1), (256, 3), (1024, 1), (1024, 2), (1024, 4)}
    assert {1, 63, 64, 65, 255, 256, 257, 768, 769, 1023, 1024, 1025, 2048, 2049, 4095, 4096} <= states
    assert above >= 1
    assert {0, 1, 2, 8} <= indeg and max(indeg) >= 500
    deep = fp.case("deep")
    assert deep.num_nodes[0] == 1025 and deep.em.shape[1] == 360
    assert set((deep.arcs[0, :deep.num_arcs[0], 1] - deep.arcs[0, :deep.num_arcs[0], 0]).tolist()) == {1, 2, 3}
    assert {2, 5, 37, 256} <= labels
    assert {0, 1} <= frames and len(frames) > 4
    for pad in (np.nan, np.inf):
        c = fp._ragged_case(pad)
        assert all((np.isnan(c.em[b, f:]).all() if np.isnan(pad) else (c.em[b, f:] == pad).all())
                   for b, f in enumerate(fp.RAGGED_FRAMES))


# ---- the builders ----
def test_decomposition_lattice_gives_the_lattice_of_the(gtn):
    import gtn_amd
    arcs, K = gtn_amd.decomposition_lattice("the", fp.the_pieces())
    assert K == 4 and arcs.dtype == np.int32
    # examples/learned_decompositions.cpp: t, th, the, h, he, e with the labels e 0, h 1, t 2, th 3, he 4, the 5
    assert sorted(map(tuple, arcs.tolist())) == sorted([(0, 1, 2), (0, 2, 3), (0, 3, 5), (1, 2, 1), (1, 3, 4), (2, 3, 0)])
    assert (np.diff(arcs[:, 1]) >= 0).all()
    short, _ = gtn_amd.decomposition_lattice(list("the"), {("t",): 2, ("h",): 1, ("e",): 0, ("t", "h"): 3}, max_piece_len=1)
    assert short.tolist() == [[0, 1, 2], [1, 2, 1], [2, 3, 0]]
    none, K0 = gtn_amd.decomposition_lattice("", fp.the_pieces())
    assert none.shape == (0, 3) and K0 == 1


def test_lattice_from_graph(gtn):
    import gtn_amd
    g = gtn.Graph(False)
    for n in range(5):
        g.add_node(n == 3, n == 1)  # start 3, accept 1: the numbering is turned round
    g.add_arc(3, 0, 7, 7, 0.5)
    g.add_arc(0, 1, 8, 8, -0.25)
    g.add_arc(3, 1, 9, 9, 1.5)
    g.add_arc(0, 2, 6, 6, 0.0)  # a dead end: trimmed
    g.add_arc(4, 1, 5, 5, 0.0)  # out of an unreachable node: trimmed
    arcs, K, w = gtn_amd.lattice_from_graph(g)
    assert K == 3 and arcs.tolist() == [[0, 1, 7], [0, 2, 9], [1, 2, 8]] and w.tolist() == [0.5, 1.5, -0.25]
    cyc = gtn.Graph(False)
    cyc.add_node(True, False)
    cyc.add_node(False, True)
    cyc.add_arc(0, 1, 1)
    cyc.add_arc(1, 0, 2)
    with pytest.raises(ValueError, match="cycle"):
        gtn_amd.lattice_from_graph(cyc)
    eps = gtn.Graph(False)
    eps.add_node(True, False)
    eps.add_node(False, True)
    eps.add_arc(0, 1, gtn.epsilon)
    with pytest.raises(ValueError, match="epsilon"):
        gtn_amd.lattice_from_graph(eps)
    two = gtn.Graph(False)
    two.add_node(True, True)
    two.add_node(True, False)
    with pytest.raises(ValueError, match="exactly one start"):
        gtn_amd.lattice_from_graph(two)


def test_pack_lattices_sorts_by_dst(gtn):
    import gtn_amd
    a = ([(1, 2, 5), (0, 2, 4), (0, 1, 3)], 3, [0.5, 0.25, 0.125])
    b = (np.zeros((0, 3), np.int32), 1)
    arcs, na, nn_, w = gtn_amd.pack_lattices([a, b, gtn_amd.decomposition_lattice("the", fp.the_pieces())])
    assert arcs.shape == (3, 6, 3) and arcs.dtype == np.int32 and w.dtype == np.float32 and w.shape == (3, 6)
    assert na.tolist() == [3, 0, 6] and nn_.tolist() == [3, 1, 4]
    assert arcs[0, :3].tolist() == [[0, 1, 3], [0, 2, 4], [1, 2, 5]] and w[0, :3].tolist() == [0.125, 0.25, 0.5]
    for r in range(3):
        assert (np.diff(arcs[r, :na[r], 1]) >= 0).all()
    assert (w[1:] == 0).all()


# ---- the entry points ----
def test_entry_points_exist(gtn):
    from gtn_amd import torch_loss
    assert callable(torch_loss.ctc_lattice_score) and callable(torch_loss.ctc_lattice_loss)
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    assert hasattr(lib, "gtn_ctc_lattice_score_n") and hasattr(lib, "gtn_ctc_lattice_score_grad_n")
    eng = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_amd.so"))
    for name in ("gtnx_batch_ctc_lattice_score", "gtnx_batch_ctc_lattice_score_grad",
                 "gtnx_batch_ctc_lattice_score_stats"):
        assert hasattr(eng, name), name
    assert callable(gtn.Batch.ctc_lattice_score) and callable(gtn.Batch.ctc_lattice_score_grad)
    calls, utts = gtn.debug_ctc_lattice_score_stats()
    assert calls >= 0 and utts >= 0
    for header, name in (("include/gtn_amd.h", "gtnx_batch_ctc_lattice_score_grad"),
                         ("include/gtn_amd.h", "gtnx_batch_ctc_lattice_score_stats"),
                         ("include/gtn/batch.h", "ctcLatticeScoreGrad"), ("include/gtn/batch.h", "ctcLatticeScore"),
                         ("gtn_amd/criteria/ctc_criterion.h", "ctcLatticeScoreBatch"),
                         ("gtn_amd/csrc/kernels.h", "CtcLatticeArgs"), ("gtn_amd/csrc/batch.h", "batch_ctc_lattice_score_grad")):
        with open(os.path.join(ROOT, header)) as f:
            assert name in f.read(), header


def test_argument_errors_come_before_the_device(gtn):
    """what the arguments alone decide is GTNX_INVALID_ARGUMENT (1) with or without a device"""
    import gtn_amd
    lib = gtn_amd._lib
    batch = gtn.Batch([gtn.linear_graph(2, 8)])
    p = ctypes.c_void_p
    score, grad = lib.gtnx_batch_ctc_lattice_score, lib.gtnx_batch_ctc_lattice_score_grad
    #        ems      frames blank arcs stride num_arcs num_nodes weights A  max_states
    good = [batch._h, None, 0, p(64), 12, p(64), p(64), None, 4, 8]
    before = gtn.debug_ctc_lattice_score_stats()

    def bad(i, v):
        a = list(good)
        a[i] = v
        return a
    refused = [bad(0, None), bad(3, None), bad(5, None), bad(6, None), bad(8, -1), bad(4, 11), bad(4, -1), bad(2, -1),
               bad(9, 0), bad(9, 4097), bad(9, -5)]
    for a in refused:
        assert score(*a, p(64)) == 1, a
        assert grad(*a, p(64), p(64), None) == 1, a
    assert score(*good, None) == 1
    assert grad(*good, None, p(64), None) == 1
    assert grad(*good, p(64), None, p(64)) == 1
    assert gtn.debug_ctc_lattice_score_stats() == before  # (nothing launched)
    with pytest.raises(ValueError, match="max_states outside"):
        batch.ctc_lattice_score(64, 64, 64, 64, A=4, row_stride=12, max_states=0)
    with pytest.raises(ValueError, match="needs A and row_stride"):
        batch.ctc_lattice_score(64, 64, 64, 64)
    with pytest.raises(ValueError, match="null weights or grad"):
        batch.ctc_lattice_score_grad(64, 64, 64, 0, 64, A=4, row_stride=12, max_states=8)
    with pytest.raises(ValueError, match="shorter than the rows' width"):
        batch.ctc_lattice_score(64, 64, 64, 64, A=4, row_stride=11, max_states=8)


def test_a_batch_without_an_utterance_needs_no_device(gtn):
    import gtn_amd
    lib = gtn_amd._lib
    p = ctypes.c_void_p
    empty = gtn.Batch([])
    if empty._h:  # (a batch without elements may have no handle to give: then there is nothing to call with)
        before = gtn.debug_ctc_lattice_score_stats()
        assert lib.gtnx_batch_ctc_lattice_score(empty._h, None, 0, p(64), 12, p(64), p(64), None, 4, 8, p(64)) == 0
        assert lib.gtnx_batch_ctc_lattice_score_grad(empty._h, None, 0, p(64), 12, p(64), p(64), None, 4, 8, p(64), p(64),
                                                     None) == 0
        assert gtn.debug_ctc_lattice_score_stats() == before


def test_torch_argument_checks():
    import torch
    from gtn_amd import torch_loss
    em = torch.zeros(2, 3, 8)
    arcs = torch.zeros(2, 4, 3, dtype=torch.int32)
    na = torch.zeros(2, dtype=torch.int32)
    nn_ = torch.ones(2, dtype=torch.int32)
    w = torch.zeros(2, 4)
    for args, kw, msg in (((em.double(), arcs, na, nn_), {}, "float32 tensor"), ((em[0], arcs, na, nn_), {}, "float32 tensor"),
                          ((em, arcs.long(), na, nn_), {}, "arcs must be an int32"),
                          ((em, arcs[:1], na, nn_), {}, "arcs must be an int32"),
                          ((em, arcs[:, :, :2], na, nn_), {}, "arcs must be an int32"),
                          ((em, arcs, na.float(), nn_), {}, "num_arcs must be an int32 or int64"),
                          ((em, arcs, na, nn_[:1]), {}, "num_nodes must be an int32 or int64"),
                          ((em, arcs, na, nn_, w[:, :3]), {}, "arc_weights must be a floating-point"),
                          ((em, arcs, na, nn_, w.long()), {}, "arc_weights must be a floating-point"),
                          ((em, arcs, na, nn_), dict(blank=8), "blank must be one of"),
                          ((em, arcs, na, nn_), dict(blank=-1), "blank must be one of"),
                          ((em, arcs, na, nn_), dict(max_states=0), "max_states outside 1 .. 4096"),
                          ((em, arcs, na, nn_), dict(max_states=4097), "max_states outside 1 .. 4096"),
                          ((em, arcs, na, nn_), dict(input_lengths=[4, 1]), "input length outside 0 .. 3"),
                          ((em, arcs, na, nn_), dict(input_lengths=[1]), "input lengths for a batch of 2")):
        with pytest.raises(ValueError, match=msg):
            torch_loss.ctc_lattice_score(*args, **kw)
        with pytest.raises(ValueError, match=msg):
            torch_loss.ctc_lattice_loss(*args, **kw)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        torch_loss.ctc_lattice_score(em, arcs, na, nn_)
    assert "sorted by dst" in torch_loss.ctc_lattice_score.__doc__ and "ctc_loss" in torch_loss.ctc_lattice_loss.__doc__


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU behaviour")
def test_ctc_lattice_score_fails_loudly_without_gpu(gtn):
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.gtn_ctc_lattice_score_n.argtypes = [P, I, I, I, I, P, P, P, P, P, I, I, P]
    lib.gtn_ctc_lattice_score_n.restype = I
    lib.gtn_ctc_lattice_score_grad_n.argtypes = [P, I, I, I, I, P, P, P, P, P, I, I, P, P, P]
    lib.gtn_ctc_lattice_score_grad_n.restype = I
    lib.gtn_criteria_last_error.restype = ctypes.c_char_p
    rc = lib.gtn_ctc_lattice_score_n(None, 1, 2, 8, 0, None, P(64), P(64), P(64), None, 2, 4, P(64))
    assert rc == -1 and "no HIP device" in lib.gtn_criteria_last_error().decode()
    rc = lib.gtn_ctc_lattice_score_grad_n(None, 1, 2, 8, 0, None, P(64), P(64), P(64), None, 2, 4, P(64), P(64), None)
    assert rc == -1 and "no HIP device" in lib.gtn_criteria_last_error().decode()
    batch = gtn.Batch([gtn.linear_graph(2, 8)])
    with pytest.raises(RuntimeError, match="no HIP device"):
        batch.ctc_lattice_score(64, 64, 64, 64, A=2, row_stride=6, max_states=4)
    with pytest.raises(RuntimeError, match="no HIP device"):
        batch.ctc_lattice_score_grad(64, 64, 64, 64, 64, A=2, row_stride=6, max_states=4)
