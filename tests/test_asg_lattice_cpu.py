"""ASG scores of token lattices, the parts that need no GPU.  The float64 yardstick of tests/asg_lattice_fp.py (which
test_asg_lattice_gpu.py judges the kernels by) is pinned twice on small lattices: to the enumeration of the lattice's
paths -- logsumexp of w(p) + asg_loss_fp.fal_fp64(em, labels(p)), its gradients the softmax-weighted sums (1e-9) -- and
to the oracle's forwardScore of the expanded graph built arc by arc (1e-4 max(1, |score|), the bound the CPU tests give
that float32 oracle).  A chain lattice is asg_score, and full-connect minus its score asg_loss.  The float32
transcription of the kernel stays inside all three gates on every case the GPU file runs, the cases sit at the kernel's
edges, and the entry points exist in every layer, refuse bad arguments before they ask for a device, and fail loudly
without one."""
import ctypes
import os

import numpy as np
import pytest

import asg_lattice_fp as fp
import ctc_beam_fp as bfp
from asg_loss_fp import asg_terms_fp64, fal_fp64
from conftest import ROOT, has_gpu
from ctc_fp64 import _lse
from oracle_lib import OGraph, lib as oracle

NEG = -np.inf

# small lattices: (name, arcs (src, dst, label), nodes, weights or None); labels below C = 3 or 4
SMALL_LATTICES = [
    ("parallel arcs of equal label", [(0, 1, 1), (0, 1, 1), (1, 2, 2), (0, 2, 2)], 3, [0.3, -0.7, 0.1, 0.4]),
    ("consecutive arcs of equal label", [(0, 1, 1), (1, 2, 1), (1, 2, 2), (2, 3, 1)], 4, None),
    ("label 0 among the others", [(0, 1, 0), (0, 1, 2), (1, 2, 0), (1, 2, 2), (0, 2, 1)], 3, [0.2, 0.0, -0.4, 0.9, -1.0]),
    ("a dead-end arc", [(0, 1, 1), (0, 2, 2), (1, 3, 2), (1, 4, 1), (0, 4, 2)], 5, None),  # nodes 2 and 3 lead nowhere
    ("an unreachable node", [(0, 1, 1), (2, 3, 2), (1, 3, 2), (0, 3, 1)], 4, [0.5, 0.25, -0.5, 0.0]),
    ("a -inf weight", [(0, 1, 1), (0, 1, 2), (1, 2, 1), (1, 2, 2)], 3, [0.1, NEG, -0.2, 0.3]),
    ("the one-node lattice", [], 1, None),
    ("a diamond of decompositions", [(0, 1, 2), (0, 2, 1), (1, 2, 1), (0, 3, 2), (1, 3, 1), (2, 3, 2)], 4,
     [0.1, 0.2, -0.3, 0.4, 0.0, -0.6]),
]
SMALL_EMS = [("continuous", 0, 1, 3), ("continuous", 1, 3, 3), ("holes", 2, 4, 3), ("integer", 3, 5, 4),
             ("continuous", 4, 6, 3), ("holes", 5, 6, 4)]


def small_model(kind, seed, T, C):
    make = {"continuous": bfp.continuous_case, "holes": bfp.holes_case, "integer": bfp.integer_case}[kind]
    rng = np.random.default_rng(300 + seed)
    return (make(200 + seed, 1, T, C)[0], rng.normal(0.0, 0.5, (C, C)).astype(np.float32),
            rng.normal(0.0, 0.5, C).astype(np.float32))


def lattice_arrays(arcs, weights):
    a, w = fp.sort_by_dst(arcs, weights)
    a = a.astype(np.int64)
    return a[:, 0], a[:, 1], a[:, 2], (np.zeros(len(a)) if w is None else w.astype(np.float64))


def by_enumeration(em, trans, start, src, dst, lab, w, K):
    """(score, d / d em, d / d w, d / d table) as the sum over the lattice's paths of asg_score's yardstick"""
    paths = [p for p in fp.paths_of(src, dst, K) if p]
    assert len(paths) <= 400
    terms = []
    for p in paths:
        z, g, gt = fal_fp64(em, trans, start, lab[p])
        terms.append((float(np.sum(w[p])) + z if np.isfinite(z) else NEG, g, gt, p))
    zs = np.array([t[0] for t in terms] or [NEG])
    total = float(_lse(zs)) if np.isfinite(zs).any() else NEG
    if not np.isfinite(total):
        return NEG, None, None, None
    C = em.shape[1]
    grad, garc, gtable = np.zeros(em.shape), np.zeros(len(src)), np.zeros(C + C * C)
    for z, g, gt, p in terms:
        if np.isfinite(z):
            grad += np.exp(z - total) * g
            gtable += np.exp(z - total) * gt
            np.add.at(garc, p, np.exp(z - total))  # (an arc counts once per use)
    return total, grad, garc, gtable


@pytest.mark.parametrize("kind,seed,T,C", SMALL_EMS)
@pytest.mark.parametrize("which", range(len(SMALL_LATTICES)))
def test_yardstick_is_the_enumeration(kind, seed, T, C, which):
    name, arcs, K, weights = SMALL_LATTICES[which]
    em, trans, start = small_model(kind, seed, T, C)
    src, dst, lab, w = lattice_arrays(arcs, weights)
    want = by_enumeration(em, trans, start, src, dst, lab, w, K)
    got = fp.lattice_fp64(em, trans, start, src, dst, lab, w, K)
    if np.isfinite(want[0]):
        assert abs(got[0] - want[0]) <= 1e-9, (name, got[0], want[0])
        for g, wnt in zip(got[1:], want[1:]):
            np.testing.assert_allclose(g, wnt, rtol=0, atol=1e-9)
    else:
        assert got[0] == NEG and all(g is None for g in got[1:]), (name, got[0])


@pytest.mark.parametrize("kind,seed,T,C", SMALL_EMS)
@pytest.mark.parametrize("which", range(len(SMALL_LATTICES)))
def test_yardstick_is_the_oracle(kind, seed, T, C, which):
    """forwardScore of the expanded graph, built arc by arc -- a start node plus one node per arc, start and step arcs
    carrying w_a + the table entry, self-loops carrying tr[l][l] -- intersected with linearGraph(T, C) (float32)"""
    name, arcs, K, weights = SMALL_LATTICES[which]
    em, trans, start = small_model(kind, seed, T, C)
    src, dst, lab, w = lattice_arrays(arcs, weights)
    wo = np.where(np.isfinite(w), w, -1e30)  # (the float32 oracle adds weights: a very low one stands in for -inf)
    L = oracle()
    g = OGraph()
    A = len(src)
    L.og_add_node(g.h, 1, 0)
    for a in range(A):
        L.og_add_node(g.h, 0, int(dst[a] == K - 1))
    for a in range(A):
        s, l = 1 + a, int(lab[a])
        L.og_add_arc(g.h, s, s, l, l, float(trans[l, l]))
        if src[a] == 0:
            L.og_add_arc(g.h, 0, s, l, l, float(wo[a] + start[l]))
        for a2 in range(A):
            if dst[a2] == src[a]:
                L.og_add_arc(g.h, 1 + a2, s, l, l, float(wo[a] + trans[l, int(lab[a2])]))
    want = g.compose(OGraph.linear(T, C, em), "intersect").shortest_distance(tropical=False)
    got = fp.lattice_fp64(em, trans, start, src, dst, lab, w, K)[0]
    if want is None or not np.isfinite(want) or want < -1e29:
        assert got == NEG, (name, got, want)
    else:
        assert abs(got - want) <= 1e-4 * max(1.0, abs(want)), (name, got, want)


@pytest.mark.parametrize("kind,seed,T,C", SMALL_EMS + [("continuous", 7, 12, 5)])
def test_a_chain_is_asg_score_and_full_connect_minus_it_asg_loss(kind, seed, T, C):
    em, trans, start = small_model(kind, seed, T, C)
    rng = np.random.default_rng(seed)
    for n in range(1, T + 2):
        y = rng.integers(0, C, n)
        arcs, K = fp.chain_lattice(y)
        src, dst, lab, w = lattice_arrays(arcs, None)
        z, g, ga, gt = fp.lattice_fp64(em, trans, start, src, dst, lab, w, K)
        want, gw, gtw = fal_fp64(em, trans, start, y)
        if np.isfinite(want):
            assert abs(z - want) <= 1e-12 * max(1.0, abs(want)), (n, z, want)
            np.testing.assert_allclose(g, gw, rtol=0, atol=1e-12)
            np.testing.assert_allclose(gt, gtw, rtol=0, atol=1e-12)
            np.testing.assert_allclose(ga, np.ones(n), rtol=0, atol=1e-9)  # (every arc of a chain is used)
            terms = asg_terms_fp64(em, trans, start, y)  # (the full-connect term on its own, and the loss)
            assert abs((terms["fcc"] - z) - terms["loss"]) <= 1e-9 * max(1.0, abs(terms["loss"]))
        else:
            assert z == NEG and g is None


def test_every_invalid_lattice_gives_minus_infinity_and_zero_gradients():
    c, r = fp.case("edges"), fp.result("edges")
    fin = np.isfinite(r.scores)
    want = [n.startswith("valid") or n == "num_arcs above the width" for n in fp.EDGES]
    assert fin.tolist() == want, list(zip(fp.EDGES, r.scores))
    assert np.isneginf(r.scores[~fin]).all() and np.isneginf(r.scores32[~fin]).all()
    for b in np.nonzero(~fin)[0]:
        assert (r.grad[b] == 0).all() and (r.garc[b] == 0).all() and (r.grad32[b] == 0).all() and (r.garc32[b] == 0).all()
    assert (r.grad[0] == 0).all() and (r.garc[0] == 0).all()  # a weight of exactly 0 on a finite score
    assert r.scores[13] != r.scores[0] and np.count_nonzero(r.garc[13]) == 12  # the width counts where num_arcs is above
    # the forbidden arc, the dead end and the arc out of the unreachable node carry nothing (nor arc 0, which leads there)
    assert (r.garc[10, [0, 2, 3, 5]] == 0).all() and np.count_nonzero(r.garc[10]) == 3
    # one of two paths crosses the -inf bigram: the arc of label 6 carries nothing, the other two everything
    np.testing.assert_allclose(r.garc[18, :3] / c.gout[18], [0.0, 1.0, 1.0], atol=1e-12)
    assert np.isfinite(r.grad).all() and np.isfinite(r.garc).all() and np.isfinite(r.gtable).all()
    assert not np.isnan(r.scores).any() and not np.isnan(r.scores32).any() and np.isfinite(r.gtable32).all()
    # the utterances that use labels 5 and 6 are these three alone: only the last of them reaches the table's rows
    C = fp.EDGES_C
    assert r.gtable[5] == 0 and r.gtable[C + 5 * C + 6] == 0 and r.gtable[C + 5 * C + 1] != 0


def test_frames_equal_slicing_and_pad_rows_have_no_gradient():
    c, r = fp.case("ragged"), fp.result("ragged")
    for b, f in enumerate(fp.RAGGED_FRAMES):
        assert (r.grad[b, f:] == 0).all() and (r.grad32[b, f:] == 0).all()
    assert np.isneginf(r.scores[2]) and np.isneginf(r.scores[6]) and np.isfinite(r.scores[[0, 1, 3, 4, 5]]).all()
    assert c.num_arcs[6] == fp.RAGGED_FRAMES[6] + 1 and c.num_nodes[6] == c.num_arcs[6] + 1  # a chain, one frame short
    assert np.isfinite(r.grad).all() and not np.isnan(r.scores).any() and np.isnan(c.em[0:3, 1:]).any()


@pytest.mark.parametrize("name", fp.ALL_GPU_CASES)
def test_the_transcription_stays_inside_the_gates(name):
    """float32 in the kernel's order against float64, on every case the GPU file runs"""
    c, r = fp.case(name), fp.result(name)
    assert np.abs(c.gout).max() <= 1.0
    print(name, "score error", fp.score_err(r.scores32, r.scores), "gradient error", fp.grad_err(r.grad32, r.grad),
          "arc gradient error", fp.grad_err(r.garc32, r.garc), "table gradient error", fp.table_err(r.gtable32, r.gtable))
    assert fp.score_ok(r.scores32, r.scores)
    assert fp.grad_err(r.grad32, r.grad) <= fp.GRAD_GATE
    assert fp.grad_err(r.garc32, r.garc) <= fp.GRAD_GATE
    assert fp.table_err(r.gtable32, r.gtable) <= fp.TABLE_GATE
    assert np.isfinite(r.scores).any()  # (a case that scores nothing shows nothing)


def test_the_cases_cover_the_kernels_edges():
    states, configs, indeg, labels, frames = set(), set(), set(), set(), set()
    above = at_cap = over_cap = 0
    for name in fp.ALL_GPU_CASES:
        c = fp.case(name)
        B, T, C = c.em.shape
        configs.add(fp.config(c.max_states))
        labels.add(C)
        frames |= set(c.frames if c.frames is not None else [T])
        cap = fp.max_edges_of(c)
        assert 1 <= cap <= fp.MAX_EDGES and 1 <= c.max_states <= fp.MAX_STATES
        for b in range(B):
            A = min(max(int(c.num_arcs[b]), 0), c.arcs.shape[1])
            S = int(c.num_nodes[b]) + A
            above += S > c.max_states
            lat = fp.lattice_of(c.arcs[b], c.num_arcs[b], c.num_nodes[b], None, C, c.max_states)
            if lat is not None:
                E = fp.edge_count(lat[0], lat[1], lat[4])
                at_cap += E == cap
                over_cap += E == cap + 1
                if E <= cap:
                    states.add(S)
                    indeg |= set(np.bincount(lat[1], minlength=lat[4]).tolist())
    assert configs == {(64, 1), (256, 1), (256, 3), (1024, 1), (1024, 2), (1024, 4)}
    assert {1, 63, 64, 65, 255, 256, 257, 768, 769, 1023, 1024, 1025, 2048, 2049, 4095, 4096} <= states
    assert above >= 10  # (every state-count case has one)
    assert at_cap >= 6 and over_cap == 1  # max_edges itself is legal, one more is not
    assert {0, 1, 2, 8} <= indeg and max(indeg) >= 500
    sa = fp.case("sausage")
    lat = fp.lattice_of(sa.arcs[0], sa.num_arcs[0], sa.num_nodes[0], None, 5, 4096)
    assert 1.8e6 < fp.edge_count(lat[0], lat[1], lat[4]) <= fp.MAX_EDGES and fp.max_edges_of(sa) == fp.MAX_EDGES
    deep = fp.case("deep")
    assert deep.num_nodes[0] == 1025 and deep.em.shape[1] == fp.DEEP_T < 360
    assert set((deep.arcs[0, :deep.num_arcs[0], 1] - deep.arcs[0, :deep.num_arcs[0], 0]).tolist()) == {1, 2, 3}
    assert {1, 5, 37, 300, 301} <= labels and 301 % 4 != 0
    assert {0, 1} <= frames and len(frames) > 4
    # the default max_edges is in use where the case leaves it open
    assert fp.case("indeg8-c37").max_edges is None and fp.max_edges_of(fp.case("indeg8-c37")) == 8 * fp.case("indeg8-c37").max_states
    for pad in (np.nan, np.inf):
        c = fp._ragged_case(pad)
        assert all((np.isnan(c.em[b, f:]).all() if np.isnan(pad) else (c.em[b, f:] == pad).all())
                   for b, f in enumerate(fp.RAGGED_FRAMES))


# ---- the entry points ----
def test_entry_points_exist(gtn):
    from gtn_amd import torch_loss
    assert callable(torch_loss.asg_lattice_score) and callable(torch_loss.asg_lattice_loss)
    assert callable(torch_loss.asg_full_connect)
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    for name in ("gtn_asg_lattice_score_n", "gtn_asg_lattice_score_grad_n", "gtn_asg_full_connect_n"):
        assert hasattr(lib, name), name
    eng = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_amd.so"))
    for name in ("gtnx_batch_asg_lattice_score", "gtnx_batch_asg_lattice_score_grad",
                 "gtnx_batch_asg_lattice_score_stats"):
        assert hasattr(eng, name), name
    assert callable(gtn.Batch.asg_lattice_score) and callable(gtn.Batch.asg_lattice_score_grad)
    calls, utts = gtn.debug_asg_lattice_score_stats()
    assert calls >= 0 and utts >= 0
    for header, name in (("include/gtn_amd.h", "gtnx_batch_asg_lattice_score_grad"),
                         ("include/gtn_amd.h", "gtnx_batch_asg_lattice_score_stats"),
                         ("include/gtn/batch.h", "asgLatticeScoreGrad"), ("include/gtn/batch.h", "asgLatticeScore"),
                         ("gtn_amd/criteria/asg_criterion.h", "asgLatticeScoreBatch"),
                         ("gtn_amd/criteria/asg_criterion.h", "asgFullConnectBatch"),
                         ("gtn_amd/csrc/kernels.h", "AsgLatticeArgs"), ("gtn_amd/csrc/kernels.h", "asg_lattice_config"),
                         ("gtn_amd/csrc/batch.h", "batch_asg_lattice_score_grad")):
        with open(os.path.join(ROOT, header)) as f:
            assert name in f.read(), header


def test_argument_errors_come_before_the_device(gtn):
    """what the arguments alone decide is GTNX_INVALID_ARGUMENT (1) with or without a device"""
    import gtn_amd
    lib = gtn_amd._lib
    batch = gtn.Batch([gtn.linear_graph(2, 8)])
    p = ctypes.c_void_p
    score, grad = lib.gtnx_batch_asg_lattice_score, lib.gtnx_batch_asg_lattice_score_grad
    #        ems      frames table arcs stride num_arcs num_nodes weights A  max_states max_edges
    good = [batch._h, None, p(64), p(64), 12, p(64), p(64), None, 4, 8, 64]
    before = gtn.debug_asg_lattice_score_stats()

    def bad(i, v):
        a = list(good)
        a[i] = v
        return a
    refused = [bad(0, None), bad(2, None), bad(3, None), bad(5, None), bad(6, None), bad(8, -1), bad(4, 11), bad(4, -1),
               bad(9, 0), bad(9, 4097), bad(9, -5), bad(10, 0), bad(10, (1 << 21) + 1), bad(10, -1)]
    for a in refused:
        assert score(*a, p(64)) == 1, a
        assert grad(*a, p(64), p(64), None, None) == 1, a
    assert score(*good, None) == 1
    assert grad(*good, None, p(64), None, None) == 1   # no weights
    assert grad(*good, p(64), None, None, None) == 1   # none of the three gradients
    assert gtn.debug_asg_lattice_score_stats() == before  # (nothing launched)
    with pytest.raises(ValueError, match="max_states outside"):
        batch.asg_lattice_score(64, 64, 64, 64, 64, A=4, row_stride=12, max_states=0)
    with pytest.raises(ValueError, match="max_edges outside"):
        batch.asg_lattice_score(64, 64, 64, 64, 64, A=4, row_stride=12, max_states=8, max_edges=0)
    with pytest.raises(ValueError, match="needs A and row_stride"):
        batch.asg_lattice_score(64, 64, 64, 64, 64)
    with pytest.raises(ValueError, match="none of grad_out"):
        batch.asg_lattice_score_grad(64, 64, 64, 64, 64, A=4, row_stride=12, max_states=8)
    with pytest.raises(ValueError, match="shorter than the rows' width"):
        batch.asg_lattice_score(64, 64, 64, 64, 64, A=4, row_stride=11, max_states=8)


def test_a_batch_without_an_utterance_needs_no_device(gtn):
    import gtn_amd
    lib = gtn_amd._lib
    p = ctypes.c_void_p
    empty = gtn.Batch([])
    if empty._h:  # (a batch without elements may have no handle to give: then there is nothing to call with)
        before = gtn.debug_asg_lattice_score_stats()
        args = (empty._h, None, p(64), p(64), 12, p(64), p(64), None, 4, 8, 64)
        assert lib.gtnx_batch_asg_lattice_score(*args, p(64)) == 0
        assert lib.gtnx_batch_asg_lattice_score_grad(*args, p(64), p(64), p(64), None) == 0
        assert gtn.debug_asg_lattice_score_stats() == before


def test_torch_argument_checks():
    import torch
    from gtn_amd import torch_loss
    em = torch.zeros(2, 3, 8)
    tr = torch.zeros(8, 8)
    arcs = torch.zeros(2, 4, 3, dtype=torch.int32)
    na = torch.zeros(2, dtype=torch.int32)
    nn_ = torch.ones(2, dtype=torch.int32)
    w = torch.zeros(2, 4)
    for args, kw, msg in (((em.double(), tr, arcs, na, nn_), {}, "float32 tensor"), ((em[0], tr, arcs, na, nn_), {}, "float32 tensor"),
                          ((em, tr[:7], arcs, na, nn_), {}, r"transitions must be \[8, 8\]"),
                          ((em, tr, arcs, na, nn_), dict(start=torch.zeros(7)), r"start must be \[8\]"),
                          ((em, tr, arcs.long(), na, nn_), {}, "arcs must be an int32"),
                          ((em, tr, arcs[:1], na, nn_), {}, "arcs must be an int32"),
                          ((em, tr, arcs[:, :, :2], na, nn_), {}, "arcs must be an int32"),
                          ((em, tr, arcs, na.float(), nn_), {}, "num_arcs must be an int32 or int64"),
                          ((em, tr, arcs, na, nn_[:1]), {}, "num_nodes must be an int32 or int64"),
                          ((em, tr, arcs, na, nn_, w[:, :3]), {}, "arc_weights must be a floating-point"),
                          ((em, tr, arcs, na, nn_, w.long()), {}, "arc_weights must be a floating-point"),
                          ((em, tr, arcs, na, nn_), dict(max_states=0), "max_states outside 1 .. 4096"),
                          ((em, tr, arcs, na, nn_), dict(max_states=4097), "max_states outside 1 .. 4096"),
                          ((em, tr, arcs, na, nn_), dict(max_edges=0), "max_edges outside 1 .. 2\\^21"),
                          ((em, tr, arcs, na, nn_), dict(max_edges=(1 << 21) + 1), "max_edges outside 1 .. 2\\^21"),
                          ((em, tr, arcs, na, nn_), dict(input_lengths=[4, 1]), "input length outside 0 .. 3"),
                          ((em, tr, arcs, na, nn_), dict(input_lengths=[1]), "input lengths for a batch of 2")):
        with pytest.raises(ValueError, match=msg):
            torch_loss.asg_lattice_score(*args, **kw)
        with pytest.raises(ValueError, match=msg):
            torch_loss.asg_lattice_loss(*args, **kw)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        torch_loss.asg_lattice_score(em, tr, arcs, na, nn_)
    for args, kw, msg in (((em.double(), tr), {}, "float32 tensor"), ((em, tr[:7]), {}, r"transitions must be \[8, 8\]"),
                          ((em, tr), dict(start=torch.zeros(7)), r"start must be \[8\]"),
                          ((em, tr), dict(reduction="max"), "reduction must be"),
                          ((em, tr), dict(input_lengths=[0, 1]), "input length outside 1 .. 3")):
        with pytest.raises(ValueError, match=msg):
            torch_loss.asg_full_connect(*args, **kw)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        torch_loss.asg_full_connect(em, tr)
    assert "sorted by dst" in torch_loss.asg_lattice_score.__doc__ and "asg_loss" in torch_loss.asg_lattice_loss.__doc__


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU behaviour")
def test_asg_lattice_score_fails_loudly_without_gpu(gtn):
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.gtn_asg_lattice_score_n.argtypes = [P, I, I, I, P, P, P, P, P, P, I, I, I, P]
    lib.gtn_asg_lattice_score_n.restype = I
    lib.gtn_asg_lattice_score_grad_n.argtypes = [P, I, I, I, P, P, P, P, P, P, I, I, I, P, P, P, P]
    lib.gtn_asg_lattice_score_grad_n.restype = I
    lib.gtn_asg_full_connect_n.argtypes = [P, I, I, I, P, P, P, P, P]
    lib.gtn_asg_full_connect_n.restype = I
    lib.gtn_criteria_last_error.restype = ctypes.c_char_p
    rc = lib.gtn_asg_lattice_score_n(None, 1, 2, 8, P(64), None, P(64), P(64), P(64), None, 2, 4, 32, P(64))
    assert rc == -1 and "no HIP device" in lib.gtn_criteria_last_error().decode()
    rc = lib.gtn_asg_lattice_score_grad_n(None, 1, 2, 8, P(64), None, P(64), P(64), P(64), None, 2, 4, 32, P(64), P(64),
                                          None, None)
    assert rc == -1 and "no HIP device" in lib.gtn_criteria_last_error().decode()
    rc = lib.gtn_asg_full_connect_n(None, 1, 2, 8, P(64), None, P(64), None, None)
    assert rc == -1 and "no HIP device" in lib.gtn_criteria_last_error().decode()
    batch = gtn.Batch([gtn.linear_graph(2, 8)])
    with pytest.raises(RuntimeError, match="no HIP device"):
        batch.asg_lattice_score(64, 64, 64, 64, 64, A=2, row_stride=6, max_states=4)
    with pytest.raises(RuntimeError, match="no HIP device"):
        batch.asg_lattice_score_grad(64, 64, 64, 64, 64, 64, A=2, row_stride=6, max_states=4)
