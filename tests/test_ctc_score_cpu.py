"""CTC scores of device-resident hypotheses, the parts that need no GPU.  The float64 yardstick of tests/ctc_score_fp.py
(which test_ctc_score_gpu.py judges the kernels by) is pinned three times on small cases: to a brute-force enumeration
of all C^T alignments (scores and gradients, 1e-9), to ctc_loss_fp64 through score == sum lse(rows) - loss and grad ==
softmax - grad_loss (1e-12), and to the oracle's forwardScore of the built product (1e-4 max(1, |score|), the bound the
CPU tests give that float32 oracle).  The float32 transcription of the kernel stays inside the gate on every case the
GPU file runs, so the gate is within reach of the method before a GPU is involved.  The entry points exist in every
layer, refuse bad arguments before they ask for a device, and fail loudly without one."""
import ctypes
import itertools
import os

import numpy as np
import pytest

import ctc_beam_fp as bfp
import ctc_score_fp as fp
from conftest import ROOT, has_gpu
from ctc_fp64 import _lse, ctc_loss_fp64
from oracle_lib import OGraph, lib as oracle

NEG = -np.inf
SMALL = [(kind, seed, T, C) for kind in ("continuous", "holes", "integer") for seed, (T, C) in
         enumerate([(1, 2), (3, 3), (4, 3), (5, 2), (6, 3), (6, 2)])]


def small_case(kind, seed, T, C):
    make = {"continuous": bfp.continuous_case, "holes": bfp.holes_case, "integer": bfp.integer_case}[kind]
    return make(100 + seed, 1, T, C)[0]


def brute_force(em, blank):
    """{label sequence: (log of the summed weight of its alignments, d of that log / d em)} over all C^T alignments"""
    T, C = em.shape
    x = em.astype(np.float64)
    paths = {}
    for path in itertools.product(range(C), repeat=T):
        y = tuple(c for t, c in enumerate(path) if c != blank and (t == 0 or c != path[t - 1]))
        paths.setdefault(y, []).append((path, float(sum(x[t, c] for t, c in enumerate(path)))))
    out = {}
    for y, ps in paths.items():
        z = float(_lse(np.array([s for _, s in ps])))
        g = np.zeros((T, C))
        if np.isfinite(z):
            for path, s in ps:
                g[np.arange(T), list(path)] += np.exp(s - z)
        out[y] = (z, g)
    return out


@pytest.mark.parametrize("kind,seed,T,C", SMALL)
@pytest.mark.parametrize("blank", ["first", "last"])
def test_yardstick_is_the_enumeration(kind, seed, T, C, blank):
    blank = 0 if blank == "first" else C - 1
    em = small_case(kind, seed, T, C)
    want = brute_force(em, blank)
    for y, (z, g) in want.items():
        got, grad = fp.pair_fp64(em, list(y), blank)
        if np.isfinite(z):
            assert abs(got - z) <= 1e-9, (y, got, z)
            np.testing.assert_allclose(grad, g, rtol=0, atol=1e-9)
        else:
            assert got == NEG and grad is None, (y, got)
    # a sequence no alignment spells: too long for T frames
    labels = [c for c in range(C) if c != blank]
    assert fp.pair_fp64(em, [labels[0]] * (T // 2 + 1) + labels[:1], blank)[0] == NEG
    # a token equal to blank is a label: its alignments are not in the collapsed enumeration, the recursion still
    # equals the oracle (test_yardstick_is_the_oracle)


@pytest.mark.parametrize("kind,seed,T,C", SMALL)
def test_yardstick_is_ctc_loss_fp64(kind, seed, T, C):
    em = small_case(kind, seed, T, C)
    rng = np.random.default_rng(seed)
    for n in range(0, T + 1):
        y = rng.integers(1, C, n)
        loss, gloss, _ = ctc_loss_fp64(em, y, 0)
        z, g = fp.pair_fp64(em, y, 0)
        rows = _lse(em.astype(np.float64), axis=1)
        if np.isfinite(loss):
            assert abs(z - (np.sum(rows) - loss)) <= 1e-12 * max(1.0, abs(z)), (n, z, loss)
            np.testing.assert_allclose(g, np.exp(em.astype(np.float64) - rows[:, None]) - gloss, rtol=0, atol=1e-12)
        else:
            assert z == NEG and g is None


def oracle_score(em, y, blank):
    """forwardScore(ctcTarget(y) intersected with linearGraph(T, C)) by the oracle (float32)"""
    T, C = em.shape
    tg = np.ascontiguousarray(y, dtype=np.int32)
    ctc = OGraph(oracle().og_ctc_graph(tg.ctypes.data, int(tg.size), int(blank), 1))
    return ctc.compose(OGraph.linear(T, C, em), "intersect").shortest_distance(tropical=False)


@pytest.mark.parametrize("kind,seed,T,C", SMALL)
def test_yardstick_is_the_oracle(kind, seed, T, C):
    em = small_case(kind, seed, T, C)
    rng = np.random.default_rng(50 + seed)
    for blank in (0, C - 1):
        for n in range(0, T + 1):
            y = rng.integers(0, C, n)  # (blank among the tokens: a label like any other)
            got = fp.pair_fp64(em, y, blank, want_grad=False)[0]
            want = oracle_score(em, y, blank)
            if want is None or not np.isfinite(want):
                assert got == NEG, (y, got, want)
            else:
                assert abs(got - want) <= 1e-4 * max(1.0, abs(want)), (y, got, want)


def test_the_contract_of_the_edges_case():
    """which slots score -inf, and that they and the zero weights add nothing"""
    r = fp.result("edges")
    fin = np.isfinite(r.scores)
    assert fin.tolist() == [[True, False, True, True], [False, False, True, True], [True, True, True, True]]
    assert np.isneginf(r.scores[~fin]).all()
    r7 = fp.result("edges-u7")
    assert np.isneginf(r7.scores[1, 3]) and np.isfinite(r7.scores[2, 3])  # a length above max_length
    c = fp.case("edges")
    empty = fp.pair_fp64(c.em[1], [], c.blank)[0]
    assert r.scores[1, 2] == empty == float(np.sum(c.em[1, :, c.blank].astype(np.float64)))  # finite: all blanks
    # utterance 0: its gradient is that of the three finite pairs with a non-zero weight
    want = sum(float(c.weights[0, k]) * fp.pair_fp64(c.em[0], fp.hypothesis(c.tokens[0, k], c.lengths[0, k], 8, 5, 8),
                                                     c.blank)[1] for k in (0, 2, 3))
    np.testing.assert_allclose(r.grad[0], want, rtol=0, atol=1e-12)


def test_frames_equal_slicing_and_pad_rows_have_no_gradient():
    c, r = fp.case("ragged"), fp.result("ragged")
    for b, f in enumerate(fp.RAGGED_FRAMES):
        assert (r.grad[b, f:] == 0).all() and (r.grad32[b, f:] == 0).all()
        if f == 0:
            assert np.isneginf(r.scores[b]).all()
    assert np.isfinite(r.grad).all() and not np.isnan(r.scores).any()
    assert np.isfinite(r.scores[0]).all()


@pytest.mark.parametrize("name", fp.ALL_GPU_CASES)
def test_the_transcription_stays_inside_the_gate(name):
    """float32 in the kernel's order against float64, on every case the GPU file runs"""
    c, r = fp.case(name), fp.result(name)
    assert np.abs(c.weights).max() <= 1.0
    print(name, "score error", fp.score_err(r.scores32, r.scores), "gradient error", fp.grad_err(r.grad32, r.grad))
    assert fp.score_ok(r.scores32, r.scores)
    assert fp.grad_err(r.grad32, r.grad) <= fp.GRAD_GATE
    assert np.isfinite(r.scores).any()  # (a case that scores nothing shows nothing)


def test_the_cases_cover_the_kernels_edges():
    lens = set()
    configs = set()
    for name in fp.ALL_GPU_CASES:
        c = fp.case(name)
        L = c.tokens.shape[-1]
        U = c.max_length if c.max_length is not None else fp.default_max_length(c)
        configs.add(fp.config(U))
        lens |= {min(max(int(n), 0), L) for n in np.asarray(c.lengths).reshape(-1)}
    assert configs == {(64, 1), (256, 1), (256, 3), (1024, 1), (1024, 2), (1024, 4), (1024, 9)}
    assert {0, 1, 31, 32, 33, 127, 128, 129} <= lens
    # the lengths at which the states a lane works on change: 2 len + 1 around the multiples of the width
    assert {127, 128, 255, 256, 383} <= lens and {511, 512, 1023, 1024, 1535, 1536, 2047, 2048} <= lens
    assert {2559, 2560, 3071, 3072, 3583, 3584, 4095, 4096} <= lens
    assert {fp.case(n).em.shape[2] for n in fp.ALL_GPU_CASES} >= {2, 5, 37, 256}


# ---- the entry points ----
def test_entry_points_exist(gtn):
    from gtn_amd import torch_loss
    assert callable(torch_loss.ctc_score)
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    assert hasattr(lib, "gtn_ctc_score_n") and hasattr(lib, "gtn_ctc_score_grad_n")
    eng = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_amd.so"))
    for name in ("gtnx_batch_ctc_score", "gtnx_batch_ctc_score_grad", "gtnx_batch_ctc_score_stats"):
        assert hasattr(eng, name), name
    assert callable(gtn.Batch.ctc_score) and callable(gtn.Batch.ctc_score_grad)
    calls, pairs = gtn.debug_ctc_score_stats()
    assert calls >= 0 and pairs >= 0
    for header, name in (("include/gtn_amd.h", "gtnx_batch_ctc_score_grad"), ("include/gtn/batch.h", "ctcScoreGrad"),
                         ("include/gtn/batch.h", "ctcScore"), ("gtn_amd/criteria/ctc_criterion.h", "ctcScoreBatch")):
        with open(os.path.join(ROOT, header)) as f:
            assert name in f.read(), header


def test_argument_errors_come_before_the_device(gtn):
    """what the arguments alone decide is GTNX_INVALID_ARGUMENT (1) with or without a device; a batch that is not a
    native linear one, a frame count outside 0 .. M and blank >= C are reached on the device only"""
    import gtn_amd
    lib = gtn_amd._lib
    batch = gtn.Batch([gtn.linear_graph(2, 8)])
    p = ctypes.c_void_p
    score, grad = lib.gtnx_batch_ctc_score, lib.gtnx_batch_ctc_score_grad
    #            ems       frames blank tokens stride lengths N  L  U  out...
    good = [batch._h, None, 0, p(64), 4, p(64), 1, 4, 4]
    before = gtn.debug_ctc_score_stats()

    def bad(i, v):
        a = list(good)
        a[i] = v
        return a
    refused = [bad(0, None), bad(3, None), bad(5, None), bad(6, -1), bad(7, -1), bad(4, -1), bad(2, -1), bad(4, 3),
               bad(8, 0), bad(8, 4097), bad(8, -5)]
    for a in refused:
        assert score(*a, p(64)) == 1, a
        assert grad(*a, p(64), p(64)) == 1, a
    assert score(*good, None) == 1
    assert grad(*good, None, p(64)) == 1
    assert grad(*good, p(64), None) == 1
    # no pair: OK without a device (N == 0 here; a batch without elements has no handle to give)
    assert score(*bad(6, 0), p(64)) == 0
    assert grad(*bad(6, 0), p(64), p(64)) == 0
    assert gtn.debug_ctc_score_stats() == before  # (nothing launched)
    with pytest.raises(ValueError, match="max_length outside"):
        batch.ctc_score(64, 64, 64, N=1, L=4, row_stride=4, max_length=0)
    with pytest.raises(ValueError, match="needs N, L and row_stride"):
        batch.ctc_score(64, 64, 64)
    with pytest.raises(ValueError, match="null weights or grad"):
        batch.ctc_score_grad(64, 64, 0, 64, N=1, L=4, row_stride=4, max_length=4)
    with pytest.raises(ValueError, match="shorter than the rows' width"):
        batch.ctc_score(64, 64, 64, N=1, L=4, row_stride=3, max_length=4)


def test_torch_argument_checks():
    import torch
    from gtn_amd import torch_loss
    em = torch.zeros(2, 3, 8)
    tok = torch.zeros(2, 2, 3, dtype=torch.int32)
    ln = torch.zeros(2, 2, dtype=torch.int32)
    for args, kw, msg in (((em.double(), tok, ln), {}, "float32 tensor"), ((em[0], tok, ln), {}, "float32 tensor"),
                          ((em, tok.long(), ln), {}, "tokens must be an int32"),
                          ((em, tok[:1], ln), {}, "tokens must be an int32"),
                          ((em, tok, ln.float()), {}, "lengths must be an int32 or int64"),
                          ((em, tok, ln[:, :1]), {}, "lengths must be an int32 or int64"),
                          ((em, tok[:, 0], ln), {}, "lengths must be an int32 or int64"),
                          ((em, tok, ln), dict(blank=8), "blank must be one of"),
                          ((em, tok, ln), dict(blank=-1), "blank must be one of"),
                          ((em, tok, ln), dict(max_length=0), "max_length outside 1 .. 4096"),
                          ((em, tok, ln), dict(max_length=4097), "max_length outside 1 .. 4096"),
                          ((em, tok, ln), dict(input_lengths=[4, 1]), "input length outside 0 .. 3"),
                          ((em, tok, ln), dict(input_lengths=[1]), "input lengths for a batch of 2")):
        with pytest.raises(ValueError, match=msg):
            torch_loss.ctc_score(*args, **kw)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        torch_loss.ctc_score(em, tok, ln)
    assert "mask such slots" in torch_loss.ctc_score.__doc__ and "empty" in torch_loss.ctc_score.__doc__


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU behaviour")
def test_ctc_score_fails_loudly_without_gpu(gtn):
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    lib.gtn_ctc_score_n.argtypes = ([ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 3
                                    + [ctypes.c_void_p])
    lib.gtn_ctc_score_n.restype = ctypes.c_int
    lib.gtn_criteria_last_error.restype = ctypes.c_char_p
    rc = lib.gtn_ctc_score_n(None, 1, 2, 8, 0, None, ctypes.c_void_p(64), ctypes.c_void_p(64), 1, 2, 2,
                             ctypes.c_void_p(64))
    assert rc == -1 and "no HIP device" in lib.gtn_criteria_last_error().decode()
    with pytest.raises(RuntimeError, match="no HIP device"):
        gtn.Batch([gtn.linear_graph(2, 8)]).ctc_score(64, 64, 64, N=1, L=2, row_stride=2, max_length=2)
