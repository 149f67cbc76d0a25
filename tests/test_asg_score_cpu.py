"""ASG scores of device-resident hypotheses, the parts that need no GPU.  The float64 yardstick (tests/asg_loss_fp.py:
fal_fp64, which test_asg_score_gpu.py judges the kernels by through tests/asg_score_fp.py) is pinned twice on small
cases: to a brute-force enumeration of all alignments (scores and both gradients, 1e-9) and to the oracle's forwardScore
of emissions o (forceAlign o transitions) (1e-4 max(1, |score|), the bound the CPU tests give that float32 oracle).  The
float32 transcription of the kernels stays inside the gates on every case the GPU file runs, so the gates are within
reach of the method before a GPU is involved, and the cases sit on the edges of the launch configuration, which is read
out of the kernel's source.  The entry points exist in every layer, refuse bad arguments before they ask for a device,
and fail loudly without one."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import asg_score_fp as fp
from asg_loss_fp import fal_fp64
from conftest import ROOT, has_gpu
from oracle_lib import OGraph

NEG = -np.inf
# (seed, T, C, hypothesis)
SMALL = [(0, 1, 2, [1]), (1, 3, 3, [0, 1]), (2, 4, 3, [2, 2]), (3, 5, 2, [0, 1, 0]), (4, 6, 3, [1, 1, 1]),
         (5, 6, 4, [3, 0, 3]), (6, 3, 3, [0, 1, 2]), (7, 6, 2, [1]), (8, 2, 3, [0, 1, 2])]


def small_model(seed, T, C, holes=False):
    rng = np.random.default_rng(300 + seed)
    em, trans, start = (a[0] if a.ndim == 3 else a for a in fp.model_of(rng, 1, T, C, sigma=1.0))
    if holes:
        em[rng.random(em.shape) < 0.2] = NEG
        trans[rng.random(trans.shape) < 0.2] = NEG
    return em, trans, start


def brute_force(em, trans, start, y):
    """(score, d score / d em [T, C], d score / d table [C + C * C]) over every alignment of y: the positions of the
    frames start at 0, end at len - 1 and rise by 0 or 1"""
    T, C = em.shape
    n = len(y)
    x, tr, st = em.astype(np.float64), trans.astype(np.float64), start.astype(np.float64)
    paths = []
    for steps in itertools.product((0, 1), repeat=T - 1):
        pos = np.concatenate([[0], np.cumsum(steps)]).astype(int)
        if pos[-1] != n - 1:
            continue
        s = st[y[0]] + x[0, y[0]]
        for t in range(1, T):
            s += tr[y[pos[t]], y[pos[t - 1]]] + x[t, y[pos[t]]]
        paths.append((pos, s))
    g_em, g_tab = np.zeros((T, C)), np.zeros(C + C * C)
    if not paths or not np.isfinite(max(s for _, s in paths)):
        return NEG, g_em, g_tab
    top = max(s for _, s in paths)
    z = top + np.log(sum(np.exp(s - top) for _, s in paths))
    for pos, s in paths:
        p = np.exp(s - z)
        g_tab[y[0]] += p
        for t in range(T):
            g_em[t, y[pos[t]]] += p
            if t:
                g_tab[C + y[pos[t]] * C + y[pos[t - 1]]] += p
    return float(z), g_em, g_tab


@pytest.mark.parametrize("seed,T,C,y", SMALL)
@pytest.mark.parametrize("holes", [False, True])
def test_yardstick_is_the_enumeration(seed, T, C, y, holes):
    em, trans, start = small_model(seed, T, C, holes)
    want = brute_force(em, trans, start, y)
    got = fal_fp64(em, trans, start, y)
    if np.isfinite(want[0]):
        assert abs(got[0] - want[0]) <= 1e-9, (got[0], want[0])
        np.testing.assert_allclose(got[1], want[1], rtol=0, atol=1e-9)
        np.testing.assert_allclose(got[2], want[2], rtol=0, atol=1e-9)
    else:
        assert got[0] == NEG and not got[1].any() and not got[2].any()
    if T < len(y):
        assert want[0] == NEG  # (no alignment: fewer frames than labels)


def oracle_score(em, trans, start, y):
    """forwardScore((forceAlign(y) o transitions) o linearGraph(T, C)) by the oracle (float32)"""
    T, C = em.shape
    n = len(y)
    td = {"start": [1] + [0] * C, "accept": [0] + [1] * C, "src": [], "dst": [], "il": [], "ol": [], "w": [], "sort": "i"}
    for i in range(C):
        td["src"].append(0), td["dst"].append(i + 1), td["il"].append(i), td["ol"].append(i)
        td["w"].append(float(start[i]))
    for i in range(C):
        for j in range(C):
            td["src"].append(j + 1), td["dst"].append(i + 1), td["il"].append(i), td["ol"].append(i)
            td["w"].append(float(trans[i, j]))
    fd = {"start": [1] + [0] * n, "accept": [int(n == 0)] + [int(l == n) for l in range(1, n + 1)],
          "src": [], "dst": [], "il": [], "ol": [], "w": [], "sort": None}
    for l in range(1, n + 1):
        for s in (l - 1, l):
            fd["src"].append(s), fd["dst"].append(l), fd["il"].append(int(y[l - 1])), fd["ol"].append(int(y[l - 1]))
            fd["w"].append(0.0)
    fa = OGraph.from_dict(fd).compose(OGraph.from_dict(td))
    return fa.compose(OGraph.linear(T, C, em.reshape(-1))).shortest_distance()


@pytest.mark.parametrize("seed,T,C,y", SMALL + [(20, 9, 5, [0, 1, 0, 1]), (21, 12, 4, [3, 3, 3, 0, 0]),
                                                (22, 7, 33, [32, 0, 5, 5, 31, 32, 0])])
def test_yardstick_is_the_oracle(seed, T, C, y):
    em, trans, start = small_model(seed, T, C)
    got = fal_fp64(em, trans, start, y)[0]
    want = oracle_score(em, trans, start, y)
    if want is None or not np.isfinite(want):
        assert got == NEG, (got, want)
        assert T < len(y)
    else:
        assert abs(got - want) <= 1e-4 * max(1.0, abs(want)), (got, want)


def test_the_contract_of_the_edges_case():
    """which slots score -inf, and that they and the zero weights add nothing"""
    c, r = fp.case("edges"), fp.result("edges")
    fin = np.isfinite(r.scores)
    assert fin.tolist() == [[True, True, False, True], [False, False, True, True], [True, False, True, True]]
    assert np.isneginf(r.scores[~fin]).all()
    r7 = fp.result("edges-u7")
    assert np.isneginf(r7.scores[2, 3]) and np.isfinite(r.scores[2, 3])  # a length above max_length
    C = c.em.shape[2]
    # the -inf entry kills (2, 1) and spares (2, 2), which has the same labels; nothing flows into the entry
    assert np.isneginf(c.trans[3, 4]) and r.gtable[C + 3 * C + 4] == 0 and r.gtable32[C + 3 * C + 4] == 0
    # utterance 2: its emission gradient is that of the pairs 2 and 3 ((2, 0) has weight 0, (2, 1) no score)
    want = sum(float(c.weights[2, k]) * fal_fp64(c.em[2], c.trans, c.start,
                                                 fp.hypothesis(c.tokens[2, k], c.lengths[2, k], 8, C, 8))[1]
               for k in (2, 3))
    np.testing.assert_allclose(r.grad[2], want, rtol=0, atol=1e-12)
    # the bigram 0 -> 1 is in (0, 1) twice, in (1, 2), (1, 3), (2, 3) twice -- and in (2, 0), whose weight is 0
    for b, k in ((0, 1), (1, 2), (1, 3), (2, 0), (2, 3)):
        y = c.tokens[b, k, :min(int(c.lengths[b, k]), 8)].tolist()
        assert any(y[i:i + 2] == [0, 1] for i in range(len(y)))
    assert r.gtable[C + 1 * C + 0] != 0


def test_frame_counts_from_no_frame_to_all():
    c, r = fp.case("frames"), fp.result("frames")
    n = fp.FRAMES_LEN
    assert fp.FRAMES[:4] == (n, n + 1, n - 1, 0) and (np.asarray(c.lengths)[:, 0] == n).all()
    fin = np.isfinite(r.scores)
    assert fin[:, 0].tolist() == [True, True, False, False, True, False]
    assert fin[:, 1].tolist() == [True, True, True, False, True, True]
    for b, f in enumerate(fp.FRAMES):
        assert (r.grad[b, f:] == 0).all() and (r.grad32[b, f:] == 0).all()
    assert np.isfinite(r.grad).all() and np.isfinite(r.gtable).all() and not np.isnan(r.scores).any()
    # T_b == len: the one alignment, every occupancy is 1
    np.testing.assert_allclose(fal_fp64(c.em[0, :n], c.trans, c.start, c.tokens[0, 0, :n])[1].sum(axis=1), 1.0)


@pytest.mark.parametrize("name", fp.ALL_GPU_CASES)
def test_the_transcription_stays_inside_the_gates(name):
    """float32 in the kernels' order against float64, on every case the GPU file runs"""
    c, r = fp.case(name), fp.result(name)
    assert np.abs(c.weights).max() <= 1.0
    print(name, "score error", fp.score_err(r.scores32, r.scores), "gradient error", fp.grad_err(r.grad32, r.grad),
          "table error", fp.table_err(r.gtable32, r.gtable))
    assert fp.score_ok(r.scores32, r.scores)
    assert fp.grad_err(r.grad32, r.grad) <= fp.GRAD_GATE
    assert fp.table_err(r.gtable32, r.gtable) <= fp.TABLE_GATE
    assert np.isfinite(r.scores).any()  # (a case that scores nothing shows nothing)
    assert np.abs(r.gtable).max() > 1e-3


def kernel_configs():
    """asg_score_config as gtn_amd/csrc/asg_score.hip has it: ((bound on max_length, (width, per lane)), ...), and the
    limits of gtn_amd/csrc/kernels.h"""
    with open(os.path.join(ROOT, "gtn_amd", "csrc", "asg_score.hip")) as f:
        body = f.read().split("void asg_score_config(")[1].split("\n}\n")[0]
    rows = [(int(u), (int(w), int(p))) for u, w, p in re.findall(r"U <= (\d+)\) wg = (\d+), per = (\d+);", body)]
    (w, p), = re.findall(r"else wg = (\d+), per = (\d+);", body)
    with open(os.path.join(ROOT, "gtn_amd", "csrc", "kernels.h")) as f:
        text = f.read()
    max_u = int(re.search(r"kAsgScoreMaxU = (\d+);", text).group(1))
    max_c = int(re.search(r"kAsgScoreMaxC = (\d+);", text).group(1))
    return tuple(rows) + ((max_u, (int(w), int(p))),), max_u, max_c


def test_the_cases_cover_the_kernels_edges():
    configs, max_u, max_c = kernel_configs()
    assert configs == fp.CONFIGS and (max_u, max_c) == (fp.MAX_U, fp.MAX_C)  # (the transcription's copy is the kernel's)
    widths = sorted({64} | {w for _, (w, _) in configs})  # (the wave and every workgroup width)
    finite, dead, seen, labels = set(), set(), set(), set()
    for name in fp.ALL_GPU_CASES:
        c, r = fp.case(name), fp.result(name)
        B, T, C = c.em.shape
        L = c.tokens.shape[-1]
        U = fp.max_length_of(c)
        seen.add(fp.config(U))
        labels.add(C)
        lens = np.minimum(np.maximum(np.asarray(c.lengths).reshape(B, -1), 0), L)
        frames = np.asarray(c.frames if c.frames is not None else [T] * B)
        for b in range(B):
            for k in range(lens.shape[1]):
                n = int(lens[b, k])
                (finite if np.isfinite(r.scores.reshape(B, -1)[b, k]) else dead).add(n)
                if n == U + 1:
                    assert np.isneginf(r.scores.reshape(B, -1)[b, k])
                if n == U and frames[b] >= n and name.startswith("wide"):
                    assert np.isfinite(r.scores.reshape(B, -1)[b, k]), (name, n)
    assert seen == {cfg for _, cfg in configs}
    assert {1, 2} <= finite and 0 in dead
    for w in widths:
        assert {w - 1, w, w + 1} <= finite, w
    # the lengths at which a lane's second, third and fourth position come in, and the limit and one above it
    assert {257, 512, 513, 768, 769, 1025, 2048, 2049, 3072, 3073, max_u} <= finite and max_u + 1 in dead
    assert labels >= {4, 5, 33}
    c = fp.case("c5-holes")
    assert np.isneginf(c.em).any() and np.isneginf(c.trans).any()
    fin = np.isfinite(fp.result("c5-holes").scores)
    assert fin.any() and not fin.all()
    assert np.asarray(fp.case("c33").lengths).dtype == np.int64


# ---- the entry points ----
def test_entry_points_exist(gtn):
    from gtn_amd import torch_loss
    assert callable(torch_loss.asg_score)
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    assert hasattr(lib, "gtn_asg_score_n") and hasattr(lib, "gtn_asg_score_grad_n")
    eng = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_amd.so"))
    for name in ("gtnx_batch_asg_score", "gtnx_batch_asg_score_grad", "gtnx_batch_asg_score_stats"):
        assert hasattr(eng, name), name
    assert callable(gtn.Batch.asg_score) and callable(gtn.Batch.asg_score_grad)
    calls, pairs = gtn.debug_asg_score_stats()
    assert calls >= 0 and pairs >= 0
    for header, name in (("include/gtn_amd.h", "gtnx_batch_asg_score_grad"), ("include/gtn/batch.h", "asgScoreGrad"),
                         ("include/gtn/batch.h", "asgScore"), ("gtn_amd/criteria/asg_criterion.h", "asgScoreBatch"),
                         ("gtn_amd/csrc/Makefile", "asg_score.hip")):
        with open(os.path.join(ROOT, header)) as f:
            assert name in f.read(), header


def test_argument_errors_come_before_the_device(gtn):
    """what the arguments alone decide is GTNX_INVALID_ARGUMENT (1) with or without a device; a batch that is not a
    native linear one, a frame count outside 0 .. M, too many labels and a table in host memory are reached on the
    device only"""
    import gtn_amd
    lib = gtn_amd._lib
    batch = gtn.Batch([gtn.linear_graph(2, 8)])
    p = ctypes.c_void_p
    score, grad = lib.gtnx_batch_asg_score, lib.gtnx_batch_asg_score_grad
    #            ems   frames table tokens stride lengths N  L  U  out...
    good = [batch._h, None, p(64), p(64), 4, p(64), 1, 4, 4]
    before = gtn.debug_asg_score_stats()

    def bad(i, v):
        a = list(good)
        a[i] = v
        return a
    refused = [bad(0, None), bad(2, None), bad(3, None), bad(5, None), bad(6, -1), bad(7, -1), bad(4, -1), bad(4, 3),
               bad(8, 0), bad(8, 4097), bad(8, -5)]
    for a in refused:
        assert score(*a, p(64)) == 1, a
        assert grad(*a, p(64), p(64), p(64)) == 1, a
    assert score(*good, None) == 1
    assert grad(*good, None, p(64), p(64)) == 1   # no weights
    assert grad(*good, p(64), None, None) == 1    # neither gradient
    # no pair: OK without a device (N == 0 here; a batch without elements has no handle to give)
    assert score(*bad(6, 0), p(64)) == 0
    assert grad(*bad(6, 0), p(64), p(64), None) == 0
    assert grad(*bad(6, 0), p(64), None, p(64)) == 0
    assert gtn.debug_asg_score_stats() == before  # (nothing launched)
    assert score(*bad(8, 0), p(64)) == 1
    lib.gtnx_last_error.restype = ctypes.c_char_p
    assert lib.gtnx_last_error().decode().startswith("[gtnx_batch_asg_score] max_length outside")
    with pytest.raises(ValueError, match="max_length outside"):
        batch.asg_score(64, 64, 64, 64, N=1, L=4, row_stride=4, max_length=0)
    with pytest.raises(ValueError, match="needs N, L and row_stride"):
        batch.asg_score(64, 64, 64, 64)
    with pytest.raises(ValueError, match="null weights"):
        batch.asg_score_grad(64, 64, 64, 0, 64, N=1, L=4, row_stride=4, max_length=4)
    with pytest.raises(ValueError, match="neither grad_out nor grad_table_out"):
        batch.asg_score_grad(64, 64, 64, 64, N=1, L=4, row_stride=4, max_length=4)
    with pytest.raises(ValueError, match="shorter than the rows' width"):
        batch.asg_score(64, 64, 64, 64, N=1, L=4, row_stride=3, max_length=4)


def test_torch_argument_checks():
    import torch
    from gtn_amd import torch_loss
    em = torch.zeros(2, 3, 8)
    tr = torch.zeros(8, 8)
    tok = torch.zeros(2, 2, 3, dtype=torch.int32)
    ln = torch.zeros(2, 2, dtype=torch.int32)
    for args, kw, msg in (((em.double(), tr, tok, ln), {}, "float32 tensor"), ((em[0], tr, tok, ln), {}, "float32 tensor"),
                          ((em, tr[:7], tok, ln), {}, r"transitions must be \[8, 8\]"),
                          ((em, tr, tok, ln), dict(start=torch.zeros(7)), r"start must be \[8\]"),
                          ((em, tr, tok.long(), ln), {}, "tokens must be an int32"),
                          ((em, tr, tok[:1], ln), {}, "tokens must be an int32"),
                          ((em, tr, tok, ln.float()), {}, "lengths must be an int32 or int64"),
                          ((em, tr, tok, ln[:, :1]), {}, "lengths must be an int32 or int64"),
                          ((em, tr, tok[:, 0], ln), {}, "lengths must be an int32 or int64"),
                          ((em, tr, tok, ln), dict(max_length=0), "max_length outside 1 .. 4096"),
                          ((em, tr, tok, ln), dict(max_length=4097), "max_length outside 1 .. 4096"),
                          ((em, tr, tok, ln), dict(input_lengths=[4, 1]), "input length outside 0 .. 3"),
                          ((em, tr, tok, ln), dict(input_lengths=[1]), "input lengths for a batch of 2")):
        with pytest.raises(ValueError, match=msg):
            torch_loss.asg_score(*args, **kw)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        torch_loss.asg_score(em, tr, tok, ln)
    assert "16384" in torch_loss.asg_score.__doc__


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU behaviour")
def test_asg_score_fails_loudly_without_gpu(gtn):
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    lib.gtn_asg_score_n.argtypes = ([ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 4 + [ctypes.c_int] * 3
                                    + [ctypes.c_void_p])
    lib.gtn_asg_score_n.restype = ctypes.c_int
    lib.gtn_criteria_last_error.restype = ctypes.c_char_p
    rc = lib.gtn_asg_score_n(None, 1, 2, 8, ctypes.c_void_p(64), None, ctypes.c_void_p(64), ctypes.c_void_p(64), 1, 2, 2,
                             ctypes.c_void_p(64))
    assert rc == -1 and "no HIP device" in lib.gtn_criteria_last_error().decode()
    with pytest.raises(RuntimeError, match="no HIP device"):
        gtn.Batch([gtn.linear_graph(2, 8)]).asg_score(64, 64, 64, 64, N=1, L=2, row_stride=2, max_length=2)
