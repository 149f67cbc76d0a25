"""ASG token alignment of device-resident hypotheses, the parts that need no GPU.  The float32 yardstick of
tests/asg_token_align_fp.py (which test_asg_token_align_gpu.py compares the kernel with bit for bit) is pinned to the
oracle's shortest_path over the built emissions o (forceAlign o transitions) lattice on integer-valued inputs (frame
labels identical, scores equal as floats, no path exactly where the oracle has none) and to two float64 forms on
continuous ones.  Every case the GPU file runs keeps the span invariants and the case list reaches every
instantiation of the kernel.  The entry points exist in every layer, refuse bad arguments before they ask for a device
with their whole texts, and fail loudly without one."""
import ctypes
import os
import re

import numpy as np
import pytest

import asg_token_align_fp as fp
from asg_align_fp import FP_CASES, asg_align_fp64, seeded_case
from conftest import ROOT, has_gpu
from oracle_lib import OGraph

NEG = -np.inf


def _graph(n_nodes, start, accept, arcs, sort=None):
    return OGraph.from_dict({
        "start": [int(i in start) for i in range(n_nodes)], "accept": [int(i in accept) for i in range(n_nodes)],
        "src": [a[0] for a in arcs], "dst": [a[1] for a in arcs], "il": [a[2] for a in arcs],
        "ol": [a[2] for a in arcs], "w": [float(a[3]) for a in arcs], "sort": sort})


def oracle_path(em, trans, start, target):
    """score and labels of the reference's viterbiPath over emissions o (forceAlign(target) o transitions), the
    transitions arc-sorted as asgTransitions leaves them (as tests/test_asg_align_cpu.py has it); (None, None) when no
    accepting path exists"""
    T, N = em.shape
    arcs = [(0, i + 1, i, start[i]) for i in range(N)]
    for i in range(N):
        for j in range(N):
            arcs.append((j + 1, i + 1, i, trans[i, j]))
    tr = _graph(N + 1, {0}, set(range(1, N + 1)), arcs, "i")
    U = len(target)
    arcs = []
    for l in range(1, U + 1):
        arcs.append((l - 1, l, int(target[l - 1]), 0.0))
        arcs.append((l, l, int(target[l - 1]), 0.0))
    o = OGraph.linear(T, N, em).compose(_graph(U + 1, {0}, {U}, arcs).compose(tr))
    path, has = o.shortest_path()
    if not has:
        return None, None
    d = o.to_dict()
    return o.shortest_distance(tropical=True), [d["il"][x] for x in path]


def tie_inputs(kind, rng, T, C):
    """integer-valued emissions [T, C], transitions [C, C] and start [C]"""
    if kind == "zero":
        return np.zeros((T, C), np.float32), np.zeros((C, C), np.float32), np.zeros(C, np.float32)
    if kind == "01":
        return rng.integers(0, 2, (T, C)).astype(np.float32), np.zeros((C, C), np.float32), np.zeros(C, np.float32)
    return (rng.integers(-2, 3, (T, C)).astype(np.float32), rng.integers(-1, 2, (C, C)).astype(np.float32),
            rng.integers(-1, 2, C).astype(np.float32))


@pytest.mark.parametrize("kind", ["zero", "01", "int"])
def test_yardstick_is_the_oracle_on_ties(kind):
    """U = 1 .. 6, T = 1 .. 13, 2 - 5 labels, half of the labels repeated: every combination, none left out"""
    rng = np.random.default_rng({"zero": 1, "01": 2, "int": 3}[kind])
    none = 0
    for U in range(1, 7):
        for T in range(1, 14):
            for rep in range(2):
                C = int(rng.integers(2, 6))
                y = fp.labels_of(rng, U, C, 0.5 * rep)
                em, trans, start = tie_inputs(kind, rng, T, C)
                row = np.concatenate([y, np.full(2, -1, np.int32)])
                r = fp.align_pair(em, fp.table_of(start, trans), row, U, T, 8)
                want_score, want = oracle_path(em, trans, start, y)
                if want is None:
                    none += 1
                    assert T < U
                    assert r.score == NEG and (r.frame_tokens == -1).all() and (r.starts == -1).all(), (kind, U, T, y)
                    continue
                assert r.score > NEG, (kind, U, T, y)
                assert y[r.frame_tokens[:T]].tolist() == want, (kind, U, T, y.tolist(), em.tolist())
                assert np.float32(r.score) == np.float32(want_score), (kind, U, T, y)
    assert none == 2 * 15  # (T < U: "no path" was seen, and nowhere else)


@pytest.mark.parametrize("seed,B,T,C,Umax,ragged", FP_CASES)
def test_yardstick_is_the_float64_forms_on_continuous_inputs(seed, B, T, C, Umax, ragged):
    """the seeds are ones on which float32 and float64 pick the same path on every utterance (a seed where rounding
    separated them would be replaced, not tolerated)"""
    em, trans, start, targets, frames = seeded_case(seed, B, T, C, Umax, ragged)
    table = fp.table_of(start, trans)
    for b in range(B):
        y = np.asarray(targets[b], np.int32)
        f = int(frames[b])
        r = fp.align_pair(em[b], table, y, len(y), f, Umax)
        labels, tokens, score = asg_align_fp64(em[b], trans, start, targets[b], f)
        assert (r.frame_tokens == tokens).all()
        assert y[r.frame_tokens[:f]].tolist() == labels[:f].tolist()
        score64, ft64 = fp.align_pair64(em[b], table, y, len(y), f)
        assert (r.frame_tokens[:f] == ft64).all() and score64 == score
        assert abs(float(r.score) - score) <= 1e-5 * max(1.0, abs(score))


def check_spans(case, res):
    B, M, _ = case.em.shape
    N, L = case.tokens.shape[1:]
    for b in range(B):
        T = M if case.frames is None else int(case.frames[b])
        for k in range(N):
            st, en, ft, ts = res.starts[b, k], res.ends[b, k], res.frame_tokens[b, k], res.token_scores[b, k]
            if not res.scores[b, k] > NEG:
                assert (st == -1).all() and (en == -1).all() and (ft == -1).all() and np.isneginf(ts).all()
                continue
            n = min(max(int(case.lengths[b, k]), 0), L)
            y = case.tokens[b, k, :n]
            assert n >= 1
            assert (st[n:] == -1).all() and (en[n:] == -1).all() and np.isneginf(ts[n:]).all() and (ft[T:] == -1).all()
            assert st[0] == 0 and en[n - 1] == T
            assert (en[:n - 1] == st[1:n]).all()
            assert (en[:n] - st[:n] >= 1).all()
            want = np.full(M, -1, np.int32)
            for i in range(n):
                want[st[i]:en[i]] = i
            assert (want == ft).all() and (ft[:T] >= 0).all()
            for i in range(n):
                x = case.em[b, st[i]:en[i], y[i]].astype(np.float64)
                # (n - 1 float32 additions: the textbook bound (n - 1) u sum |x| with u = 2^-24, doubled)
                assert abs(float(ts[i]) - np.sum(x)) <= (x.size - 1) * 2.0 ** -23 * np.sum(np.abs(x))


@pytest.mark.parametrize("name", fp.ALL_GPU_CASES)
def test_span_invariants(name):
    case, res = fp.case(name), fp.result(name)
    check_spans(case, res)
    assert (res.scores > NEG).any()  # (a case that aligns nothing shows nothing)


def test_the_contract_of_the_nopath_case():
    c, r = fp.case("nopath"), fp.result("nopath")
    fin = (r.scores > NEG).tolist()
    assert fin[0] == [True, True, False, True]                    # length 0: no path
    assert fin[1] == [False] * 4                                  # T_b == 0
    assert fin[2] == [False, True, False, False]                  # one frame too few; an exact fit; 0; too long
    assert fin[3] == [False, True, False, True]                   # a -inf column cuts every path of the first only
    assert fin[4] == [False] * 4                                  # tokens -1 and C; a negative length; one above L
    assert fin[5] == [True, True, False, False]                   # ... and a length above max_length
    assert fin[6] == [False, True, False, False]                  # a -inf transition
    assert fin[7] == [False, True, False, False]                  # a -inf start entry
    assert c.lengths[2, 0] == fp.NOPATH_FRAMES[2] + 1 and c.lengths[2, 1] == fp.NOPATH_FRAMES[2]
    assert c.lengths[5, 3] == c.max_length + 1 == fp.NOPATH_FRAMES[5]
    assert np.isneginf(c.trans[3, 4]) and np.isneginf(c.start[5]) and np.isneginf(c.trans).sum() == 1


def kernel_configs():
    """asg_score_config as gtn_amd/csrc/asg_score.hip has it (read as tests/test_asg_score_cpu.py reads it): ((bound on
    max_length, (width, per lane)), ...)"""
    with open(os.path.join(ROOT, "gtn_amd", "csrc", "asg_score.hip")) as f:
        body = f.read().split("void asg_score_config(")[1].split("\n}\n")[0]
    rows = [(int(u), (int(w), int(p))) for u, w, p in re.findall(r"U <= (\d+)\) wg = (\d+), per = (\d+);", body)]
    (w, p), = re.findall(r"else wg = (\d+), per = (\d+);", body)
    with open(os.path.join(ROOT, "gtn_amd", "csrc", "kernels.h")) as f:
        max_u = int(re.search(r"kAsgScoreMaxU = (\d+);", f.read()).group(1))
    return tuple(rows) + ((max_u, (int(w), int(p))),)


def test_the_cases_cover_the_kernels_edges():
    configs = kernel_configs()
    assert configs == fp.CONFIGS  # (the transcription's copy is the kernel's)
    with open(os.path.join(ROOT, "gtn_amd", "csrc", "asg_token_align.hip")) as f:
        text = f.read()
    assert "asg_score_config(a.U, &wg, &per)" in text  # (the new kernel takes its widths from there)
    for w, p in {cfg for _, cfg in configs}:
        assert f"fn<{w}, {p}>(a, st)" in text, (w, p)
    assert fp.WIDTHS == (1, 2, 63, 64, 65, 255, 256, 257, 768, 769, 1024, 1025, 2048, 2049, 4096)
    assert {fp.config(fp.case(f"width-{U}").max_length) for U in fp.WIDTHS} == {cfg for _, cfg in configs}
    for bound, _ in configs:  # (each bound and one above it, where there is one)
        assert bound in fp.WIDTHS and (bound == 4096 or bound + 1 in fp.WIDTHS)
    for U in fp.WIDTHS:
        c, r = fp.case(f"width-{U}"), fp.result(f"width-{U}")
        assert c.em.shape == (1, U + 3, 5) and c.tokens.shape == (1, 2, U) and c.max_length == U
        assert c.lengths.tolist() == [[U, U - 1]]
        assert r.scores[0, 0] > NEG and (r.scores[0, 1] > NEG) == (U > 1)
    assert fp.WORD_FRAMES == (1, 31, 32, 33, 63, 64, 65, 129)
    w = fp.case("words")
    assert w.frames.tolist() == list(fp.WORD_FRAMES) and (w.lengths[:, 0] == np.minimum(w.frames, 7)).all()
    d, rd = fp.case("descent"), fp.result("descent")
    assert fp.DESCENT_LENS == (32, 33, 64, 65, 129)
    for b, n in enumerate(fp.DESCENT_LENS):
        assert d.frames[b] == n and (d.lengths[b] == n).all()
        assert (rd.frame_tokens[b, :, :n] == np.arange(n)).all()  # one position a frame
    s, rs = fp.case("steady"), fp.result("steady")
    assert (s.lengths == 1).all() and all((rs.frame_tokens[b, 0, :f] == 0).all() for b, f in enumerate(fp.STEADY_FRAMES))
    for name, values in (("ties-zero", {0.0}), ("ties-01", {0.0, 1.0})):
        t = fp.case(name)
        assert set(fp.TIE_LENS) == set(t.lengths.reshape(-1).tolist()) == {5, 40, 200}
        for a in (t.em, t.trans, t.start):
            assert set(np.unique(a).tolist()) == values
        assert all((np.diff(t.tokens[b, k, :t.lengths[b, k]]) == 0).any() for b in range(2) for k in range(3))
    assert fp.ALPHABETS == (1, 2, 5, 33, 257, 300)
    for C in fp.ALPHABETS:
        assert fp.case(f"alphabet-{C}").em.shape[2] == C
    assert fp.ALIGN_LENS == (1, 64, 128, 511)
    for C in (8, 300):
        a = fp.case(f"align-c{C}")
        assert a.em.shape[2] == C and a.lengths.reshape(-1).tolist() == list(fp.ALIGN_LENS)
    assert 0 in fp.NOPATH_FRAMES


# ---- the entry points ----
def test_entry_points_exist(gtn):
    from gtn_amd import _capi, torch_loss
    assert callable(torch_loss.asg_token_align)
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    assert hasattr(lib, "gtn_asg_token_align_n")
    eng = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_amd.so"))
    for name in ("gtnx_batch_asg_token_align", "gtnx_batch_asg_token_align_stats"):
        assert hasattr(eng, name), name
        assert name in _capi.ALL_SYMBOLS
    assert callable(gtn.Batch.asg_token_align)
    calls, pairs = gtn.debug_asg_token_align_stats()
    assert calls >= 0 and pairs >= 0
    for header, name in (("include/gtn_amd.h", "gtnx_batch_asg_token_align"),
                         ("include/gtn_amd.h", "gtnx_batch_asg_token_align_stats"),
                         ("include/gtn/batch.h", "asgTokenAlign"),
                         ("gtn_amd/criteria/asg_criterion.h", "asgTokenAlignBatch"),
                         ("gtn_amd/csrc/kernels.h", "launch_asg_token_align"),
                         ("gtn_amd/csrc/batch.h", "batch_asg_token_align_stats")):
        with open(os.path.join(ROOT, header)) as f:
            assert name in f.read(), header


def test_argument_errors_come_before_the_device(gtn):
    """what the arguments alone decide is GTNX_INVALID_ARGUMENT (1) with its whole text, with or without a device"""
    import gtn_amd
    lib = gtn_amd._lib
    lib.gtnx_last_error.restype = ctypes.c_char_p
    batch = gtn.Batch([gtn.linear_graph(2, 8)])
    p = ctypes.c_void_p
    align = lib.gtnx_batch_asg_token_align
    #        0 ems     1 frames 2 table 3 tokens 4 stride 5 lengths 6 N 7 L 8 U 9 scores 10 starts 11 ends 12 tscores
    #        13 out_stride 14 frame tokens 15 frame_stride
    good = [batch._h, None, p(64), p(64), 4, p(64), 1, 4, 4, p(64), p(64), p(64), p(64), 4, p(64), 2]
    before = gtn.debug_asg_token_align_stats()
    outs = "null output pointer (scores, starts and ends are all written)"
    refused = [(2, None, "null table pointer"),
               (3, None, "null input pointer (tokens and lengths are both read)"),
               (5, None, "null input pointer (tokens and lengths are both read)"),
               (6, -1, "negative N or L"), (7, -1, "negative N or L"), (4, -1, "negative row stride"),
               (4, 3, "row_stride is shorter than the rows' width L"), (8, 0, "max_length outside 1 .. 4096"),
               (8, 4097, "max_length outside 1 .. 4096"), (8, -5, "max_length outside 1 .. 4096"), (9, None, outs),
               (10, None, outs), (11, None, outs), (13, 3, "out_stride is shorter than the rows' width L"),
               (13, -1, "negative row stride"), (15, -1, "negative row stride")]
    for i, v, text in refused:
        a = list(good)
        a[i] = v
        assert align(*a) == 1, (i, v)
        assert lib.gtnx_last_error().decode() == "[gtnx_batch_asg_token_align] " + text, (i, v)
    a = list(good)
    a[0] = None  # (refused where the handle is unwrapped, before the entry point's own checks)
    assert align(*a) == 1 and lib.gtnx_last_error().decode() == "null batch handle"
    # no pair: OK without a device (N == 0 here; a batch without elements has no handle to give)
    a = list(good)
    a[6] = 0
    assert align(*a) == 0
    assert gtn.debug_asg_token_align_stats() == before  # (nothing launched, nothing counted)
    with pytest.raises(ValueError, match="max_length outside"):
        batch.asg_token_align(64, 64, 64, 64, 64, table=64, N=1, L=4, row_stride=4, max_length=0)
    with pytest.raises(ValueError, match="needs N, L and row_stride"):
        batch.asg_token_align(64, 64, 64, 64, 64, table=64)
    with pytest.raises(ValueError, match="null table pointer"):
        batch.asg_token_align(64, 64, 64, 64, 64, N=1, L=4, row_stride=4, max_length=4)
    with pytest.raises(ValueError, match="null output pointer"):
        batch.asg_token_align(64, 64, 64, 0, 64, table=64, N=1, L=4, row_stride=4, max_length=4)
    with pytest.raises(ValueError, match="out_stride is shorter"):
        batch.asg_token_align(64, 64, 64, 64, 64, table=64, N=1, L=4, row_stride=4, max_length=4, out_stride=3)


def test_torch_argument_checks():
    import torch
    from gtn_amd import torch_loss
    em = torch.zeros(2, 3, 8)
    tr = torch.zeros(8, 8)
    tok = torch.zeros(2, 2, 3, dtype=torch.int32)
    ln = torch.zeros(2, 2, dtype=torch.int32)
    for args, kw, msg in (((em.double(), tr, tok, ln), {}, "float32 tensor"), ((em[0], tr, tok, ln), {}, "float32 tensor"),
                          ((em, tr[:7], tok, ln), {}, "transitions must be"),
                          ((em, tr, tok, ln), dict(start=torch.zeros(7)), "start must be"),
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
            torch_loss.asg_token_align(*args, **kw)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        torch_loss.asg_token_align(em, tr, tok, ln)
    assert "asg_forced_align" in torch_loss.asg_token_align.__doc__


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU behaviour")
def test_asg_token_align_fails_loudly_without_gpu(gtn):
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    lib.gtn_asg_token_align_n.argtypes = ([ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 4
                                          + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 5)
    lib.gtn_asg_token_align_n.restype = ctypes.c_int
    lib.gtn_criteria_last_error.restype = ctypes.c_char_p
    q = ctypes.c_void_p(64)
    rc = lib.gtn_asg_token_align_n(None, 1, 2, 8, q, None, q, q, 1, 2, 2, q, q, q, None, None)
    assert rc == -1 and "no HIP device" in lib.gtn_criteria_last_error().decode()
    with pytest.raises(RuntimeError, match="no HIP device"):
        gtn.Batch([gtn.linear_graph(2, 8)]).asg_token_align(64, 64, 64, 64, 64, table=64, N=1, L=2, row_stride=2,
                                                            max_length=2)
