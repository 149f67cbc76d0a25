"""CTC token alignment of device-resident hypotheses, the parts that need no GPU.  The float32 yardstick of
tests/ctc_token_align_fp.py (which test_ctc_token_align_gpu.py compares the kernel with bit for bit) is pinned three
times: to the oracle's shortest_path on tie-heavy integer emissions (labels identical, scores equal as floats, no path
exactly where the oracle has none), to ctc_align_fp64 on continuous ones, and -- for tokens that include `blank` as a
label, which the oracle's route does not cover -- to an enumeration of all alignments.  Every case the GPU file runs
keeps the span invariants.  The entry points exist in every layer, refuse bad arguments before they ask for a device,
and fail loudly without one."""
import ctypes
import itertools
import os

import numpy as np
import pytest

import ctc_token_align_fp as fp
import graphgen as gg
from conftest import ROOT, has_gpu
from ctc_align_fp import FP_CASES, ctc_align_fp64, seeded_case
from oracle_lib import OGraph

NEG = -np.inf


def oracle_path(em, target, blank=0):
    """score and labels of the reference's viterbiPath over the built lattice (as tests/test_align_cpu.py has it);
    (None, None) when no accepting path exists"""
    T, C = em.shape
    a = OGraph.from_dict(gg.ctc_target_graph(list(target), blank))
    b = OGraph.linear(T, C, em)
    o = a.compose(b, "intersect")
    arcs, has = o.shortest_path()
    if not has:
        return None, None
    d = o.to_dict()
    return o.shortest_distance(tropical=True), [d["il"][x] for x in arcs]


def frame_labels(r, y, blank, T):
    return [int(y[i]) if i >= 0 else blank for i in r.frame_tokens[:T]]


def tie_emissions(kind, rng, T, C):
    if kind == "zero":
        return np.zeros((T, C), np.float32)
    lo, hi = (-2, 2) if kind == "pm2" else (0, 1)
    return rng.integers(lo, hi + 1, (T, C)).astype(np.float32)


@pytest.mark.parametrize("kind", ["zero", "pm2", "01"])
def test_yardstick_is_the_oracle_on_ties(kind):
    rng = np.random.default_rng({"zero": 1, "pm2": 2, "01": 3}[kind])
    none = 0
    for U in range(0, 7):
        for T in range(1, 14):
            for rep in range(2):
                C = int(rng.integers(2, 6))
                y = rng.integers(1, C, U).astype(np.int32)
                em = tie_emissions(kind, rng, T, C)
                row = np.concatenate([y, np.full(2, -1, np.int32)])
                r = fp.align_pair(em, row, U, 0, T, 8)
                want_score, want = oracle_path(em, y)
                if want is None:
                    none += 1
                    assert r.score == NEG and (r.frame_tokens == -1).all() and (r.starts == -1).all(), (kind, U, T, y)
                    continue
                assert r.score > NEG, (kind, U, T, y)
                assert frame_labels(r, y, 0, T) == want, (kind, U, T, y.tolist(), em.tolist())
                assert np.float32(r.score) == np.float32(want_score), (kind, U, T, y)
    assert none > 10  # ("no path" was seen)


@pytest.mark.parametrize("seed,B,T,C,Umax,ragged", FP_CASES)
def test_yardstick_is_ctc_align_fp64_on_continuous_inputs(seed, B, T, C, Umax, ragged):
    em, targets, frames = seeded_case(seed, B, T, C, Umax, ragged)
    for b in range(B):
        y = np.asarray(targets[b], np.int32)
        labels, tokens, score = ctc_align_fp64(em[b], targets[b], 0, int(frames[b]))
        r = fp.align_pair(em[b], y, len(y), 0, int(frames[b]), Umax)
        assert (r.frame_tokens == tokens).all()
        f = int(frames[b])
        assert frame_labels(r, y, 0, f) == labels[:f].tolist()
        assert abs(float(r.score) - score) <= 1e-5 * max(1.0, abs(score))


def enumerate_alignments(em, y, blank):
    """every state path of ctcGraph(y, blank) over T frames with its float64 score: (score, frame token indices)"""
    T = em.shape[0]
    S = 2 * len(y) + 1
    lab = [int(y[(s - 1) // 2]) if s % 2 else blank for s in range(S)]
    out = []

    def go(t, s, score, path):
        if t == T:
            if s >= S - 2:
                out.append((score, list(path)))
            return
        for d in (0, 1, 2):
            n = s + d
            if n >= S or (d == 2 and not (n % 2 and n > 1 and y[n // 2] != y[n // 2 - 1])):
                continue
            path.append((n - 1) // 2 if n % 2 else -1)
            go(t + 1, n, score + float(em[t, lab[n]]), path)
            path.pop()
    go(0, 0, 0.0, [])
    return out


def test_yardstick_is_the_enumeration_with_blank_among_the_tokens():
    rng = np.random.default_rng(5)
    seen = 0
    for trial in range(60):
        C = int(rng.integers(2, 4))
        blank = int(rng.integers(0, C))
        T = int(rng.integers(1, 7))
        U = int(rng.integers(0, 4))
        y = rng.integers(0, C, U).astype(np.int32)
        em = (rng.integers(-2, 3, (T, C)) if trial % 2 else rng.normal(0, 2, (T, C))).astype(np.float32)
        r = fp.align_pair(em, y, U, blank, T, 4)
        paths = enumerate_alignments(em, y, blank)
        if not paths:
            assert r.score == NEG
            continue
        seen += int((y == blank).any())
        best = max(s for s, _ in paths)
        assert abs(float(r.score) - best) <= 1e-5 * max(1.0, abs(best))
        mine = r.frame_tokens[:T].tolist()
        hit = [s for s, p in paths if p == mine]
        assert len(hit) >= 1, "the returned path is no alignment of y"
        assert abs(hit[0] - float(r.score)) <= 1e-5 * max(1.0, abs(best))
    assert seen >= 10


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
            assert (st[n:] == -1).all() and (en[n:] == -1).all() and np.isneginf(ts[n:]).all() and (ft[T:] == -1).all()
            assert (np.diff(st[:n]) > 0).all()
            assert (st[:n] < en[:n]).all()
            if n:
                assert st[0] >= 0 and en[n - 1] <= T
            for i in range(n - 1):
                assert en[i] <= st[i + 1]
                if y[i] == y[i + 1]:
                    assert en[i] < st[i + 1]
            want = np.full(M, -1, np.int32)
            for i in range(n):
                want[st[i]:en[i]] = i
            assert (want == ft).all()
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
    assert fin[0] == [True] * 4
    assert fin[1] == [False] * 4                                  # T_b == 0
    assert fin[2] == [False, False, True, True]                   # one frame too few twice; the empty one; an exact fit
    assert fin[3][0] is False and fin[3][1] is True               # a -inf column cuts every path of the first only
    assert fin[4] == [False, False, True, False]                  # tokens -1 and C; a negative length; one above L
    assert fin[5][3] is False and fin[5][2] is True               # a length above max_length; the empty sequence
    assert fp.frames_needed(c.tokens[2, 0, :7]) == fp.NOPATH_FRAMES[2] + 1
    empty = np.float32(0)  # the empty sequence: all blanks, added frame by frame
    for t in range(fp.NOPATH_FRAMES[4]):
        empty = np.float32(empty + c.em[4, t, c.blank])
    assert r.scores[4, 2] == empty
    assert (r.starts[4, 2] == -1).all() and (r.frame_tokens[4, 2] == -1).all()


def test_the_cases_cover_the_kernels_edges():
    configs = {fp.config(fp.case(f"width-{U}").max_length) for U in fp.WIDTHS}
    assert configs == {(64, 1), (256, 1), (256, 3), (1024, 1), (1024, 2), (1024, 4), (1024, 9)}
    for U in fp.WIDTHS:
        c = fp.case(f"width-{U}")
        assert c.lengths.max() == U == c.max_length and c.tokens.shape[0] * c.tokens.shape[1] <= 4
        assert c.em.shape[1] <= max(fp.frames_needed(c.tokens[0, k, :c.lengths[0, k]]) for k in range(2)) + 3
    assert fp.WORD_FRAMES == (1, 15, 16, 17, 63, 64, 65, 129)
    w = fp.case("words")
    assert {0, 1} <= set(w.lengths.reshape(-1).tolist())
    d, rd = fp.case("descent"), fp.result("descent")
    for b, n in enumerate(fp.DESCENT_LENS):
        assert d.frames[b] == n and (rd.frame_tokens[b, :, :n] == np.arange(n)).all()  # two states a frame
    t = fp.case("ties")
    assert set(fp.TIE_LENS) == set(t.lengths.reshape(-1).tolist()) and (t.em[0] == 0).all()
    assert set(np.unique(t.em[1]).tolist()) == {0.0, 1.0}
    assert any(fp.frames_needed(t.tokens[b, k, :t.lengths[b, k]]) > t.lengths[b, k] for b in range(2) for k in range(3))
    tb = fp.case("ties-blank-tokens")
    assert (tb.tokens[:, :, :5] == tb.blank).any()
    assert 0 in fp.NOPATH_FRAMES


# ---- the entry points ----
def test_entry_points_exist(gtn):
    from gtn_amd import torch_loss
    assert callable(torch_loss.ctc_token_align)
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    assert hasattr(lib, "gtn_ctc_token_align_n")
    eng = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_amd.so"))
    for name in ("gtnx_batch_ctc_token_align", "gtnx_batch_ctc_token_align_stats"):
        assert hasattr(eng, name), name
    assert callable(gtn.Batch.ctc_token_align)
    calls, pairs = gtn.debug_ctc_token_align_stats()
    assert calls >= 0 and pairs >= 0
    for header, name in (("include/gtn_amd.h", "gtnx_batch_ctc_token_align"), ("include/gtn/batch.h", "ctcTokenAlign"),
                         ("gtn_amd/criteria/ctc_criterion.h", "ctcTokenAlignBatch")):
        with open(os.path.join(ROOT, header)) as f:
            assert name in f.read(), header


def test_argument_errors_come_before_the_device(gtn):
    """what the arguments alone decide is GTNX_INVALID_ARGUMENT (1) with or without a device"""
    import gtn_amd
    lib = gtn_amd._lib
    batch = gtn.Batch([gtn.linear_graph(2, 8)])
    p = ctypes.c_void_p
    align = lib.gtnx_batch_ctc_token_align
    #        0 ems     1 frames 2 blank 3 tokens 4 stride 5 lengths 6 N 7 L 8 U 9 scores 10 starts 11 ends 12 tscores
    #        13 out_stride 14 frame tokens 15 frame_stride
    good = [batch._h, None, 0, p(64), 4, p(64), 1, 4, 4, p(64), p(64), p(64), p(64), 4, p(64), 2]
    before = gtn.debug_ctc_token_align_stats()

    def bad(i, v):
        a = list(good)
        a[i] = v
        return a
    refused = [bad(0, None), bad(3, None), bad(5, None), bad(6, -1), bad(7, -1), bad(4, -1), bad(2, -1), bad(4, 3),
               bad(8, 0), bad(8, 4097), bad(8, -5), bad(9, None), bad(10, None), bad(11, None), bad(13, 3), bad(13, -1),
               bad(15, -1)]
    for a in refused:
        assert align(*a) == 1, a
    # no pair: OK without a device (N == 0 here; a batch without elements has no handle to give)
    assert align(*bad(6, 0)) == 0
    assert gtn.debug_ctc_token_align_stats() == before  # (nothing launched)
    with pytest.raises(ValueError, match="max_length outside"):
        batch.ctc_token_align(64, 64, 64, 64, 64, N=1, L=4, row_stride=4, max_length=0)
    with pytest.raises(ValueError, match="needs N, L and row_stride"):
        batch.ctc_token_align(64, 64, 64, 64, 64)
    with pytest.raises(ValueError, match="null output pointer"):
        batch.ctc_token_align(64, 64, 64, 0, 64, N=1, L=4, row_stride=4, max_length=4)
    with pytest.raises(ValueError, match="out_stride is shorter"):
        batch.ctc_token_align(64, 64, 64, 64, 64, N=1, L=4, row_stride=4, max_length=4, out_stride=3)


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
            torch_loss.ctc_token_align(*args, **kw)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        torch_loss.ctc_token_align(em, tok, ln)
    assert "empty sequence" in torch_loss.ctc_token_align.__doc__


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU behaviour")
def test_ctc_token_align_fails_loudly_without_gpu(gtn):
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    lib.gtn_ctc_token_align_n.argtypes = ([ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3
                                          + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 5)
    lib.gtn_ctc_token_align_n.restype = ctypes.c_int
    lib.gtn_criteria_last_error.restype = ctypes.c_char_p
    q = ctypes.c_void_p(64)
    rc = lib.gtn_ctc_token_align_n(None, 1, 2, 8, 0, None, q, q, 1, 2, 2, q, q, q, None, None)
    assert rc == -1 and "no HIP device" in lib.gtn_criteria_last_error().decode()
    with pytest.raises(RuntimeError, match="no HIP device"):
        gtn.Batch([gtn.linear_graph(2, 8)]).ctc_token_align(64, 64, 64, 64, 64, N=1, L=2, row_stride=2, max_length=2)
