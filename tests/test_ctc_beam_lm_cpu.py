"""CTC prefix beam search with a bigram table fused in, the parts that need no GPU.  The float64 yardstick of
tests/ctc_beam_lm_fp.py (which test_ctc_beam_lm_gpu.py judges the kernel by) is pinned to a brute-force enumeration --
every label sequence, exact CTC score plus L, sorted -- with -inf entries in the table, and to ctc_beam_fp.beam_search at
alpha = beta = 0 in all three float forms.  Every case the GPU file runs vets; the re-created cases re-create; the entry
points exist in every layer and refuse bad arguments before they ask for a device."""
import ctypes
import itertools
import math
import os

import numpy as np
import pytest

import ctc_beam_fp as fp
import ctc_beam_lm_fp as lfp
from conftest import ROOT


def brute_force_lm(em, blank, w, alpha, beta):
    """{label sequence: (acoustic log score over all C^T alignments, L)} in float64; sequences with a forbidden bigram
    or first label are left out"""
    T, C = em.shape
    x = em.astype(np.float64)
    am = {}
    for path in itertools.product(range(C), repeat=T):
        y = tuple(c for t, c in enumerate(path) if c != blank and (t == 0 or c != path[t - 1]))
        s = float(sum(x[t, c] for t, c in enumerate(path)))
        am[y] = s if y not in am else max(am[y], s) + math.log1p(math.exp(-abs(am[y] - s)))
    alpha, beta = float(np.float32(alpha)), float(np.float32(beta))
    out = {}
    for y, s in am.items():
        L, prev = 0.0, -1
        for c in y:
            L += alpha * float(w[c] if prev < 0 else w[C + c * C + prev]) + beta
            prev = c
        if math.isfinite(L):
            out[y] = (s, L)
    return out


@pytest.mark.parametrize("T,C,blank", [(1, 2, 0), (2, 3, 0), (3, 3, 2), (3, 4, 1), (4, 3, 0)])
def test_unpruned_search_is_the_enumeration(T, C, blank):
    em = fp.continuous_case(10 * T + C, 1, T, C)[0]
    w = lfp.table_case(10 * T + C, C, holes=0.15)
    if not np.isneginf(w).any():
        w[C + (0 if blank else 1) * C + (0 if blank else 1)] = -np.inf  # (a tiny table: at least one hole)
    want = brute_force_lm(em, blank, w, 0.7, -0.3)
    assert 0 < len(want) <= 64
    got = lfp.beam_search_lm(em, blank, 64, C, w, 0.7, -0.3, "f64")
    assert [y for y, _, _ in got] == sorted(want, key=lambda y: -(want[y][0] + want[y][1]))
    for y, total, am in got:
        assert abs(am - want[y][0]) <= 1e-9 and abs(total - (want[y][0] + want[y][1])) <= 1e-9, (y, total, am, want[y])


@pytest.mark.parametrize("form", fp.FORMS)
def test_zero_weight_and_bonus_is_the_search_without_a_table(form):
    for seed, (T, C, blank, W, K) in enumerate([(40, 6, 0, 8, 4), (65, 5, 4, 4, 3), (12, 29, 0, 16, 16), (3, 3, 1, 64, 3)]):
        em = fp.continuous_case(seed + 30, 2, T, C)
        w = lfp.table_case(seed, C)
        for b, frames in ((0, None), (1, T - 1)):
            plain = fp.beam_search(em[b], blank, W, K, form, frames)
            got = lfp.beam_search_lm(em[b], blank, W, K, w, 0.0, 0.0, form, frames)
            assert [(y, s) for y, s, _ in got] == plain and [(y, a) for y, _, a in got] == plain
            assert all(s.tobytes() == p[1].tobytes() for (_, s, _), p in zip(got, plain))


def test_a_forbidden_first_label_and_bigram_never_come_back():
    C, T = 4, 3  # (at most 40 label sequences: a beam of 64 prunes nothing)
    em = fp.continuous_case(3, 1, T, C)[0]
    w = np.zeros(C + C * C, np.float32)
    w[2] = -np.inf               # 2 may not begin a sequence
    w[C + 3 * C + 1] = -np.inf   # 1 may not be followed by 3
    got = lfp.beam_search_lm(em, 0, 64, C, w, 1.0, 0.0, "f64")
    free = lfp.beam_search_lm(em, 0, 64, C, np.zeros_like(w), 1.0, 0.0, "f64")
    bad = lambda y: (len(y) > 0 and y[0] == 2) or any(a == 1 and b == 3 for a, b in zip(y, y[1:]))
    assert any(bad(y) for y, _, _ in free) and not any(bad(y) for y, _, _ in got)
    assert sorted(y for y, _, _ in got) == sorted(y for y, _, _ in free if not bad(y))
    w[:C] = -np.inf  # nothing may begin: the empty prefix alone, with the all-blank path's score
    only = lfp.beam_search_lm(em, 0, 64, C, w, 1.0, 0.0, "f64")
    assert [y for y, _, _ in only] == [()]
    assert abs(only[0][1] - em[:, 0].astype(np.float64).sum()) <= 1e-12 and only[0][1] == only[0][2]


def test_the_table_changes_the_first_hypothesis():
    """what the issue records for these cases: every utterance's 1-best differs from the search without a table, 42 of
    65 in the (65, 3, 5) case"""
    for case in lfp.SHAPE_CASES:
        seed, B, T, C, blank, W, K, nbest, frames, holes = case
        em, w, res, _ = lfp.results_of(case)
        differ = sum(res["f64"][b][0][0] != fp.beam_search(em[b], blank, W, K, "f64")[0][0] for b in range(B))
        assert differ == (42 if B == 65 else B), (case, differ)


@pytest.mark.parametrize("case", lfp.ALL_GPU_CASES, ids=lambda c: "-".join(str(v) for v in c[:8]))
def test_every_gpu_case_vets(case):
    seed, B, T, C, blank, W, K, nbest, frames, holes = case
    assert nbest <= 4 or T <= 3
    assert nbest <= W
    em, w, res, again = lfp.results_of(case)
    ok, err, gap = lfp.vet_lm(res, nbest)
    print(f"[ctc_beam_lm] {case}: err {err:.3g} smallest gap {gap:.3g} re-created {again}")
    assert ok, (err, gap)
    if holes:
        assert 0.15 <= np.isneginf(w).mean() <= 0.30


@pytest.mark.parametrize("case", lfp.RECREATED_CASES, ids=lambda c: "-".join(str(v) for v in c[:8]))
def test_recreated_cases_recreate(case):
    assert len(lfp.RECREATED_CASES) >= 2
    assert lfp.results_of(case)[3] > 0


def test_ragged_and_constrained_cases_are_what_they_say():
    assert lfp.RAGGED_CASE[8] == (40, 1, 0, 39, 33, 2, 40)
    assert lfp.CONSTRAINED_CASE[9] > 0


def test_entry_points_exist(gtn):
    import inspect
    from gtn_amd import torch_loss
    for name in ("transitions", "start", "lm_weight", "insertion_bonus", "return_am_scores"):
        assert name in inspect.signature(torch_loss.ctc_beam_decode).parameters
    for name in ("lm", "lm_weight", "insertion_bonus", "am_scores_out"):
        assert name in inspect.signature(gtn.Batch.ctc_beam_decode).parameters
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    assert hasattr(lib, "gtn_ctc_beam_decode_lm_n")
    eng = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_amd.so"))
    assert hasattr(eng, "gtnx_batch_ctc_beam_decode_lm")
    for header, name in (("include/gtn_amd.h", "gtnx_batch_ctc_beam_decode_lm"), ("include/gtn/batch.h", "lmDevice"),
                         ("gtn_amd/criteria/ctc_criterion.h", "lmDev")):
        with open(os.path.join(ROOT, header)) as f:
            assert name in f.read(), header


def test_argument_errors_come_before_the_device(gtn):
    """what the arguments alone decide is refused as an invalid argument, with or without a device: a weight or bonus
    that is not finite, a null table, nbest above beam_size (a table on the host is reached on the device only:
    test_ctc_beam_lm_gpu.py)"""
    import torch
    import gtn_amd
    from gtn_amd import torch_loss
    batch = gtn.Batch([gtn.linear_graph(2, 8)])
    inf, nan = float("inf"), float("nan")
    for kw, msg in ((dict(lm=64, lm_weight=nan), "must be finite"), (dict(lm=64, lm_weight=inf), "must be finite"),
                    (dict(lm=64, insertion_bonus=-inf), "must be finite"), (dict(lm=64, insertion_bonus=nan), "must be finite"),
                    (dict(lm=0), "null language model table"), (dict(lm=64, nbest=17), "nbest above beam_size"),
                    (dict(lm=64, beam_size=2, nbest=3), "nbest above beam_size"),
                    (dict(lm=64, am_scores_out=64, beam_size=65), "beam_size outside"),
                    (dict(am_scores_out=64), "am_scores_out needs lm")):
        with pytest.raises(ValueError, match=msg):
            batch.ctc_beam_decode(64, 64, 64, row_stride=2, **kw)
    with pytest.raises(ValueError, match="null output pointer"):
        batch.ctc_beam_decode(64, 64, 0, row_stride=2, lm=64)
    for lm, msg in ((torch.zeros(72, dtype=torch.float64), "lm must be a float32"), (torch.zeros(8, 9), "lm must be a float32"),
                    (torch.zeros(72), "lm must be a float32")):  # (the last: not a CUDA tensor)
        with pytest.raises(ValueError, match=msg):
            batch.ctc_beam_decode(64, 64, 64, row_stride=2, lm=lm)
    with pytest.raises(ValueError, match="am_scores_out must be a float32"):
        batch.ctc_beam_decode(64, 64, 64, row_stride=2, lm=64, am_scores_out=torch.zeros(1, 1, dtype=torch.int32))
    # the C ABI itself: 1 is GTNX_INVALID_ARGUMENT
    p = ctypes.c_void_p
    call = gtn_amd._lib.gtnx_batch_ctc_beam_decode_lm
    assert call(batch._h, None, 0, 16, 16, 1, None, 1.0, 0.0, p(64), 2, p(64), p(64), None) == 1
    assert call(batch._h, None, 0, 16, 16, 1, p(64), nan, 0.0, p(64), 2, p(64), p(64), None) == 1
    assert call(batch._h, None, 0, 16, 16, 1, p(64), 1.0, inf, p(64), 2, p(64), p(64), p(64)) == 1
    assert call(batch._h, None, 0, 16, 16, 17, p(64), 1.0, 0.0, p(64), 2, p(64), p(64), None) == 1
    assert call(batch._h, None, 0, 16, 16, 1, p(64), 1.0, 0.0, p(64), 2, p(64), None, None) == 1
    assert call(None, None, 0, 16, 16, 1, p(64), 1.0, 0.0, p(64), 2, p(64), p(64), None) == 1
    em = torch.zeros(2, 3, 8)
    tr = torch.zeros(8, 8)
    for kw, msg in ((dict(transitions=tr, lm_weight=nan), "must be finite"),
                    (dict(transitions=tr, insertion_bonus=inf), "must be finite"),
                    (dict(transitions=torch.zeros(8, 7)), r"transitions must be a tensor \[8, 8\]"),
                    (dict(transitions=torch.zeros(64)), r"transitions must be a tensor \[8, 8\]"),
                    (dict(transitions=tr, start=torch.zeros(7)), r"start must be a tensor \[8\]"),
                    (dict(transitions=tr, beam_size=4, nbest=5), "nbest outside")):
        with pytest.raises(ValueError, match=msg):
            torch_loss.ctc_beam_decode(em, **kw)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        torch_loss.ctc_beam_decode(em, transitions=tr)
