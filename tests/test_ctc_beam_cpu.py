"""CTC prefix beam search, the parts that need no GPU.  The float64 yardstick of tests/ctc_beam_fp.py (which
test_ctc_beam_gpu.py judges the kernels by) is pinned twice on cases where nothing is pruned: to a brute-force
enumeration of all C^T alignments (every label sequence, the argmax first, scores to 1e-9) and to the oracle's
forwardScore(ctcTarget(y) o linearGraph) (1e-4 max(1, |score|), the bound the CPU tests give that float32 oracle).
Pruning is shown to be real; every case the GPU file runs vets; the rules of the contract one by one; the entry points
exist in every layer, refuse bad arguments before they ask for a device, and fail loudly without one."""
import ctypes
import itertools
import math
import os

import numpy as np
import pytest

import ctc_beam_fp as fp
from conftest import ROOT, has_gpu
from oracle_lib import OGraph, lib as oracle

NEG = -np.inf


def brute_force(em, blank):
    """{label sequence: log of the summed probability of its alignments} over all C^T alignments, float64"""
    T, C = em.shape
    x = em.astype(np.float64)
    out = {}
    for path in itertools.product(range(C), repeat=T):
        y = tuple(c for t, c in enumerate(path) if c != blank and (t == 0 or c != path[t - 1]))
        s = float(sum(x[t, c] for t, c in enumerate(path)))
        out[y] = s if y not in out else max(out[y], s) + math.log1p(math.exp(-abs(out[y] - s)))
    return out


def oracle_score(em, y, blank):
    """forwardScore(ctcTarget(y) intersected with linearGraph(T, C)) by the oracle (float32)"""
    T, C = em.shape
    tg = np.ascontiguousarray(y, dtype=np.int32)
    ctc = OGraph(oracle().og_ctc_graph(tg.ctypes.data, int(tg.size), int(blank), 1))
    return ctc.compose(OGraph.linear(T, C, em), "intersect").shortest_distance(tropical=False)


@pytest.mark.parametrize("T,C", [(1, 2), (3, 3), (4, 3), (5, 2), (4, 4), (6, 3)])
@pytest.mark.parametrize("blank", ["first", "last"])
def test_unpruned_search_is_the_enumeration_and_the_oracle(T, C, blank):
    blank = 0 if blank == "first" else C - 1
    em = fp.continuous_case(10 * T + C, 1, T, C)[0]
    want = brute_force(em, blank)
    assert len(want) <= 64
    got = fp.beam_search(em, blank, 64, C, "f64")
    assert sorted(y for y, _ in got) == sorted(want)
    assert got[0][0] == max(want, key=want.get)
    scores = [s for _, s in got]
    assert scores == sorted(scores, reverse=True)
    for y, s in got:
        assert abs(s - want[y]) <= 1e-9, (y, s, want[y])
        ref = oracle_score(em, y, blank)
        assert abs(s - ref) <= 1e-4 * max(1.0, abs(s)), (y, s, ref)


def _first(em, blank, W, K):
    return fp.beam_search(em, blank, W, K, "f64")[0][0]


def test_a_cutoff_of_one_label_changes_the_first_hypothesis():
    """the blank is the best label of both frames, so cutoff_top_n = 1 offers nothing else: '' wins with 0.16 where
    the exhaustive run finds 'a' with 0.32 * 0.32 + 2 * 0.32 * 0.4"""
    em = np.log(np.array([[0.4, 0.32, 0.28], [0.4, 0.32, 0.28]])).astype(np.float32)
    assert _first(em, 0, 64, 3) == (1,)
    assert _first(em, 0, 64, 1) == ()


def test_a_beam_of_two_changes_the_first_hypothesis():
    """searched on the host: a seeded case whose exhaustive winner a beam of 2 does not reach"""
    seed, T, C = W2_CASE
    em = fp.continuous_case(seed, 1, T, C)[0]
    assert _first(em, 0, 2, C) != _first(em, 0, 64, C)


def _find_w2_case():
    for seed in range(1, 2000):
        for T, C in ((4, 3), (5, 3), (4, 4)):
            em = fp.continuous_case(seed, 1, T, C)[0]
            if _first(em, 0, 2, C) != _first(em, 0, 64, C):
                return seed, T, C


W2_CASE = (3, 4, 3)  # (seed, T, C): the first that `python tests/test_ctc_beam_cpu.py` finds


@pytest.mark.parametrize("case", fp.ALL_GPU_CASES, ids=lambda c: "-".join(str(v) for v in c[:9]))
def test_every_gpu_case_vets(case):
    kind, seed, B, T, C, blank, W, K, nbest, frames = case
    assert nbest <= 4 or T <= 3
    assert nbest <= W
    _, res = fp.results_of(case)
    ok, err, gap = fp.vet(res, nbest)
    print(f"[ctc_beam] {case}: err {err:.3g} smallest gap {gap:.3g}")
    assert ok, (err, gap)


@pytest.mark.parametrize("case", fp.RECREATED_CASES, ids=lambda c: "-".join(str(v) for v in c[:9]))
def test_recreated_prefix_cases_need_exact_identity(case):
    """knowing a prefix by the number its node got when it was created gets these cases wrong: a prefix that left the
    list and was created again has a new number, its child that stayed is no longer merged with, and the list holds the
    same tokens twice"""
    kind, seed, B, T, C, blank, W, K, nbest, frames = case
    em, res = fp.results_of(case)
    wrong = 0
    for b in range(B):
        model = fp.beam_search(em[b], blank, W, K, "f64", fresh_nodes=True)
        exact = res["f64"][b]
        assert len(set(y for y, _ in exact)) == len(exact)
        wrong += ([y for y, _ in model[:nbest]] != [y for y, _ in exact[:nbest]]
                  or any(abs(m[1] - e[1]) > 1e-3 for m, e in zip(model[:nbest], exact[:nbest])))
    assert wrong > 0


def test_integer_cases_are_exact_at_one_frame():
    """T = 1: every score is an entry of the row, so ties are exact and the three forms are one"""
    em = fp.integer_case(3, 65, 1, 29)
    for b in range(65):
        got = [fp.beam_search(em[b], 0, 8, 3, f) for f in fp.FORMS]
        assert got[0] == got[1] == got[2]


def test_top_k_ties_go_to_the_smaller_label():
    row = np.array([0, 2, 2, 1, 2, 1], np.float32)
    assert fp.token_set(row, 2, 0)[0].tolist() == [1, 2, 0]
    assert fp.token_set(row, 4, 0)[0].tolist() == [1, 2, 4, 3, 0]
    assert fp.token_set(row, 32, 3)[0].tolist() == [1, 2, 4, 3, 5, 0]
    # the hypotheses of one frame: the stay first, then extensions by (score, label)
    got = fp.beam_search(row[None], 0, 8, 4, "f64")
    assert got == [((1,), 2.0), ((2,), 2.0), ((4,), 2.0), ((3,), 1.0), ((), 0.0)]
    assert fp.beam_search(np.zeros((1, 4), np.float32), 1, 8, 4, "f64") == [((), 0.0), ((0,), 0.0), ((2,), 0.0),
                                                                             ((3,), 0.0)]


def test_nan_and_minus_infinity_are_never_chosen():
    row = np.array([np.nan, NEG, 1.0, np.nan, -2.0, NEG], np.float32)
    assert fp.token_set(row, 4, 2)[0].tolist() == [2, 4]
    assert fp.token_set(row, 1, 4)[0].tolist() == [2, 4]   # blank appended: finite and outside the top K
    assert fp.token_set(row, 1, 1)[0].tolist() == [2]      # blank omitted: -inf
    assert fp.token_set(row, 1, 0)[0].tolist() == [2]      # blank omitted: NaN
    assert fp.token_set(row, 1, 2)[0].tolist() == [2]      # blank inside the top K: once


def test_a_row_without_anything_kills_the_utterance():
    em = fp.continuous_case(4, 1, 5, 4)[0].copy()
    assert len(fp.beam_search(em, 0, 8, 4)) == 8
    em[2] = NEG
    assert fp.beam_search(em, 0, 8, 4) == []
    em[2] = np.nan
    assert fp.beam_search(em, 0, 8, 4) == []
    tokens, lengths, scores = fp.decode_batch(em[None], None, 0, 8, 4, 3)
    assert (tokens == -1).all() and (lengths == 0).all() and np.isneginf(scores).all()


def test_zero_frames_is_no_hypothesis():
    """as ctc_decode: linearGraph(0, C) is one start node that does not accept"""
    g = OGraph.linear(0, 4)
    assert g.shortest_distance(tropical=False) in (None, NEG) or not g.shortest_path()[1]
    em = fp.continuous_case(5, 1, 5, 4)[0]
    assert fp.beam_search(em, 0, 8, 4, frames=0) == []


def test_frames_equal_slicing():
    em = fp.continuous_case(6, 3, 12, 5)
    for form in fp.FORMS:
        assert fp.beam_search(em[1], 0, 8, 3, form, frames=7) == fp.beam_search(em[1, :7], 0, 8, 3, form)
    tokens, lengths, scores = fp.decode_batch(em, [12, 7, 0], 0, 8, 3, 2)
    part = fp.beam_search(em[1, :7], 0, 8, 3)
    for r in range(2):
        assert tokens[1, r, :lengths[1, r]].tolist() == list(part[r][0]) and (tokens[1, r, lengths[1, r]:] == -1).all()
        assert scores[1, r] == part[r][1]
    assert (lengths[2] == 0).all() and np.isneginf(scores[2]).all() and (tokens[2] == -1).all()


def test_fewer_hypotheses_than_nbest_leave_empty_slots():
    em = fp.continuous_case(7, 1, 1, 2)
    tokens, lengths, scores = fp.decode_batch(em, None, 0, 8, 2, 4)  # one frame, two labels: '' and 'a'
    assert np.isfinite(scores[0, :2]).all() and np.isneginf(scores[0, 2:]).all()
    assert sorted(lengths[0].tolist()) == [0, 0, 0, 1] and (tokens[0, 2:] == -1).all()


def test_entry_points_exist(gtn):
    from gtn_amd import torch_loss
    assert callable(torch_loss.ctc_beam_decode)
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    assert hasattr(lib, "gtn_ctc_beam_decode_n")
    eng = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_amd.so"))
    assert hasattr(eng, "gtnx_batch_ctc_beam_decode") and hasattr(eng, "gtnx_batch_ctc_beam_stats")
    assert hasattr(eng, "gtnx_batch_linear_shape")
    assert callable(gtn.Batch.ctc_beam_decode)
    calls, utterances = gtn.debug_ctc_beam_stats()
    assert calls >= 0 and utterances >= 0
    for header, name in (("include/gtn_amd.h", "gtnx_batch_ctc_beam_decode"), ("include/gtn/batch.h", "ctcBeamDecode"),
                         ("gtn_amd/criteria/ctc_criterion.h", "ctcBeamDecodeBatch")):
        with open(os.path.join(ROOT, header)) as f:
            assert name in f.read(), header


def test_argument_errors_come_before_the_device(gtn):
    """what the arguments alone decide is refused as an invalid argument, with or without a device (a batch that is not
    a native linear one, a frame count outside 0 .. M or above the batch's rows, row_stride < M and blank >= C are
    reached on the device only: test_ctc_beam_gpu.py; their torch counterparts are here)"""
    import torch
    import gtn_amd
    from gtn_amd import torch_loss
    batch = gtn.Batch([gtn.linear_graph(2, 8)])
    with pytest.raises(ValueError, match="row_stride"):
        batch.ctc_beam_decode(64, 64, 64)
    with pytest.raises(ValueError, match="one frame count per element"):
        batch.ctc_beam_decode(64, 64, 64, frames=[1, 1], row_stride=2)
    for out in ((0, 64, 64), (64, 0, 64), (64, 64, 0), (None, 64, 64)):
        with pytest.raises(ValueError, match="null output pointer"):
            batch.ctc_beam_decode(*out, row_stride=2)
    with pytest.raises(ValueError, match="negative row stride"):
        batch.ctc_beam_decode(64, 64, 64, row_stride=-1)
    for kw, msg in ((dict(beam_size=0), "beam_size outside"), (dict(beam_size=65), "beam_size outside"),
                    (dict(cutoff_top_n=0), "cutoff_top_n outside"), (dict(cutoff_top_n=33), "cutoff_top_n outside"),
                    (dict(nbest=0), "nbest below 1"), (dict(nbest=17), "nbest above beam_size"),
                    (dict(beam_size=2, nbest=3), "nbest above beam_size"), (dict(blank=-1), "negative blank")):
        with pytest.raises(ValueError, match=msg):
            batch.ctc_beam_decode(64, 64, 64, row_stride=2, **kw)
    # tensors of the wrong kind are refused by the Python layer, not filled with reinterpreted bits
    tok, ln, sc = torch.zeros(1, 1, 2, dtype=torch.int32), torch.zeros(1, 1, dtype=torch.int32), torch.zeros(1, 1)
    for out, msg in (((tok.float(), ln, sc), "tokens_out must be an int32"), ((tok, ln.float(), sc), "lengths_out must be"),
                     ((tok, ln, sc.int()), "scores_out must be"), ((tok, ln.long(), sc), "lengths_out must be"),
                     ((tok[0], ln, sc), "tokens_out must be an int32"),
                     ((torch.zeros(1, 2, 2, dtype=torch.int32), ln, sc), "tokens_out must be an int32")):
        with pytest.raises(ValueError, match=msg):
            batch.ctc_beam_decode(*out)
    rows, labels = ctypes.c_int(0), ctypes.c_int(0)
    assert gtn_amd._lib.gtnx_batch_linear_shape(batch._h, ctypes.byref(rows), ctypes.byref(labels)) == 0
    assert (rows.value, labels.value) == (-1, -1)  # (a batch of graphs has no slabs)
    # the C ABI itself: 1 is GTNX_INVALID_ARGUMENT
    lib = gtn_amd._lib
    p = ctypes.c_void_p
    call = lib.gtnx_batch_ctc_beam_decode
    assert call(batch._h, None, 0, 16, 16, 1, None, 2, p(64), p(64)) == 1
    assert call(batch._h, None, 0, 16, 16, 1, p(64), 2, None, p(64)) == 1
    assert call(batch._h, None, 0, 16, 16, 1, p(64), 2, p(64), None) == 1
    assert call(None, None, 0, 16, 16, 1, p(64), 2, p(64), p(64)) == 1
    assert call(batch._h, None, 0, 16, 16, 1, p(64), -1, p(64), p(64)) == 1
    assert call(batch._h, None, 0, 65, 16, 1, p(64), 2, p(64), p(64)) == 1
    assert call(batch._h, None, 0, 16, 33, 1, p(64), 2, p(64), p(64)) == 1
    assert call(batch._h, None, 0, 16, 16, 17, p(64), 2, p(64), p(64)) == 1
    assert call(batch._h, None, 0, 16, 16, 0, p(64), 2, p(64), p(64)) == 1
    assert call(batch._h, None, -1, 16, 16, 1, p(64), 2, p(64), p(64)) == 1
    em = torch.zeros(2, 3, 8)
    for kw, msg in ((dict(beam_size=0), "beam_size outside 1 .. 64"), (dict(beam_size=65), "beam_size outside 1 .. 64"),
                    (dict(cutoff_top_n=0), "cutoff_top_n outside 1 .. 32"),
                    (dict(cutoff_top_n=33), "cutoff_top_n outside 1 .. 32"), (dict(nbest=0), "nbest outside"),
                    (dict(nbest=17), "nbest outside"), (dict(beam_size=4, nbest=5), "nbest outside"),
                    (dict(blank=8), "blank must be one of"), (dict(blank=-1), "blank must be one of"),
                    (dict(input_lengths=[4, 1]), "input length outside 0 .. 3"),
                    (dict(input_lengths=[-1, 1]), "input length outside 0 .. 3"),
                    (dict(input_lengths=[1]), "input lengths for a batch of 2")):
        with pytest.raises(ValueError, match=msg):
            torch_loss.ctc_beam_decode(em, **kw)
    with pytest.raises(ValueError, match="float32 tensor"):
        torch_loss.ctc_beam_decode(em.double())
    with pytest.raises(ValueError, match="float32 tensor"):
        torch_loss.ctc_beam_decode(em[0])
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        torch_loss.ctc_beam_decode(em)


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU behaviour")
def test_ctc_beam_decode_fails_loudly_without_gpu(gtn):
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    lib.gtn_ctc_beam_decode_n.argtypes = ([ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] + [ctypes.c_int] * 3
                                          + [ctypes.c_void_p] * 3)
    lib.gtn_ctc_beam_decode_n.restype = ctypes.c_int
    lib.gtn_criteria_last_error.restype = ctypes.c_char_p
    rc = lib.gtn_ctc_beam_decode_n(None, 1, 2, 8, 0, None, 16, 16, 1, None, None, None)
    assert rc == -1 and "no HIP device" in lib.gtn_criteria_last_error().decode()
    with pytest.raises(RuntimeError, match="no HIP device"):
        gtn.Batch([gtn.linear_graph(2, 8)]).ctc_beam_decode(64, 64, 64, row_stride=2)


if __name__ == "__main__":
    print("W2_CASE =", _find_w2_case())
