"""CTC best-path decode, the parts that need no GPU: the numpy yardstick of tests/ctc_decode_fp.py (which
test_ctc_decode_gpu.py judges the kernels by) is pinned to the oracle's shortestPath on linearGraph(T, C) -- labels with
`==` everywhere; scores with `==` on the integer-valued cases (exact ties and -inf entries among them) AND on every
continuous seed below: the oracle adds the row maxima in frame order from 0, as the yardstick does, and no seed has
shown another association, so nothing is tolerated.  A case with an all--inf row is "no path" on both sides.  The
collapse rules; the entry points exist, refuse bad arguments before they ask for a device, and fail loudly without
one."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT, has_gpu
from ctc_decode_fp import (collapse, continuous_case, ctc_decode_ref, decode_batch, first_max, first_max_rows,
                           holes_case, planted_case, tie_case)
from oracle_lib import OGraph


def oracle_path(em):
    """(labels, score) of the reference's viterbiPath on linearGraph(T, C), or None without a path"""
    T, C = em.shape
    g = OGraph.linear(T, C, em)
    path, has = g.shortest_path()
    if not has:
        return None
    d = g.to_dict()
    return [d["il"][a] for a in path], g.shortest_distance(tropical=True)


TIE_CASES = [(s, T, C, kind) for s, (T, C) in enumerate([(1, 1), (1, 6), (2, 2), (5, 3), (11, 6), (7, 5), (13, 4)])
             for kind in ("zero", "01", "int")]


@pytest.mark.parametrize("seed,T,C,kind", TIE_CASES)
def test_yardstick_breaks_exact_ties_like_the_oracle(seed, T, C, kind):
    em = tie_case(seed, 1, T, C, kind)[0]
    labels, score, _, _ = ctc_decode_ref(em)
    want, want_score = oracle_path(em)
    assert labels.tolist() == want
    assert score == want_score


@pytest.mark.parametrize("seed", range(40))
def test_yardstick_with_minus_infinity_entries(seed):
    """integer-valued rows with -inf holes, T <= 11, C <= 6: labels and score == the oracle's where a path exists; an
    all--inf row gives no path on both sides (seeds 0 .. 39 hold both kinds: checked below)"""
    rng = np.random.default_rng(1000 + seed)
    T, C = int(rng.integers(1, 12)), int(rng.integers(1, 7))
    em = holes_case(seed, 1, T, C, p=0.45)[0]
    labels, score, tokens, starts = ctc_decode_ref(em, blank=0)
    got = oracle_path(em)
    dead = bool(np.isneginf(em).all(axis=1).any())
    if dead:
        assert got is None
        assert (labels == -1).all() and score == -np.inf and tokens == [] and starts == []
    else:
        assert got is not None and labels.tolist() == got[0] and score == got[1]


def test_the_hole_cases_hold_both_kinds():
    dead = 0
    for seed in range(40):
        rng = np.random.default_rng(1000 + seed)
        T, C = int(rng.integers(1, 12)), int(rng.integers(1, 7))
        dead += bool(np.isneginf(holes_case(seed, 1, T, C, p=0.45)[0]).all(axis=1).any())
    assert 5 <= dead <= 35


@pytest.mark.parametrize("seed,T,C", [(1, 1, 2), (2, 9, 29), (3, 40, 7), (4, 65, 3), (5, 129, 64), (6, 200, 5),
                                      (7, 33, 300), (8, 64, 65)])
def test_yardstick_agrees_with_the_oracle_on_continuous_scores(seed, T, C):
    """labels == and scores == (not within a bound): both sides add the maxima in frame order in float32"""
    for em in (continuous_case(seed, 1, T, C)[0], planted_case(seed, 1, T, C, 0)[0]):
        labels, score, _, _ = ctc_decode_ref(em)
        want, want_score = oracle_path(em)
        assert labels.tolist() == want
        assert score == np.float32(want_score), (score, want_score)


def test_zero_frames_is_no_path():
    """linearGraph(0, C) is one start node that does not accept (reference creations.cpp:22): no path, score -inf"""
    g = OGraph.linear(0, 4)
    path, has = g.shortest_path()
    assert not has and path == [] and g.shortest_distance(tropical=True) == -np.inf
    labels, score, tokens, starts = ctc_decode_ref(np.zeros((3, 4), np.float32), frames=0, blank=0)
    assert (labels == -1).all() and score == -np.inf and tokens == [] and starts == []


def test_vectorised_rows_are_the_loop():
    em = holes_case(5, 1, 50, 7, p=0.5)[0]
    em[3, 2] = np.nan
    em[4] = np.nan
    em[5, 1] = np.inf
    em[6] = [-np.inf, np.nan, -np.inf, 2.0, 2.0, np.nan, -np.inf]
    lab, m = first_max_rows(em)
    for t in range(em.shape[0]):
        l1, m1 = first_max(em[t])
        assert lab[t] == l1 and m[t] == m1
    assert lab[4] == -1 and lab[6] == 3


def test_collapse_rules():
    a, b, _ = 1, 2, 0
    assert collapse([a, a, _, a, b, b], blank=_) == ([a, a, b], [0, 3, 4])
    assert collapse([_, _, _, _], blank=_) == ([], [])
    assert collapse([a, a, _, a, b, b], blank=-1) == ([a, _, a, b], [0, 2, 3, 4])
    assert collapse([], blank=0) == ([], [])
    assert collapse([2, 2, 2], blank=2) == ([], [])
    assert collapse([0, 2, 2, 0], blank=2) == ([0, 0], [0, 3])


def test_frame_counts_and_dense_rows():
    em = planted_case(9, 3, 12, 5, 0)
    full = ctc_decode_ref(em[1, :7], blank=0)
    part = ctc_decode_ref(em[1], frames=7, blank=0)
    assert part[0][:7].tolist() == full[0].tolist() and (part[0][7:] == -1).all()
    assert part[1] == full[1] and part[2:] == full[2:]
    labels, scores, tokens, starts, lengths = decode_batch(em, [12, 7, 0], 0)
    assert labels[1].tolist() == part[0].tolist() and scores[1] == part[1] and lengths[1] == len(part[2])
    assert tokens[1, :lengths[1]].tolist() == part[2] and (tokens[1, lengths[1]:] == -1).all()
    assert starts[1, :lengths[1]].tolist() == part[3] and (starts[1, lengths[1]:] == -1).all()
    assert lengths[2] == 0 and scores[2] == -np.inf and (labels[2] == -1).all()
    assert 0 < lengths[0] < 12


def test_entry_points_exist(gtn):
    from gtn_amd import torch_loss
    assert callable(torch_loss.ctc_decode)
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    assert hasattr(lib, "gtn_ctc_decode_n")
    eng = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_amd.so"))
    assert hasattr(eng, "gtnx_batch_linear_decode") and hasattr(eng, "gtnx_batch_linear_decode_stats")
    assert callable(gtn.Batch.linear_decode)
    fast, fallback = gtn.debug_linear_decode_stats()
    assert fast >= 0 and fallback >= 0


def test_argument_errors_come_before_the_device(gtn):
    """what the arguments alone decide is refused as an invalid argument, with or without a device (the checks that
    need a native linear batch -- a frame count outside 0 .. M or above the batch's rows, row_stride < M, blank >= C --
    are reached on the device only: test_ctc_decode_gpu.py; their torch counterparts are here)"""
    import torch
    import gtn_amd
    from gtn_amd import torch_loss
    batch = gtn.Batch([gtn.linear_graph(2, 8)])
    with pytest.raises(ValueError, match="row_stride"):
        batch.linear_decode(0)
    with pytest.raises(ValueError, match="need collapsed_out"):
        batch.linear_decode(0, lengths_out=0, row_stride=2)
    with pytest.raises(ValueError, match="need collapsed_out"):
        batch.linear_decode(0, starts_out=0, row_stride=2)
    with pytest.raises(ValueError, match="one frame count per element"):
        batch.linear_decode(0, frames=[1, 1], row_stride=2)
    with pytest.raises(ValueError, match="null labels pointer"):
        batch.linear_decode(0, row_stride=2)
    with pytest.raises(ValueError, match="negative row stride"):
        batch.linear_decode(64, row_stride=-1)
    with pytest.raises(ValueError, match="frame counts need a native linear batch"):
        batch.linear_decode(64, frames=[1], row_stride=2)
    # the C ABI itself: lengths / starts without collapsed, a null batch
    lib = gtn_amd._lib
    p = ctypes.c_void_p
    assert lib.gtnx_batch_linear_decode(batch._h, None, 0, p(64), 2, None, None, None, p(64)) == 1
    assert lib.gtnx_batch_linear_decode(batch._h, None, 0, p(64), 2, None, None, p(64), None) == 1
    assert lib.gtnx_batch_linear_decode(None, None, 0, p(64), 2, None, None, None, None) == 1
    em = torch.zeros(2, 3, 8)
    with pytest.raises(ValueError, match="blank must be below"):
        torch_loss.ctc_decode(em, blank=8)
    with pytest.raises(ValueError, match="input length outside 0 .. 3"):
        torch_loss.ctc_decode(em, input_lengths=[4, 1])
    with pytest.raises(ValueError, match="input length outside 0 .. 3"):
        torch_loss.ctc_decode(em, input_lengths=[-1, 1])
    with pytest.raises(ValueError, match="input lengths for a batch of 2"):
        torch_loss.ctc_decode(em, input_lengths=[1])
    with pytest.raises(ValueError, match="float32 tensor"):
        torch_loss.ctc_decode(em.double())
    with pytest.raises(ValueError, match="float32 tensor"):
        torch_loss.ctc_decode(em[0])
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        torch_loss.ctc_decode(em)


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU behaviour")
def test_ctc_decode_fails_loudly_without_gpu(gtn):
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    lib.gtn_ctc_decode_n.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 6
    lib.gtn_ctc_decode_n.restype = ctypes.c_int
    lib.gtn_criteria_last_error.restype = ctypes.c_char_p
    rc = lib.gtn_ctc_decode_n(None, 1, 2, 8, 0, None, None, None, None, None, None)
    assert rc == -1 and "no HIP device" in lib.gtn_criteria_last_error().decode()
    with pytest.raises(RuntimeError, match="no HIP device"):
        gtn.Batch([gtn.linear_graph(2, 8)]).linear_decode(64, row_stride=2)
