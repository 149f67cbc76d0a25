"""ASG prefix beam search, the parts that need no GPU.  The float64 yardstick of tests/asg_beam_fp.py (which
test_asg_beam_gpu.py judges the kernels by) is pinned three times on cases where nothing is pruned: to a brute-force
enumeration of all C^T labellings (the same hypothesis set, every score to 1e-12), to the oracle's
forwardScore(emissions o transitions) through the log-sum over all hypotheses (1e-4 max(1, |score|), the bound the CPU
tests give that float32 oracle), and to tests/asg_score_fp.py's score of the same tokens.  Every case the GPU file runs
vets; the recreated-prefix cases need exact identity; the rules of the contract one by one; the entry points exist in
every layer and refuse bad arguments before they ask for a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import asg_beam_fp as fp
from asg_loss_fp import fal_fp64
from conftest import ROOT, has_gpu
from oracle_lib import OGraph

NEG = -np.inf
WHO = "[gtnx_batch_asg_beam_decode] "


def _ids(c):
    return "-".join(str(v) for v in c[:8])


SMALL = [(1, 2), (2, 3), (3, 3), (4, 3), (5, 2), (3, 4), (4, 4), (5, 3)]


@pytest.mark.parametrize("T,C", SMALL)
@pytest.mark.parametrize("holes", [0.0, 0.25])
def test_unpruned_search_is_the_enumeration(T, C, holes):
    """T <= 5, C <= 4: the same hypothesis set as the enumeration over all labellings, every score within 1e-12, best
    first; with -inf table entries as well"""
    em = fp.continuous_case(10 * T + C, 1, T, C)[0]
    table = fp.table_case(10 * T + C, C, holes)
    want = fp.brute_force(em, table)
    got = fp.beam_search(em, table, 10 ** 6, C, "f64")
    assert sorted(y for y, _ in got) == sorted(want)
    assert all(a != b for y in want for a, b in zip(y, y[1:]))
    scores = [s for _, s in got]
    assert scores == sorted(scores, reverse=True)
    if got:
        assert got[0][0] == max(want, key=want.get)
    for y, s in got:
        assert abs(s - want[y]) <= 1e-12, (y, s, want[y])


def _transitions_graph(table, C):
    d = {"start": [1] + [0] * C, "accept": [0] + [1] * C, "src": [], "dst": [], "il": [], "ol": [], "w": [], "sort": "i"}
    for i in range(C):
        d["src"].append(0), d["dst"].append(i + 1), d["il"].append(i), d["ol"].append(i), d["w"].append(float(table[i]))
    for i in range(C):
        for j in range(C):
            d["src"].append(j + 1), d["dst"].append(i + 1), d["il"].append(i), d["ol"].append(i)
            d["w"].append(float(table[C + i * C + j]))
    return OGraph.from_dict(d)


@pytest.mark.parametrize("T,C", SMALL + [(7, 3), (6, 4)])
def test_the_hypotheses_partition_the_full_connect_score(T, C):
    """unpruned, the log-sum over all hypotheses is the oracle's forwardScore(emissions o transitions)"""
    em = fp.continuous_case(20 * T + C, 1, T, C)[0]
    table = fp.table_case(20 * T + C, C)
    got = fp.beam_search(em, table, 10 ** 6, C, "f64")
    total = np.logaddexp.reduce([float(s) for _, s in got])
    want = OGraph.linear(T, C, em.reshape(-1)).compose(_transitions_graph(table, C)).shortest_distance()
    assert want is not None and abs(total - want) <= 1e-4 * max(1.0, abs(want)), (total, want)


@pytest.mark.parametrize("T,C", SMALL)
def test_a_score_is_asg_score_of_the_tokens(T, C):
    """unpruned, every hypothesis's score is the force-align term of its tokens (asg_score's float64 yardstick)"""
    em = fp.continuous_case(30 * T + C, 1, T, C)[0]
    table = fp.table_case(30 * T + C, C, 0.2 if T == 4 else 0.0)
    for y, s in fp.beam_search(em, table, 10 ** 6, C, "f64"):
        ref = fal_fp64(em, table[C:].reshape(C, C), table[:C], y)[0]
        assert abs(s - ref) <= 1e-9, (y, s, ref)


def test_pruning_is_real():
    """a beam of 2 and a cutoff of 1 both change the result of a seeded case"""
    em, table = fp.continuous_case(3, 1, 6, 4)[0], fp.table_case(3, 4)
    full = fp.beam_search(em, table, 10 ** 6, 4)
    assert len(fp.beam_search(em, table, 2, 4)) == 2 < len(full)
    one = fp.beam_search(em, table, 64, 1)
    assert len(one) == 1 and one[0][1] < dict(full)[one[0][0]]  # (the best labelling alone, of all that spell it)


@pytest.mark.parametrize("case", fp.ALL_GPU_CASES, ids=_ids)
def test_every_gpu_case_vets(case):
    kind, seed, B, T, C, W, K, nbest, frames, holes = case
    assert nbest <= 4 or T <= 3
    assert nbest <= W
    _, _, res, _ = fp.results_of(case)
    ok, err, gap = fp.vet(res, nbest)
    print(f"[asg_beam] {case}: err {err:.3g} smallest gap {gap:.3g}")
    assert ok, (err, gap)


@pytest.mark.parametrize("case", [fp.CONSTRAINED_CASE, fp.NAN_TABLE_CASE], ids=["minus-inf", "nan"])
def test_the_table_holes_bite(case):
    """a start entry and a transition are among the holes, and without them the search returns both kinds"""
    C = case[4]
    _, table, res, _ = fp.results_of(case)
    assert not np.isfinite(table[:C]).all() and not np.isfinite(table[C:]).all()
    assert np.isnan(table).any() == isinstance(case[9], tuple)
    assert fp.constraints_bite(case)
    for h in res["f64"]:
        assert not any(fp.forbidden_first(table, y) or fp.forbidden_bigram(table, C, y) for y, _ in h)
        assert all(np.isfinite(s) for _, s in h)


def test_the_shape_cases_cover_the_issue():
    col = lambda i: {c[i] for c in fp.SHAPE_CASES}
    assert col(4) >= {1, 2, 3, 5, 29, 33, 64, 65, 256, 257, 300, 1000}
    assert col(3) >= {1, 2, 3, 63, 64, 65, 128, 129} and col(2) >= {1, 2, 65}
    assert col(5) >= {1, 2, 63, 64} and col(6) >= {1, 32} and col(7) >= {1, 2, 4}
    assert any(c[4] <= c[6] for c in fp.SHAPE_CASES)  # C <= K
    for c in fp.UNPRUNED_CASES:
        assert c[3] <= 3 and c[4] <= 4 and c[5] == 64 and c[6] == c[4]


@pytest.mark.parametrize("case", fp.RECREATED_CASES, ids=_ids)
def test_recreated_prefix_cases_need_exact_identity(case):
    """a prefix leaves the list while its child stays and is created again: knowing a prefix by the number its node got
    gets the compared hypotheses of these cases wrong (the child is no longer merged with, its mass is split).  A search
    of 400 seeds per shape found a case for each of the five shapes of ctc_beam_fp.RECREATED_CASES."""
    _, _, res, again = fp.results_of(case)
    assert again > 0
    for h in res["f64"]:
        assert len(set(y for y, _ in h)) == len(h)
    assert fp.fresh_differs(case)


def test_there_are_at_least_three_recreated_cases():
    assert len(fp.RECREATED_CASES) >= 3


def test_top_k_ties_go_to_the_smaller_label_and_there_is_no_blank():
    row = np.array([0, 2, 2, 1, 2, 1], np.float32)
    assert fp.token_set(row, 2)[0].tolist() == [1, 2]
    assert fp.token_set(row, 4)[0].tolist() == [1, 2, 4, 3]
    assert fp.token_set(row, 32)[0].tolist() == [1, 2, 4, 3, 5, 0]
    # one frame, a table of zeros: the extensions of the empty prefix by (score, label); no empty hypothesis
    got = fp.beam_search(row[None], np.zeros(6 + 36, np.float32), 8, 4, "f64")
    assert got == [((1,), 2.0), ((2,), 2.0), ((4,), 2.0), ((3,), 1.0)]


def test_integer_cases_are_exact_at_one_frame():
    """T = 1 with an integer table: every score is exact, so the three forms are one"""
    em = fp.integer_case(3, 65, 1, 29)
    table = np.random.default_rng(7).integers(-2, 2, 29 + 29 * 29).astype(np.float32)
    for b in range(65):
        got = [fp.beam_search(em[b], table, 8, 3, f) for f in fp.FORMS]
        assert got[0] == got[1] == got[2]


def test_nan_and_minus_infinity_are_never_chosen():
    row = np.array([np.nan, NEG, 1.0, np.nan, -2.0, NEG], np.float32)
    assert fp.token_set(row, 4)[0].tolist() == [2, 4]
    assert fp.token_set(row, 1)[0].tolist() == [2]


def test_the_token_set_restricts_the_stays():
    """label 0 wins frame 0 and is outside S_1 with K = 1: its prefix cannot stay, only grow by label 1"""
    em = np.array([[0.0, -1.0], [-5.0, 0.0]], np.float32)
    table = np.zeros(2 + 4, np.float32)
    assert [y for y, _ in fp.beam_search(em, table, 8, 1)] == [(0, 1)]
    assert sorted(y for y, _ in fp.beam_search(em, table, 8, 2)) == [(0,), (0, 1), (1,), (1, 0)]


def test_table_entries_that_are_not_finite_drop_their_candidates():
    em = fp.continuous_case(8, 1, 4, 3)[0]
    table = fp.table_case(8, 3)
    free = fp.beam_search(em, table, 64, 3)
    no_first = table.copy()
    no_first[1] = NEG  # label 1 may not come first
    no_bigram = table.copy()
    no_bigram[3 + 2 * 3 + 0] = NEG  # label 0 may not be followed by label 2
    no_self = table.copy()
    no_self[3 + 1 * 3 + 1] = np.nan  # label 1 may not stay (NaN drops like -inf)
    assert any(y[0] == 1 for y, _ in free) and not any(y[0] == 1 for y, _ in fp.beam_search(em, no_first, 64, 3))
    has = lambda h: any((a, b) == (0, 2) for y, _ in h for a, b in zip(y, y[1:]))
    assert has(free) and not has(fp.beam_search(em, no_bigram, 64, 3))
    got = fp.beam_search(em, no_self, 64, 3)
    assert all(np.isfinite(s) for _, s in got)
    want = fp.brute_force(em, np.where(np.isnan(no_self), NEG, no_self))
    assert sorted(y for y, _ in got) == sorted(want)
    for pinf in (np.inf,):  # +inf drops as well: no candidate ever scores +inf
        t = table.copy()
        t[0] = pinf
        assert not any(y[0] == 0 for y, _ in fp.beam_search(em, t, 64, 3))


def test_a_row_without_anything_kills_the_utterance():
    em = fp.continuous_case(4, 1, 5, 4)[0].copy()
    table = fp.table_case(4, 4)
    assert len(fp.beam_search(em, table, 8, 4)) == 8
    em[2] = NEG
    assert fp.beam_search(em, table, 8, 4) == []
    em[2] = np.nan
    assert fp.beam_search(em, table, 8, 4) == []
    tokens, lengths, scores = fp.decode_batch(em[None], table, None, 8, 4, 3)
    assert (tokens == -1).all() and (lengths == 0).all() and np.isneginf(scores).all()


def test_frames_equal_slicing_and_zero_frames_is_no_hypothesis():
    em = fp.continuous_case(6, 3, 12, 5)
    table = fp.table_case(6, 5)
    for form in fp.FORMS:
        assert fp.beam_search(em[1], table, 8, 3, form, frames=7) == fp.beam_search(em[1, :7], table, 8, 3, form)
    assert fp.beam_search(em[0], table, 8, 3, frames=0) == []
    tokens, lengths, scores = fp.decode_batch(em, table, [12, 7, 0], 8, 3, 2)
    part = fp.beam_search(em[1, :7], table, 8, 3)
    for r in range(2):
        assert tokens[1, r, :lengths[1, r]].tolist() == list(part[r][0]) and (tokens[1, r, lengths[1, r]:] == -1).all()
        assert scores[1, r] == part[r][1]
    assert (lengths[2] == 0).all() and np.isneginf(scores[2]).all() and (tokens[2] == -1).all()


def test_fewer_hypotheses_than_nbest_leave_empty_slots():
    em = fp.continuous_case(7, 1, 1, 2)
    tokens, lengths, scores = fp.decode_batch(em, fp.table_case(7, 2), None, 8, 2, 4)  # one frame, two labels
    assert np.isfinite(scores[0, :2]).all() and np.isneginf(scores[0, 2:]).all()
    assert lengths[0].tolist() == [1, 1, 0, 0] and (tokens[0, 2:] == -1).all()


# ---- the entry points ----
def test_entry_points_exist(gtn):
    from gtn_amd import torch_loss
    assert callable(torch_loss.asg_beam_decode)
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    assert hasattr(lib, "gtn_asg_beam_decode_n")
    eng = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_amd.so"))
    assert hasattr(eng, "gtnx_batch_asg_beam_decode") and hasattr(eng, "gtnx_batch_asg_beam_stats")
    assert callable(gtn.Batch.asg_beam_decode)
    calls, utterances = gtn.debug_asg_beam_stats()
    assert calls >= 0 and utterances >= 0
    for header, name in (("include/gtn_amd.h", "gtnx_batch_asg_beam_decode"), ("include/gtn/batch.h", "asgBeamDecode"),
                         ("gtn_amd/criteria/asg_criterion.h", "asgBeamDecodeBatch"),
                         ("gtn_amd/csrc/Makefile", "asg_beam.hip"), ("gtn_amd/csrc/kernels.h", "launch_asg_beam")):
        with open(os.path.join(ROOT, header)) as f:
            assert name in f.read(), header


def test_the_kernel_file_shares_the_rows_and_has_no_assembly():
    """read out of the two sources: both rows kernels are the shared body, the ASG set has no slot for a blank"""
    src = lambda n: open(os.path.join(ROOT, "gtn_amd", "csrc", n)).read()
    asg, ctc = src("asg_beam.hip"), src("ctc_beam.hip")
    assert "asm" not in re.sub(r"//.*", "", asg)
    assert re.search(r"constexpr int kMaxSet = 32;", asg) and re.search(r"constexpr int kMaxSet = 33;", ctc)
    assert "beam_rows_body<LPR, false>" in asg and "beam_rows_body<LPR, true>" in ctc
    assert "atomicAdd" not in asg


def test_argument_errors_come_before_the_device(gtn):
    """what the arguments alone decide is GTNX_INVALID_ARGUMENT (1) with its exact text, with or without a device; a
    call with n == 0 is OK and counts nothing (the refusals that need the device: test_asg_beam_gpu.py)"""
    import gtn_amd
    lib = gtn_amd._lib
    lib.gtnx_last_error.restype = ctypes.c_char_p
    batch = gtn.Batch([gtn.linear_graph(2, 8)])
    p = ctypes.c_void_p
    call = lib.gtnx_batch_asg_beam_decode
    #        ems     frames table  W   K   n  tokens stride lengths scores
    good = [batch._h, None, p(64), 16, 16, 1, p(64), 2, p(64), p(64)]
    before = gtn.debug_asg_beam_stats()
    out = "null output pointer (tokens, lengths and scores are all written)"
    for i, v, text in ((0, None, "null batch"), (2, None, "null table pointer"), (6, None, out), (8, None, out),
                       (9, None, out), (7, -1, "negative row stride"), (3, 0, "beam_size outside 1 .. 64"),
                       (3, 65, "beam_size outside 1 .. 64"), (4, 0, "cutoff_top_n outside 1 .. 32"),
                       (4, 33, "cutoff_top_n outside 1 .. 32"), (5, 0, "nbest outside 1 .. beam_size"),
                       (5, 17, "nbest outside 1 .. beam_size")):
        a = list(good)
        a[i] = v
        assert call(*a) == 1, (i, v)
        assert lib.gtnx_last_error().decode() == WHO + text, (i, v)
    assert call(batch._h, None, p(64), 2, 16, 3, p(64), 2, p(64), p(64)) == 1
    empty = gtn.Batch([])
    assert len(empty) == 0
    assert call(empty._h, None, p(64), 16, 16, 1, p(64), 0, p(64), p(64)) == 0
    assert call(empty._h, None, p(64), 16, 16, 0, p(64), 0, p(64), p(64)) == 1  # (the arguments are checked all the same)
    assert gtn.debug_asg_beam_stats() == before  # (nothing launched)
    # the Python layer
    with pytest.raises(ValueError, match="row_stride"):
        batch.asg_beam_decode(64, 64, 64, None, 64)
    with pytest.raises(ValueError, match="one frame count per element"):
        batch.asg_beam_decode(64, 64, 64, [1, 1], 64, row_stride=2)
    with pytest.raises(ValueError, match="null table pointer"):
        batch.asg_beam_decode(64, 64, 64, None, None, row_stride=2)
    with pytest.raises(ValueError, match="nbest outside 1 .. beam_size"):
        batch.asg_beam_decode(64, 64, 64, None, 64, 4, 4, 5, row_stride=2)


def test_torch_argument_checks():
    import torch
    from gtn_amd import torch_loss
    em = torch.zeros(2, 3, 8)
    tr = torch.zeros(8, 8)
    for args, kw, msg in (((em.double(), tr), {}, "float32 tensor"), ((em[0], tr), {}, "float32 tensor"),
                          ((em, tr[:7]), {}, r"transitions must be \[8, 8\]"),
                          ((em, tr), dict(start=torch.zeros(7)), r"start must be \[8\]"),
                          ((em, tr), dict(beam_size=0), "beam_size outside 1 .. 64"),
                          ((em, tr), dict(beam_size=65), "beam_size outside 1 .. 64"),
                          ((em, tr), dict(cutoff_top_n=0), "cutoff_top_n outside 1 .. 32"),
                          ((em, tr), dict(cutoff_top_n=33), "cutoff_top_n outside 1 .. 32"),
                          ((em, tr), dict(nbest=0), "nbest outside"), ((em, tr), dict(nbest=17), "nbest outside"),
                          ((em, tr), dict(input_lengths=[4, 1]), "input length outside 0 .. 3"),
                          ((em, tr), dict(input_lengths=[1]), "input lengths for a batch of 2")):
        with pytest.raises(ValueError, match=msg):
            torch_loss.asg_beam_decode(*args, **kw)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        torch_loss.asg_beam_decode(em, tr)


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU behaviour")
def test_asg_beam_decode_fails_loudly_without_gpu(gtn):
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    fn = lib.gtn_asg_beam_decode_n
    fn.argtypes = ([ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3
                   + [ctypes.c_void_p] * 3)
    fn.restype = ctypes.c_int
    lib.gtn_criteria_last_error.restype = ctypes.c_char_p
    p = ctypes.c_void_p
    rc = fn(None, 1, 2, 8, p(64), None, 16, 16, 1, p(64), p(64), p(64))
    assert rc == -1 and "no HIP device" in lib.gtn_criteria_last_error().decode()
    with pytest.raises(RuntimeError, match="no HIP device"):
        gtn.Batch([gtn.linear_graph(2, 8)]).asg_beam_decode(64, 64, 64, None, 64, row_stride=2)
