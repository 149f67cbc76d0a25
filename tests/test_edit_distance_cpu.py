"""Batched edit distance, the parts that need no GPU.  The yardstick of tests/edit_distance_fp.py (the textbook table and
the contract's walk back, which test_edit_distance_gpu.py judges the kernel by) is pinned to the recorded results of the
unmodified reference's -viterbiScore(compose(hyp, compose(edits, ref))) (tests/golden/edit_distance.json) and, where
oracle/_ref/libgtn_ref.so exists, to that reference live; the plain-Python transcription of the kernel's block
recurrence equals the table on every cell and the yardstick's dist and ops on every case the GPU file launches; the
invariants of the counts; the entry points exist in every layer, refuse bad arguments before they ask for a device, and
fail loudly without one.  Every comparison is ==."""
import ctypes
import json
import os

import pytest

import edit_distance_fp as fp
from conftest import ROOT, has_gpu

with open(os.path.join(ROOT, "tests", "golden", "edit_distance.json")) as _f:
    GOLDEN = json.load(_f)["pairs"]


def test_the_fixture_covers_the_specs():
    assert [(p["seed"], p["len_ref"], p["len_hyp"], p["alphabet"]) for p in GOLDEN] == list(fp.GOLDEN_SPECS)
    shapes = {(p["len_ref"], p["len_hyp"]) for p in GOLDEN}
    assert {(0, 0), (64, 70), (65, 63)} <= shapes
    assert any(m == 0 and n > 0 for m, n in shapes) and any(m > 0 and n == 0 for m, n in shapes)
    assert all(p["alphabet"] <= 5 and p["len_ref"] <= 70 and p["len_hyp"] <= 70 for p in GOLDEN)


@pytest.mark.parametrize("p", GOLDEN, ids=lambda p: f"s{p['seed']}-{p['len_ref']}x{p['len_hyp']}-a{p['alphabet']}")
def test_yardstick_equals_the_recorded_reference(p):
    ref, hyp = fp.seeded_pair(p["seed"], p["len_ref"], p["len_hyp"], p["alphabet"])
    assert len(ref) == p["len_ref"] and len(hyp) == p["len_hyp"]
    assert fp.distance_ops(ref, hyp)[0] == p["dist"]
    assert fp.blocks_forward(ref, hyp)[0] == p["dist"]


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libgtn_ref.so")),
                    reason="the reference-built library is not here")
def test_yardstick_equals_the_reference_live():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "refbackend"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import gtn_ref
    import make_edit_distance as gen
    for seed, m, n, alphabet in ((101, 0, 0, 2), (102, 5, 0, 2), (103, 0, 4, 3), (104, 9, 13, 2), (105, 30, 22, 4),
                                 (106, 17, 17, 5), (107, 33, 40, 3)):
        ref, hyp = fp.seeded_pair(seed, m, n, alphabet)
        assert gen.reference_distance(gtn_ref, ref, hyp, alphabet) == fp.distance_ops(ref, hyp)[0], (seed, m, n)


@pytest.mark.parametrize("m,n,alphabet", [(130, 90, 3), (64, 65, 2), (65, 64, 5), (63, 1, 2), (1, 1, 1), (0, 5, 2),
                                          (5, 0, 2), (128, 70, 4), (129, 66, 1000)])
def test_transcription_equals_the_table_on_every_cell(m, n, alphabet):
    ref, hyp = fp.seeded_pair(1000 + 7 * m + n, m, n, alphabet)
    D = fp.table(ref, hyp)
    dist, words = fp.blocks_forward(ref, hyp)
    nb = (m + 63) >> 6
    assert dist == D[m][n]
    for i in range(m + 1):
        for j in range(n + 1):
            assert fp.blocks_cell(words, nb, i, j) == D[i][j], (i, j)


@pytest.mark.parametrize("case", fp.gpu_cases(), ids=repr)
def test_transcription_equals_the_yardstick_on_every_gpu_case(case):
    dist, ops = fp.expected(case)
    for b, k, ref, hyp in case.pairs():
        d, o = fp.blocks_distance_ops(ref, hyp)
        assert d == dist[b, k], (b, k)
        assert tuple(o) == tuple(ops[b, k]), (b, k)


@pytest.mark.parametrize("case", fp.gpu_cases(), ids=repr)
def test_invariants_of_the_counts(case):
    for b, k, ref, hyp in case.pairs():
        dist, (s, d, i), matches = fp.distance_ops(ref, hyp)
        assert s + d + i == dist
        assert matches + s + d == len(ref)
        assert matches + s + i == len(hyp)
        assert abs(len(ref) - len(hyp)) <= dist <= max(len(ref), len(hyp))


def test_known_answers():
    assert fp.distance_ops([], []) == (0, (0, 0, 0), 0)
    assert fp.distance_ops([1, 2, 3], []) == (3, (0, 3, 0), 0)
    assert fp.distance_ops([], [1, 2]) == (2, (0, 0, 2), 0)
    # kitten / sitting: two substitutions and one insertion
    k, s = [ord(c) for c in "kitten"], [ord(c) for c in "sitting"]
    assert fp.distance_ops(k, s) == (3, (2, 0, 1), 4)
    # ab / b: the diagonal of the last cell is the match, a deletion remains
    assert fp.distance_ops([1, 2], [2]) == (1, (0, 1, 0), 1)
    # where diagonal and up both attain D[i][j], the diagonal is taken: aa / a ends on the match
    assert fp.distance_ops([5, 5], [5]) == (1, (0, 1, 0), 1)
    # up before left
    assert fp.distance_ops([1], [2, 3]) == (2, (1, 0, 1), 0)
    for case in fp.gpu_cases():
        if case.name == "disjoint":
            for (b, k, ref, hyp), d in zip(case.pairs(), fp.expected(case)[0].ravel()):
                assert d == max(len(ref), len(hyp))


def test_swapping_the_sides_keeps_dist_and_the_sum_of_deletions_and_insertions():
    for seed in range(40):
        ref, hyp = fp.seeded_pair(seed, (13 * seed) % 90, (29 * seed + 5) % 80, 2 + seed % 3)
        d1, (s1, del1, ins1), _ = fp.distance_ops(ref, hyp)
        d2, (s2, del2, ins2), _ = fp.distance_ops(hyp, ref)
        assert d1 == d2
        # (the two walks may choose different alignments of the same cost: deletions and insertions trade places only
        # in their total, D - I is fixed by the lengths)
        assert del1 - ins1 == len(ref) - len(hyp) == ins2 - del2
        assert (del1 + ins1 + s1) == (del2 + ins2 + s2)


def test_cases_are_what_the_issue_lists():
    cases = {c.name: c for c in fp.gpu_cases()}
    for a in (2, 5, 1000):
        c = cases[f"edges-a{a}"]
        assert tuple(len(r) for r in c.refs) == fp.REF_EDGES
        assert all(tuple(len(h) for h in row) == fp.HYP_EDGES for row in c.hyps)
    assert {c.B for c in cases.values()} >= {1, 5, 70} and {c.N for c in cases.values()} >= {1, 3}
    sl = cases["sliced"]
    assert 16 * sl.L * ((sl.U + 63) // 64) * sl.B * sl.N > sl.cap >= 16 * sl.L * ((sl.U + 63) // 64)
    assert max(len(r) for r in cases["ten-blocks"].refs) > 512
    vals = {t for r in cases["extreme-tokens"].refs for t in r}
    assert {-1, fp.INT_MIN, fp.INT_MAX} <= vals


def test_entry_points_exist(gtn):
    from gtn_amd import torch_loss
    assert callable(torch_loss.edit_distance)
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    assert hasattr(lib, "gtn_edit_distance_n")
    eng = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_amd.so"))
    assert hasattr(eng, "gtnx_batch_edit_distance") and hasattr(eng, "gtnx_batch_edit_distance_stats")
    assert callable(gtn.edit_distance)
    calls, pairs = gtn.debug_edit_distance_stats()
    assert calls >= 0 and pairs >= 0
    for header, name in (("include/gtn_amd.h", "gtnx_batch_edit_distance"), ("include/gtn/batch.h", "editDistance"),
                         ("gtn_amd/criteria/edit_distance.h", "editDistanceBatch"),
                         ("gtn_amd/csrc/kernels.h", "launch_edit_distance")):
        with open(os.path.join(ROOT, header)) as f:
            assert name in f.read(), header


def test_argument_errors_come_before_the_device(gtn):
    """what the arguments alone decide is refused as an invalid argument, with or without a device: without one the
    message is the argument's, never the device's"""
    import torch
    import gtn_amd
    from gtn_amd import torch_loss
    before = gtn.debug_edit_distance_stats()
    ok = dict(B=2, N=3, L=8, U=5, hyp_stride=8, ref_stride=5)

    def call(hyp=64, hl=64, ref=64, rl=64, dist=64, ops=None, **kw):
        gtn.edit_distance(hyp, hl, ref, rl, dist, ops, **{**ok, **kw})

    for kw in (dict(hyp=0), dict(hl=0), dict(ref=0), dict(rl=0), dict(hyp=None), dict(rl=None)):
        with pytest.raises(ValueError, match="null input pointer"):
            call(**kw)
    for kw in (dict(dist=0), dict(dist=None)):
        with pytest.raises(ValueError, match="null dist pointer"):
            call(**kw)
    for kw in (dict(B=-1), dict(N=-1), dict(L=-1, hyp_stride=0), dict(U=-1, ref_stride=0)):
        with pytest.raises(ValueError, match="negative B, N, L or U"):
            call(**kw)
    for kw in (dict(hyp_stride=-1), dict(ref_stride=-8)):
        with pytest.raises(ValueError, match="negative row stride"):
            call(**kw)
    with pytest.raises(ValueError, match="hyp_stride is shorter"):
        call(hyp_stride=7)
    with pytest.raises(ValueError, match="ref_stride is shorter"):
        call(ref_stride=4)
    with pytest.raises(ValueError, match="L above 65536"):
        call(L=65537, hyp_stride=65537)
    with pytest.raises(ValueError, match="U above 4096"):
        call(U=4097, ref_stride=4097)
    with pytest.raises(ValueError, match="does not fit an int"):
        call(B=1 << 20, N=1 << 12)
    # an empty call returns without touching a device -- also on a machine without one
    call(B=0)
    call(N=0)
    call(B=0, ops=64)
    # a device address needs its shape
    with pytest.raises(ValueError, match="needs B"):
        gtn.edit_distance(64, 64, 64, 64, 64, N=1, L=2, U=2, hyp_stride=2, ref_stride=2)
    with pytest.raises(ValueError, match="needs hyp_stride"):
        gtn.edit_distance(64, 64, 64, 64, 64, B=1, N=1, L=2, U=2)
    # tensors of the wrong kind are refused by the Python layer, not read as reinterpreted bits
    hyp, hl = torch.zeros(2, 3, 8, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int32)
    ref, rl = torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    dist, ops = torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3, 3, dtype=torch.int32)
    for args, msg in (((hyp.long(), hl, ref, rl, dist), "hyp must be an int32"),
                      ((hyp[0, 0], hl, ref, rl, dist), "hyp must be an int32"),
                      ((hyp.transpose(1, 2), hl, ref, rl, dist), "contiguous rows"),
                      ((hyp, hl, ref.float(), rl, dist), "ref must be an int32"),
                      ((hyp, hl, ref.t(), rl, dist), "B = 2 is not what the tensors say"),
                      ((hyp, hl, ref[:, ::2], rl, dist), "ref must have contiguous rows"),
                      ((hyp, hl.long(), ref, rl, dist), "hyp_lengths must be"),
                      ((hyp, hl[:, :2], ref, rl, dist), "hyp_lengths must be"),
                      ((hyp, hl, ref, rl.long(), dist), "ref_lengths must be"),
                      ((hyp, hl, ref, rl, dist.float()), "dist_out must be"),
                      ((hyp, hl, ref, rl, dist[:1]), "dist_out must be"),
                      ((hyp, hl, ref, rl, dist, ops[:, :, :2]), "ops_out must be"),
                      ((hyp, hl, ref, rl, dist, ops), "must be a CUDA tensor")):
        with pytest.raises(ValueError, match=msg):
            gtn.edit_distance(*args)
    with pytest.raises(ValueError, match="hyp_stride is not the row stride"):
        gtn.edit_distance(hyp, hl, ref, rl, dist, hyp_stride=9)
    with pytest.raises(ValueError, match="N = 2 is not what the tensors say"):
        gtn.edit_distance(hyp, hl, ref, rl, dist, N=2)
    # the C ABI itself: 1 is GTNX_INVALID_ARGUMENT, 0 the empty call
    p = ctypes.c_void_p
    f = gtn_amd._lib.gtnx_batch_edit_distance
    assert f(None, 8, p(64), p(64), 5, p(64), 2, 3, 8, 5, p(64), None) == 1
    assert f(p(64), 8, None, p(64), 5, p(64), 2, 3, 8, 5, p(64), None) == 1
    assert f(p(64), 8, p(64), None, 5, p(64), 2, 3, 8, 5, p(64), None) == 1
    assert f(p(64), 8, p(64), p(64), 5, None, 2, 3, 8, 5, p(64), None) == 1
    assert f(p(64), 8, p(64), p(64), 5, p(64), 2, 3, 8, 5, None, p(64)) == 1
    assert f(p(64), 8, p(64), p(64), 5, p(64), -2, 3, 8, 5, p(64), None) == 1
    assert f(p(64), 7, p(64), p(64), 5, p(64), 2, 3, 8, 5, p(64), None) == 1
    assert f(p(64), 8, p(64), p(64), 4, p(64), 2, 3, 8, 5, p(64), None) == 1
    assert f(p(64), 8, p(64), p(64), 5, p(64), 0, 3, 8, 5, p(64), None) == 0
    assert gtn.debug_edit_distance_stats() == before  # nothing refused or empty has counted
    # torch_loss: shapes and dtypes first, then the device
    for args, msg in (((hyp.long(), hl, ref, rl), "hyp must be an int32"), ((hyp[0, 0], hl, ref, rl), "hyp must be"),
                      ((hyp, hl, ref[:1], rl), "ref must be an int32 tensor"), ((hyp, hl, ref.long(), rl), "ref must be"),
                      ((hyp, hl[:, 0], ref, rl), "hyp_lengths must be"), ((hyp, hl.float(), ref, rl), "hyp_lengths must"),
                      ((hyp, hl, ref, rl[:1]), "ref_lengths must be"), ((hyp[:, 0], hl, ref, rl), "hyp_lengths must be"),
                      ((torch.zeros(1, 1, 65537, dtype=torch.int32), hl[:1, :1], ref[:1], rl[:1]), "wider than"),
                      ((hyp, hl, torch.zeros(2, 4097, dtype=torch.int32), rl), "wider than")):
        with pytest.raises(ValueError, match=msg):
            torch_loss.edit_distance(*args)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        torch_loss.edit_distance(hyp, hl, ref, rl)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        torch_loss.edit_distance(hyp[:, 0], hl[:, 0].long(), ref, rl.long(), return_ops=True)


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU behaviour (test_edit_distance_gpu.py launches these widths)")
def test_widths_of_4096_are_taken(gtn):
    """L and U of 4096 pass the argument checks: the call gets as far as the lack of a device"""
    kw = dict(B=1, N=1, L=4096, U=4096, hyp_stride=4096, ref_stride=4096)
    with pytest.raises(RuntimeError, match="no HIP device"):
        gtn.edit_distance(64, 64, 64, 64, 64, **kw)
    with pytest.raises(RuntimeError, match="no HIP device"):
        gtn.edit_distance(64, 64, 64, 64, 64, **{**kw, "L": 65536, "hyp_stride": 65536})


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU behaviour")
def test_edit_distance_fails_loudly_without_gpu(gtn):
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    lib.gtn_edit_distance_n.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 2
    lib.gtn_edit_distance_n.restype = ctypes.c_int
    lib.gtn_criteria_last_error.restype = ctypes.c_char_p
    p = ctypes.c_void_p
    rc = lib.gtn_edit_distance_n(p(64), p(64), p(64), p(64), 1, 2, 8, 8, p(64), None)
    assert rc == -1 and "no HIP device" in lib.gtn_criteria_last_error().decode()
    rc = lib.gtn_edit_distance_n(None, p(64), p(64), p(64), 1, 2, 8, 8, p(64), None)
    assert rc == -1 and "null input pointer" in lib.gtn_criteria_last_error().decode()
    with pytest.raises(RuntimeError, match="no HIP device"):
        gtn.edit_distance(64, 64, 64, 64, 64, None, B=1, N=1, L=2, U=2, hyp_stride=2, ref_stride=2)
    # a call that could not launch has not counted
    before = gtn.debug_edit_distance_stats()
    with pytest.raises(RuntimeError, match="no HIP device"):
        gtn.edit_distance(64, 64, 64, 64, 64, 64, B=1, N=1, L=2, U=2, hyp_stride=2, ref_stride=2)
    assert gtn.debug_edit_distance_stats() == before
