"""ASG loss over padded batches, the parts that need no GPU.

The float64 yardstick of tests/test_asg_frames_gpu.py (tests/asg_loss_fp.py) is pinned to the oracle on the lattices
the reference would build for an utterance of T_b frames -- linear o transitions and (forceAlign o transitions) o
linear -- and the new entry points exist and check their arguments before the engine looks for a device.
"""
import ctypes as C
import os

import numpy as np
import pytest

from asg_full_f32 import batch_f32
from asg_loss_fp import (DEAD_CASE, EDGE_SHAPES, GPU_SHAPES, LONG_SHAPES, MANY_CASE, SECOND_SEED, SEEDS, asg_loss_fp64,
                         asg_terms_fp64, kill_emissions, seeded_case, shape_seed)
from conftest import ROOT
from ctc_fp64 import asg_fp64
from oracle_lib import OGraph

# (seed, B, T, N, Umax)
ORACLE_CASES = [(31, 3, 1, 2, 1), (32, 3, 4, 3, 3), (33, 4, 7, 5, 4), (34, 4, 13, 8, 6), (35, 3, 9, 4, 9)]


def transitions_dict(trans, start):
    N = len(start)
    d = {"start": [1] + [0] * N, "accept": [0] + [1] * N, "src": [], "dst": [], "il": [], "ol": [], "w": [], "sort": "i"}
    for i in range(N):
        d["src"].append(0), d["dst"].append(i + 1), d["il"].append(i), d["ol"].append(i), d["w"].append(float(start[i]))
    for i in range(N):
        for j in range(N):
            d["src"].append(j + 1), d["dst"].append(i + 1), d["il"].append(i), d["ol"].append(i)
            d["w"].append(float(trans[i, j]))
    return d


def force_align_dict(target):
    U = len(target)
    d = {"start": [1] + [0] * U, "accept": [int(U == 0)] + [int(l == U) for l in range(1, U + 1)],
         "src": [], "dst": [], "il": [], "ol": [], "w": [], "sort": None}
    for l in range(1, U + 1):
        for s in (l - 1, l):
            d["src"].append(s), d["dst"].append(l), d["il"].append(target[l - 1]), d["ol"].append(target[l - 1])
            d["w"].append(0.0)
    return d


def oracle_asg(em, trans, start, target):
    """(fcc, fal, d loss / d em [T, N], d loss / d transitions [N + N * N]) through the oracle's graph functions"""
    T, N = em.shape
    td = transitions_dict(trans, start)
    A = len(td["src"])
    lin = OGraph.linear(T, N, em.reshape(-1))
    tr = OGraph.from_dict(td)
    fc = lin.compose(tr)
    fcc = fc.shortest_distance()
    f_em, f_tr = fc.compose_grad(fc.shortest_distance_grad(), T * N, A)
    fd = force_align_dict(target)
    fa = OGraph.from_dict(fd).compose(OGraph.from_dict(td))
    al = fa.compose(OGraph.linear(T, N, em.reshape(-1)))
    fal = al.shortest_distance()
    g_fa, a_em = al.compose_grad(al.shortest_distance_grad(), fa.A, T * N)
    _, a_tr = fa.compose_grad(g_fa, len(fd["src"]), A)
    return fcc, fal, (f_em - a_em).reshape(T, N), f_tr - a_tr


@pytest.mark.parametrize("case", ORACLE_CASES, ids=str)
def test_fp64_yardstick_is_the_oracle_on_the_lattices_the_reference_builds(case):
    em, trans, start, targets, frames = seeded_case(*case)
    for b in range(len(targets)):
        f = int(frames[b])
        want = asg_terms_fp64(em[b], trans, start, targets[b], f)
        fcc, fal, g_em, g_tr = oracle_asg(em[b, :f], trans, start, targets[b])
        tol = 1e-5 * max(1.0, abs(want["fcc"]), abs(want["fal"]))  # (the oracle is float32)
        assert abs(fcc - want["fcc"]) <= tol and abs(fal - want["fal"]) <= tol
        assert abs((fcc - fal) - want["loss"]) <= 2 * tol
        np.testing.assert_allclose(g_em, want["g_em"][:f], rtol=0, atol=1e-5)
        np.testing.assert_allclose(g_tr, want["g_tr"], rtol=0, atol=1e-5)
        assert not want["g_em"][f:].any()


def test_frames_k_is_the_yardstick_on_the_first_k_rows():
    em, trans, start, targets, _ = seeded_case(41, 3, 11, 6, 5)
    for b, t in enumerate(targets):
        for k in (len(t), len(t) + 1, 11):
            loss, g_em, g_tr = asg_loss_fp64(em[b], trans, start, t, k)
            want = asg_loss_fp64(em[b, :k], trans, start, t)
            assert loss == want[0]
            assert np.array_equal(g_em[:k], want[1]) and not g_em[k:].any()
            assert np.array_equal(g_tr, want[2])
    # fewer frames than labels: no alignment, the loss is +inf and the gradient is the full-connect term's alone
    loss, g_em, g_tr = asg_loss_fp64(em[0], trans, start, [1, 2, 3, 4], 3)
    assert loss == np.inf and np.isfinite(g_em).all() and np.isfinite(g_tr).all()
    np.testing.assert_allclose(g_em[:3].sum(1), 1.0, rtol=1e-12)


def test_yardstick_with_forbidden_transitions():
    em, trans, start, _, _ = seeded_case(42, 2, 8, 5, 4)
    trans = trans.astype(np.float64)
    trans[2, 2] = -np.inf          # label 2 may not repeat
    start = start.astype(np.float64)
    start[[0, 3]] = -np.inf
    loss, g_em, g_tr = asg_loss_fp64(em[0], trans, start, [1, 2, 4, 2], 8)
    assert np.isfinite(loss) and np.isfinite(g_em).all() and np.isfinite(g_tr).all()
    N = 5
    assert g_tr[N + 2 * N + 2] == 0.0 and g_tr[0] == 0.0 and g_tr[3] == 0.0
    # the same utterance needs 2 -> 2 once: no alignment, and the full-connect term still has paths
    loss, g_em, _ = asg_loss_fp64(em[0], trans, start, [1, 2, 2], 8)
    assert loss == np.inf and np.isfinite(g_em).all()


def test_asg_loss_input_lengths_are_checked_before_the_device():
    """torch_loss.asg_loss takes input_lengths; a wrong count or a value outside 1 .. T is a ValueError raised from
    host tensors -- before the emissions are looked at, whatever the machine"""
    import inspect

    import torch
    import gtn_amd.torch_loss as tl
    assert "input_lengths" in inspect.signature(tl.asg_loss).parameters
    em = torch.zeros(2, 4, 3)
    tr = torch.zeros(3, 3)
    for bad in ([4], [4, 4, 4]):
        with pytest.raises(ValueError, match="input lengths for a batch"):
            tl.asg_loss(em, tr, [[0], [1]], input_lengths=bad)
    for bad in ([0, 4], [4, 5], [-1, 2], torch.tensor([1, 9])):
        with pytest.raises(ValueError, match="outside 1 .. 4"):
            tl.asg_loss(em, tr, [[0], [1]], input_lengths=bad)


def test_new_entry_points_exist_in_the_built_libraries():
    import gtn_amd
    eng = gtn_amd._lib
    assert hasattr(eng, "gtnx_batch_full_connect_stats")
    fast, fallback = gtn_amd.debug_full_connect_stats()
    assert fast >= 0 and fallback >= 0
    crit = C.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    assert hasattr(crit, "gtn_asg_loss_frames_n") and hasattr(crit, "gtn_asg_loss_n")
    # null frame counts and counts outside 1 .. T are refused before anything is launched
    crit.gtn_asg_loss_frames_n.restype = C.c_int
    crit.gtn_criteria_last_error.restype = C.c_char_p
    args = [C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), 2, 4, 3, C.c_void_p(0)]
    assert crit.gtn_asg_loss_frames_n(*args, C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0)) == -1
    assert b"null frame counts" in crit.gtn_criteria_last_error()
    for frames in ([0, 4], [4, 5]):
        fr = np.asarray(frames, np.int32)
        assert crit.gtn_asg_loss_frames_n(*args, C.c_void_p(fr.ctypes.data), C.c_void_p(0), C.c_void_p(0),
                                          C.c_void_p(0)) == -1
        assert b"frame count outside 1 .. T" in crit.gtn_criteria_last_error()


# ---- the recursion of asg_full.hip in float32 (tests/asg_full_f32.py) against float64 ---------------------------------
# CONDITION: at every shape and scale tests/test_asg_frames_gpu.py launches, the float32 transcription of the kernels
# stays within HALF of each gate the GPU tests apply -- score 1e-4 * max(1, |z|), emission gradient 1e-4 absolute,
# transitions rtol 1e-3 / atol 1e-4 -- so that a GPU test which misses its gate there says "the kernel is wrong", not
# "float32 in this design cannot do it".  A shape that does not meet the condition is replaced, the gate never widened.
LETTERS = (5, 40, 27, 9)


def _shape_batch(shape, em_scale=1.0):
    em, trans, start, _, frames = seeded_case(shape_seed(shape), *shape, em_scale)
    return em, trans, start, frames


def _forbidden_batch():
    em, trans, start, _, _ = seeded_case(77, 4, 14, 9, 5)
    trans, start = trans.copy(), start.copy()
    trans[3, 3] = trans[5, 5] = trans[1, 6] = -np.inf
    start[[0, 4, 8]] = -np.inf
    return em, trans, start, np.asarray([14, 2, 1, 9], np.int32)


def _second_batch():
    _, trans, start, _ = _shape_batch((4, 12, 5, 4))
    em, _, _, _, frames = seeded_case(SECOND_SEED, 4, 12, 5, 4)
    return em, trans, start, frames


def _many_batch():
    em, trans, start, _, frames = seeded_case(*MANY_CASE)
    return em, trans, start, frames


F32_CASES = ([(str(s), _shape_batch, (s,), None) for s in GPU_SHAPES + EDGE_SHAPES + LONG_SHAPES] +
             [(f"{s} x30", _shape_batch, (s, 30.0), None) for s in [(4, 12, 5, 4), LETTERS]] +
             [("forbidden", _forbidden_batch, (), None), ("second batch", _second_batch, (), None),
              ("many", _many_batch, (), None), (f"{LETTERS} seeds", _shape_batch, (LETTERS,), SEEDS)])


def _f32_against_fp64(tag, em, trans, start, frames, delta=None, skip=()):
    """figures of the transcription against asg_fp64 over a batch, printed: (worst score error / its gate, worst
    emission gradient error, worst transitions error / its gate); utterances in `skip` have no yardstick"""
    B, T, N = em.shape
    tw = np.concatenate([start, trans.reshape(-1)]).astype(np.float64)
    d = np.ones(B) if delta is None else np.asarray(delta, np.float64)
    Z, ge, gtr = batch_f32(em, trans, start, frames, delta)
    assert not np.isnan(ge).any() and not np.isnan(gtr).any()
    want_tr = np.zeros(N + N * N)
    sc = emg = 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        for b in range(B):
            f = int(frames[b])
            assert not ge[b, f:].any()
            if b in skip:
                continue
            z, w_em, w_tr = asg_fp64(em[b, :f], tw)[:3]
            want_tr += d[b] * w_tr
            sc = max(sc, abs(float(np.float32(Z[b])) - z) / (1e-4 * max(1.0, abs(z))))
            emg = max(emg, np.abs(ge[b, :f] - d[b] * w_em).max())
    trg = (np.abs(gtr - want_tr) / (1e-4 + 1e-3 * np.abs(want_tr))).max()
    print(f"float32 transcription {tag}: score error / gate {sc:.2e}, em grad abs {emg:.2e} (gate 1e-4), "
          f"transitions error / gate {trg:.2e}")
    return sc, emg, trg


@pytest.mark.parametrize("case", F32_CASES, ids=lambda c: c[0])
def test_float32_recursion_is_within_half_of_every_gate(case):
    tag, make, args, delta = case
    sc, emg, trg = _f32_against_fp64(tag, *make(*args), delta=delta)
    assert sc <= 0.5 and emg <= 0.5e-4 and trg <= 0.5, (tag, sc, emg, trg)


def test_float32_recursion_with_dead_emissions_and_a_dead_utterance():
    """-inf emissions are probability 0; the utterance without a path scores -inf and its gradient is zeros that were
    stored, not multiplied; nothing is NaN (the float64 yardstick is NaN on that utterance and is not asked)"""
    em, trans, start, _, frames = seeded_case(*DEAD_CASE)
    assert frames.tolist() == [12, 4, 1, 5]
    em = kill_emissions(em)
    Z, ge, _ = batch_f32(em, trans, start, frames)
    assert Z[1] == -np.inf and np.isfinite(np.delete(Z, 1)).all()
    assert not ge[1].any() and not ge[np.isneginf(em)].any()
    sc, emg, trg = _f32_against_fp64("dead", em, trans, start, frames, skip=(1,))
    assert sc <= 0.5 and emg <= 0.5e-4 and trg <= 0.5


def test_float32_limit_on_a_long_utterance_at_emissions_x30_is_printed():
    """MEASURED LIMIT, printed and not asserted: at (4, 1200, 27, 30) with the emissions scaled by 30 the float32
    recursion misses the 1e-4 emission-gradient gate (6.2e-4 here; transitions 0.56 of their gate).  Log-domain
    values of magnitude ~100 are stored in float32 over ~1000 steps, the forward and the backward rounding walk
    independently (about sqrt(T) ulp), and gamma is the exponential of their sum.  That is a property of the storage
    format, not of the kernel, so this case is not launched on the GPU (Dynamic range); the same
    shape at scale 1 is, and is held to the condition here."""
    shape = LONG_SHAPES[0]
    _f32_against_fp64(f"{shape} x30", *_shape_batch(shape, 30.0))
    sc, emg, trg = _f32_against_fp64(str(shape), *_shape_batch(shape))
    assert sc <= 0.5 and emg <= 0.5e-4 and trg <= 0.5
