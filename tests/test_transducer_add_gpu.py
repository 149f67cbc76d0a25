"""The transducer score under an additive joint on the GPU (gtn_amd/csrc/transducer_add.hip): scores and
the two weighted gradients against the float64 yardstick of tests/transducer_fp.py on the summed tensor am[:, :, None] +
lm[:, None], at the gates score 1e-4 max(1, |want|) and gradient 1e-4 max(1, |want|) per element (an element is a sum of
up to 65 node gradients, each held to 1e-4 absolute by section 42), rows past the lengths == 0, and the contract's
promises about bits.  Every output carries a guard row of sentinels."""
import functools
import math

import numpy as np
import pytest

import transducer_fp as fp

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0
CAP = "GTNX_TRANSDUCER_SCRATCH_BYTES"
# tile edges of T and U + 1 at 32 and 64, the chunk edges of C, the aligned and unaligned loads, the degenerate lattice
SHAPES = [(33, 31, 5), (32, 32, 64), (65, 63, 17), (64, 64, 33), (31, 33, 129), (17, 15, 260), (3, 2, 1025), (1, 0, 1),
          (2, 1, 3), (5, 4, 4)]


def _reference(am, lm, targets, frames, tlens, blank, w):
    """(scores, grad_am, grad_lm) in float64 from the yardstick on the summed tensor"""
    x = am.astype(np.float64)[:, :, None, :] + lm.astype(np.float64)[:, None, :, :]
    scores, g = fp.reference(x, targets, frames, tlens, blank, True, w)
    return scores, g.sum(axis=2), g.sum(axis=1)


@functools.lru_cache(maxsize=None)
def _case(T, U, C):
    """(am, lm, targets, frames, tlens, blank, w, want scores, want grad_am, want grad_lm) of a seeded case, read-only"""
    B, blank = 4, C // 2
    rng = np.random.default_rng(1000 * T + 10 * U + C)
    am, lm = rng.standard_normal((B, T, C)), rng.standard_normal((B, U + 1, C))
    targets = np.zeros((B, U), np.int32)
    if U:
        targets[:] = (blank + 1 + rng.integers(0, C - 1, (B, U))) % C
    am[:, :, blank] += 3 + math.log(C)
    for u in range(U):
        lm[np.arange(B), u, targets[:, u]] += 3 + math.log(C)
    am, lm = am.astype(np.float32), lm.astype(np.float32)
    frames = np.asarray([T, rng.integers(1, T + 1), 1, 0], np.int32)
    tlens = np.asarray([U, rng.integers(0, U + 1), 0, rng.integers(0, U + 1)], np.int32)
    out = (am, lm, targets, frames, tlens, blank, fp.WEIGHTS) + _reference(am, lm, targets, frames, tlens, blank, fp.WEIGHTS)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True)).to("cuda:0")


def _run(gtn, am, lm, targets, frames, tlens, blank, w, keep_rows=False):
    """gtn.transducer_add_score and _score_grad -> (scores [B], grad_am [B, T, C], grad_lm [B, U + 1, C]) as numpy"""
    import torch
    (B, T, C), U1 = am.shape, lm.shape[1]
    ad, ld, args = _dev(am), _dev(lm), (_dev(targets), _dev(frames), _dev(tlens))
    sc = torch.full((B + 1,), SENTINEL, device="cuda:0")
    ga = torch.full((B + 1, T, C), SENTINEL, device="cuda:0")
    gl = torch.full((B + 1, U1, C), SENTINEL, device="cuda:0")
    rows = torch.full((B + 1, T, U1, 3), SENTINEL, device="cuda:0") if keep_rows else None
    torch.cuda.synchronize()
    c0 = gtn.debug_transducer_add_stats()
    gtn.transducer_add_score(ad, ld, *args, sc[:B], None if rows is None else rows[:B], blank)
    gtn.transducer_add_score_grad(ad, ld, *args, _dev(w), ga[:B], gl[:B], None if rows is None else rows[:B], blank)
    gtn.synchronize()
    c1 = gtn.debug_transducer_add_stats()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (2, 2 * B)
    for have, was in ((ad, am), (ld, lm)):  # only read
        assert (have.cpu().numpy().view(np.int32) == np.asarray(was).view(np.int32)).all()
    for guarded in (sc, ga, gl, rows):
        assert guarded is None or (guarded[-1] == SENTINEL).all(), "guard row"
    return sc[:B].cpu().numpy(), ga[:B].cpu().numpy(), gl[:B].cpu().numpy()


def _check(name, got, want, frames, tlens):
    """the gates of the module's docstring: got and want are (scores, grad_am, grad_lm)"""
    assert not any(np.isnan(g).any() for g in got), name
    for b, (have, ref) in enumerate(zip(got[0], want[0])):
        print(f"{name} b={b} score {have!r} want {ref!r}")
        assert have == ref if np.isinf(ref) else abs(have - ref) <= 1e-4 * max(1.0, abs(ref)), (name, b, have, ref)
    for what, have, ref, lens in (("grad_am", got[1], want[1], frames), ("grad_lm", got[2], want[2], tlens + 1)):
        err = np.abs(have - ref) / np.maximum(1.0, np.abs(ref))
        print(f"{name} {what} worst error over its gate's scale {err.max():.3g}, largest |want| {np.abs(ref).max():.3g}")
        assert err.max() <= 1e-4, (name, what)
        for b in range(len(lens)):
            valid = 1 <= frames[b] <= got[1].shape[1] and 0 <= tlens[b] < got[2].shape[1] and np.isfinite(want[0][b])
            assert not have[b, lens[b] if valid else 0:].any(), (name, what, b)


def _same_bits(a, b):
    return all((x.view(np.int32) == y.view(np.int32)).all() for x, y in zip(a, b))


# ---- 1. against float64 ----
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_scores_and_gradients_against_float64(gtn, shape):
    am, lm, targets, frames, tlens, blank, w, *want = _case(*shape)
    _check(str(shape), _run(gtn, am, lm, targets, frames, tlens, blank, w), want, frames, tlens)


# ---- 2. the same answer as the materialised route ----
@pytest.mark.parametrize("shape", [(33, 31, 5), (31, 33, 129)], ids=str)
def test_agrees_with_the_score_of_the_summed_tensor(gtn, shape):
    import torch
    am, lm, targets, frames, tlens, blank, w = _case(*shape)[:7]
    z = _dev(am)[:, :, None, :] + _dev(lm)[:, None, :, :]
    args = (_dev(targets), _dev(frames), _dev(tlens))
    sc, g = torch.empty(4, device="cuda:0"), torch.empty_like(z)
    gtn.transducer_score(z, *args, sc, None, blank, True)
    gtn.transducer_score_grad(z, *args, _dev(w), g, None, blank, True)
    gtn.synchronize()
    g = g.cpu().numpy().astype(np.float64)
    _check(str(shape), _run(gtn, am, lm, targets, frames, tlens, blank, w),
           (sc.cpu().numpy(), g.sum(axis=2), g.sum(axis=1)), frames, tlens)


# ---- 3. the same bits: run to run, sliced, alone, with the rows plane, with NaN in the rows that are never read ----
def test_runs_slices_neighbours_rows_and_unread_rows_change_no_bit(gtn, monkeypatch):
    am, lm, targets, frames, tlens, blank, w = _case(65, 63, 17)[:7]
    whole = _run(gtn, am, lm, targets, frames, tlens, blank, w)
    assert _same_bits(whole, _run(gtn, am, lm, targets, frames, tlens, blank, w))
    assert _same_bits(whole, _run(gtn, am, lm, targets, frames, tlens, blank, w, keep_rows=True))
    monkeypatch.setenv(CAP, "1")  # (one utterance per slice)
    assert _same_bits(whole, _run(gtn, am, lm, targets, frames, tlens, blank, w))
    monkeypatch.delenv(CAP)
    one = _run(gtn, am[:1], lm[:1], targets[:1], frames[:1], tlens[:1], blank, w[:1])
    assert _same_bits([x[:1] for x in whole], one)
    am_nan, lm_nan = am.copy(), lm.copy()
    for b in range(4):
        am_nan[b, frames[b]:] = np.nan
        lm_nan[b, tlens[b] + 1:] = np.nan
    assert np.isnan(am_nan[3]).all()  # (the T_b == 0 utterance)
    assert _same_bits(whole, _run(gtn, am_nan, lm_nan, targets, frames, tlens, blank, w))


# ---- 4. dead rows and bad tokens ----
def test_dead_rows_and_bad_tokens(gtn):
    am, lm, targets, frames, tlens, blank, w = (np.array(a) for a in _case(5, 4, 4)[:7])
    am[0, 2, 1] = np.nan  # a live frame of utterance 0: the paths through it die, and every path crosses every frame
    got = _run(gtn, am, lm, targets, frames, tlens, blank, w)
    assert np.isneginf(got[0][0]) and np.isfinite(got[0][1:3]).all() and got[1][1].any()
    _check("nan row", got, _reference(am, lm, targets, frames, tlens, blank, w), frames, tlens)
    # utterance 0 three times: as it is, with an all -inf lm row, with a token equal to blank
    am3, lm3, tg3 = (np.repeat(x[:1], 3, axis=0) for x in _case(5, 4, 4)[:3])
    lm3[1, 2] = -np.inf
    tg3[2, 1] = blank
    full, w3 = np.asarray([5, 5, 5], np.int32), np.asarray([1.25, -0.75, 0.5], np.float32)
    got = _run(gtn, am3, lm3, tg3, full, full - 1, blank, w3)
    assert np.isneginf(got[0][1:]).all() and not got[1][1:].any() and not got[2][1:].any()
    _check("-inf", got, _reference(am3, lm3, tg3, full, full - 1, blank, w3), full, full - 1)
    alone = _run(gtn, am3[:1], lm3[:1], tg3[:1], full[:1], full[:1] - 1, blank, w3[:1])
    assert _same_bits([x[:1] for x in got], alone)  # (the neighbours are unaffected)


# ---- 5. the torch entry: the mean loss and both gradients ----
def test_torch_entry(gtn):
    import gtn_amd.torch_loss as tl
    am, lm, targets, frames, tlens, blank = _case(5, 4, 4)[:6]
    want = _reference(am, lm, targets, frames, tlens, blank, np.full(4, -0.25))
    ad, ld = _dev(am).requires_grad_(True), _dev(lm).requires_grad_(True)
    args = (_dev(targets).long(), _dev(frames).long(), _dev(tlens), blank)
    loss = tl.transducer_add_loss(ad, ld, *args, reduction="mean")
    loss.backward()
    assert loss.item() == np.inf  # (the utterance without a frame has loss +inf, and a zero gradient)
    none = tl.transducer_add_loss(ad, ld, *args, reduction="none")
    assert none.shape == (4,)
    _check("torch", (-none.detach().cpu().numpy(), ad.grad.cpu().numpy(), ld.grad.cpu().numpy()), want, frames, tlens)
