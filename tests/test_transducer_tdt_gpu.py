"""The batched token-and-duration transducer (TDT) score on the GPU (gtn_amd/csrc/transducer_tdt.hip, DESIGN section
47): scores and weighted gradients against the float64 yardstick of tests/transducer_tdt_fp.py at the project's gates
(score 1e-4 max(1, |want|), gradient 1e-4 absolute, never-read rows == 0), and the contract's promises about bits:
never-read rows are never read, -inf never turns into NaN and leaves the neighbours alone, and a second run, a sliced
call, an utterance alone and the caller's rows plane all give the same bits.  Every output carries a guard row of
sentinels."""
import numpy as np
import pytest

import transducer_tdt_fp as fp

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0
CAP = "GTNX_TRANSDUCER_SCRATCH_BYTES"


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True)).to("cuda:0")  # (the cached cases are read-only)


def _run(gtn, x, targets, frames, tlens, blank, w, D, sigma=0.0, keep_rows=False):
    """gtn.transducer_tdt_score and gtn.transducer_tdt_score_grad -> (scores [B], grad [B, T, U + 1, C + D]) as numpy"""
    import torch
    B, T, U1, CD = x.shape
    xd, args = _dev(x), (_dev(targets), _dev(frames), _dev(tlens))
    sc = torch.full((B + 1,), SENTINEL, device="cuda:0")
    g = torch.full((B + 1, T, U1, CD), SENTINEL, device="cuda:0")
    rows = torch.full((B + 1, T, U1, D + 4), SENTINEL, device="cuda:0") if keep_rows else None
    torch.cuda.synchronize()
    c0 = gtn.debug_transducer_tdt_stats()
    gtn.transducer_tdt_score(xd, *args, sc[:B], D, None if rows is None else rows[:B], blank, sigma)
    gtn.transducer_tdt_score_grad(xd, *args, _dev(w), g[:B], D, None if rows is None else rows[:B], blank, sigma)
    gtn.synchronize()
    c1 = gtn.debug_transducer_tdt_stats()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (2, 2 * B)
    assert (xd.cpu().numpy().view(np.int32) == np.asarray(x).view(np.int32)).all()  # only read
    for guarded in (sc, g, rows):
        assert guarded is None or (guarded[-1] == SENTINEL).all(), "guard row"
    return sc[:B].cpu().numpy(), g[:B].cpu().numpy()


def _same_bits(a, b):
    return all((x.view(np.int32) == y.view(np.int32)).all() for x, y in zip(a, b))


# ---- 1. and 2. against float64, without and with sigma ----
@pytest.mark.parametrize("shape,sigma", [(s, 0.0) for s in fp.SHAPES] + [((65, 63, 5, 5), 0.05), ((5, 4, 4, 3), 0.05)],
                         ids=str)
def test_scores_and_gradients_against_float64(gtn, shape, sigma):
    x, targets, frames, tlens, blank, w, *want = fp.case(*shape, sigma)
    got = _run(gtn, x, targets, frames, tlens, blank, w, shape[3], sigma)
    fp.check(str(shape), *got, *want, frames, tlens)


# ---- 3. never-read rows are never read ----
def test_nan_in_the_never_read_rows_changes_no_bit(gtn):
    x, targets, frames, tlens, blank, w = fp.case(70, 129, 8, 4)[:6]
    x_nan = x.copy()
    for b in range(len(frames)):
        x_nan[b, frames[b]:] = np.nan
        x_nan[b, :, tlens[b] + 1:] = np.nan
    assert np.isnan(x_nan[3]).all()  # (the T_b == 0 utterance)
    assert _same_bits(_run(gtn, x_nan, targets, frames, tlens, blank, w, 4), _run(gtn, x, targets, frames, tlens, blank, w, 4))


# ---- 4. -inf is probability 0, and what scores -inf has a zero gradient ----
def test_minus_inf_dead_rows_and_invalid_utterances(gtn):
    C, D = 4, 3
    x, targets, frames, tlens, blank, _ = (np.array(a) for a in fp.case(5, 4, C, D)[:6])
    x, targets = np.concatenate([x, x, x[:1]]), np.concatenate([targets, targets, targets[:1]])
    frames = np.asarray([5, 5, 5, 0, 5, 5, 6, 5, 5], np.int32)  # (3: T_b == 0; 6: T_b > T)
    tlens = np.asarray([4, 4, 2, 3, 4, 4, 4, 5, 4], np.int32)   # (7: U_b > U)
    w = np.asarray([1.25, -0.75, 0.5, 1.0, 2.0, 1.5, 1.0, 1.0, 0.5], np.float32)
    x[0, 1, 2, :2] = -np.inf                           # -inf entries in either segment: paths remain
    x[0, 2, 1, blank], x[0, 3, 3, C + 1] = -np.inf, -np.inf
    x[1, 2, 1, 0], x[1, 3, 0, :C] = np.nan, -np.inf    # dead rows by the token segment: paths remain around them
    x[1, 1, 3, C + 2], x[1, 2, 3, C:] = np.inf, -np.inf  # ... and by the duration segment
    x[2, :, 1, 3] = np.inf                             # a dead column: no path
    targets[4, 2] = C                                  # a token outside 0 .. C - 1
    targets[5, 0] = blank                              # a token equal to blank
    x[8, :, :, C + 1:] = -np.inf                       # only duration 0 left: no blank arc, no path
    got = _run(gtn, x, targets, frames, tlens, blank, w, D)
    assert np.isneginf(got[0][2:]).all() and not got[1][2:].any()
    assert np.isfinite(got[0][:2]).all() and got[1][0].any() and got[1][1].any()
    for dead in ((2, 1), (3, 0), (1, 3), (2, 3)):
        assert not got[1][1][dead].any(), dead
    fp.check("-inf", *got, *fp.reference(x, targets, frames, tlens, C, blank, 0.0, w), frames, tlens)
    alone = _run(gtn, x[:2], targets[:2], frames[:2], tlens[:2], blank, w[:2], D)
    assert _same_bits((got[0][:2], got[1][:2]), alone)  # (the neighbours are unaffected)


# ---- 5. the same bits: run to run, sliced, alone, with or without the rows plane ----
@pytest.mark.parametrize("shape", [(70, 129, 8, 4), (3, 2, 4095, 5)], ids=str)
def test_runs_slices_neighbours_and_rows_change_no_bit(gtn, shape, monkeypatch):
    x, targets, frames, tlens, blank, w = fp.case(*shape)[:6]
    D = shape[3]
    whole = _run(gtn, x, targets, frames, tlens, blank, w, D)
    assert _same_bits(whole, _run(gtn, x, targets, frames, tlens, blank, w, D))
    assert _same_bits(whole, _run(gtn, x, targets, frames, tlens, blank, w, D, keep_rows=True))
    monkeypatch.setenv(CAP, "1")  # (one utterance per slice)
    assert _same_bits(whole, _run(gtn, x, targets, frames, tlens, blank, w, D))
    assert _same_bits(whole, _run(gtn, x, targets, frames, tlens, blank, w, D, keep_rows=True))
    monkeypatch.delenv(CAP)
    for b in range(len(frames)):
        one = _run(gtn, x[b:b + 1], targets[b:b + 1], frames[b:b + 1], tlens[b:b + 1], blank, w[b:b + 1], D)
        assert _same_bits((whole[0][b:b + 1], whole[1][b:b + 1]), one), b


# ---- 6. the torch entry under a non-uniform grad_out with int64 index tensors, and the mean loss ----
def test_torch_entry(gtn):
    import gtn_amd.torch_loss as tl
    x, targets, frames, tlens, blank, w, want_scores, want_grad = fp.case(5, 4, 4, 3, 0.05)
    xd = _dev(x).requires_grad_(True)
    args = (_dev(targets).long(), _dev(frames).long(), _dev(tlens).long(), 3, blank, 0.05)
    out = tl.transducer_tdt_score(xd, *args)
    out.backward(_dev(w))
    fp.check("torch", out.detach().cpu().numpy(), xd.grad.cpu().numpy(), want_scores, want_grad, frames, tlens)
    live = [0, 1, 2]  # (the utterance without a frame has loss +inf)
    xl = _dev(x[live]).requires_grad_(True)
    loss = tl.transducer_tdt_loss(xl, *(a[live] for a in args[:3]), *args[3:], reduction="mean")
    loss.backward()
    unit = fp.reference(x[live], targets[live], frames[live], tlens[live], 4, blank, 0.05, np.full(3, -1.0 / 3))
    assert abs(loss.item() + want_scores[live].mean()) <= 1e-4 * max(1.0, abs(want_scores[live].mean()))
    assert np.abs(xl.grad.cpu().numpy() - unit[1]).max() <= 1e-4
    assert tl.transducer_tdt_loss(_dev(x), *args, reduction="none").shape == (4,)
