"""The pruned (banded) transducer score on the GPU (gtn_amd/csrc/transducer_pruned.hip) against the
float64 yardstick of tests/transducer_pruned_fp.py at the project's gates (score 1e-4 max(1, |want|), gradient 1e-4
absolute, never-read rows == 0), the contract's promises about -inf and about bits, and the torch entries, with
transducer_occupancy and transducer_prune_ranges that connect the first pass to this one.  Every output carries a guard
row of sentinels; the inputs are only read."""
import numpy as np
import pytest

import transducer_pruned_fp as fp

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0
CAP = "GTNX_TRANSDUCER_SCRATCH_BYTES"


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True)).to("cuda:0")  # (the cached cases are read-only)


def _run(gtn, x, ranges, targets, frames, tlens, blank, w, normalize=True, keep_rows=False):
    """gtn.transducer_pruned_score and _score_grad -> (scores [B], grad [B, T, S, C]) as numpy"""
    import torch
    B, T, S, C = x.shape
    xd, args = _dev(x), (_dev(ranges), _dev(targets), _dev(frames), _dev(tlens))
    sc = torch.full((B + 1,), SENTINEL, device="cuda:0")
    g = torch.full((B + 1, T, S, C), SENTINEL, device="cuda:0")
    rows = torch.full((B + 1, T, S, 3), SENTINEL, device="cuda:0") if keep_rows else None
    torch.cuda.synchronize()
    c0 = gtn.debug_transducer_pruned_stats()
    gtn.transducer_pruned_score(xd, *args, sc[:B], None if rows is None else rows[:B], blank, normalize)
    gtn.transducer_pruned_score_grad(xd, *args, _dev(w), g[:B], None if rows is None else rows[:B], blank, normalize)
    gtn.synchronize()
    c1 = gtn.debug_transducer_pruned_stats()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (2, 2 * B)
    assert (xd.cpu().numpy().view(np.int32) == np.asarray(x).view(np.int32)).all()  # only read
    assert (args[0].cpu().numpy() == ranges).all()
    for guarded in (sc, g, rows):
        assert guarded is None or (guarded[-1] == SENTINEL).all(), "guard row"
    return sc[:B].cpu().numpy(), g[:B].cpu().numpy()


def _same_bits(a, b):
    return all((x.view(np.int32) == y.view(np.int32)).all() for x, y in zip(a, b))


# ---- 1. against float64 ----
@pytest.mark.parametrize("normalize", [True, False], ids=["normalised", "as-is"])
@pytest.mark.parametrize("shape", fp.CASES, ids=str)
def test_scores_and_gradients_against_float64(gtn, shape, normalize):
    x, ranges, targets, frames, tlens, blank, w, *want = fp.case(*shape, normalize)
    got = _run(gtn, x, ranges, targets, frames, tlens, blank, w, normalize)
    assert np.isfinite(want[0]).any(), "a case without a live utterance shows nothing"
    fp.check(str(shape), *got, *want, ranges, frames, tlens)


# ---- 2. S = U + 1 under zero ranges is the full lattice ----
@pytest.mark.parametrize("normalize", [True, False], ids=["normalised", "as-is"])
def test_agrees_with_the_full_lattice_entry(gtn, normalize):
    import torch
    x, ranges, targets, frames, tlens, blank, w = fp.case(7, 4, 5, 6, "zero", normalize)[:7]
    got = _run(gtn, x, ranges, targets, frames, tlens, blank, w, normalize)
    xd, args = _dev(x), (_dev(targets), _dev(frames), _dev(tlens))
    sc, g = torch.empty(len(w), device="cuda:0"), torch.empty(x.shape, device="cuda:0")
    gtn.transducer_score(xd, *args, sc, None, blank, normalize)
    gtn.transducer_score_grad(xd, *args, _dev(w), g, None, blank, normalize)
    gtn.synchronize()
    fp.check("full", *got, sc.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64), ranges, frames, tlens)


# ---- 3. -inf, never NaN, and the neighbours keep their bits ----
def _invalid(name, ranges, frames, tlens, targets, blank, S):
    """make utterance 2 of a batch of three invalid in the named way"""
    r = ranges[2]
    if name == "step of S":
        r[3:] += S - (r[3] - r[2])
    elif name == "decreasing":
        r[6] = r[5] - 1  # (9, 8, 10: the bands still share columns, only the rule makes this -inf)
    elif name == "no (0, 0)":
        r[:3] = 1
    elif name == "no (T_b - 1, U_b)":
        tlens[2] = r[frames[2] - 1] - 1
    elif name == "negative":
        r[1] = -1
    elif name == "above U":
        r[frames[2] - 1] = targets.shape[1] + 1
    elif name == "T_b == 0":
        frames[2] = 0
    elif name == "blank token":
        targets[2, 0] = blank


@pytest.mark.parametrize("name", ["step of S", "decreasing", "no (0, 0)", "no (T_b - 1, U_b)", "negative", "above U",
                                  "T_b == 0", "blank token"])
def test_minus_inf_dead_rows_and_invalid_utterances(gtn, name):
    T, U, S, C = 24, 12, 5, 6
    x, ranges, targets, frames, tlens, blank, w = (np.array(a) for a in fp.case(T, U, S, C, "mixed", True)[:7])
    assert list(ranges[0, :8]) == [0, 0, 1, 5, 9, 9, 10, 10]  # (what the edits below rely on)
    x, ranges, targets, w = x[[0, 0, 0]], ranges[[0, 0, 0]], targets[[0, 0, 0]], w[[0, 1, 3]]
    frames, tlens = frames[[0, 0, 0]], tlens[[0, 0, 0]]
    x[0, 2, 1, :] = -np.inf                       # dead rows inside the band with paths around them
    x[1, 2, 1, 0] = np.nan
    x[0, 5, 0, blank] = -np.inf                   # a -inf entry: paths remain
    _invalid(name, ranges, frames, tlens, targets, blank, S)
    got = _run(gtn, x, ranges, targets, frames, tlens, blank, w)
    assert np.isfinite(got[0][:2]).all() and np.isneginf(got[0][2]) and not got[1][2].any()
    assert got[1][0].any() and not got[1][0, 2, 1].any() and not got[1][1, 2, 1].any()
    fp.check(name, *got, *fp.reference(x, ranges, targets, frames, tlens, blank, True, w), ranges, frames, tlens)
    alone = _run(gtn, x[:2], ranges[:2], targets[:2], frames[:2], tlens[:2], blank, w[:2])
    assert _same_bits((got[0][:2], got[1][:2]), alone)  # (the neighbours are unaffected)


# ---- 4. never-read rows are never read ----
@pytest.mark.parametrize("normalize", [True, False], ids=["normalised", "as-is"])
def test_nan_in_the_never_read_rows_changes_no_bit(gtn, normalize):
    x, ranges, targets, frames, tlens, blank, w = fp.case(24, 12, 5, 6, "mixed", normalize)[:7]
    x_nan = x.copy()
    mask = fp.never_read(ranges, frames, tlens, 5)
    assert mask[:, :, 1:][(np.arange(24)[None, :] < frames[:, None])].any()  # (band rows above U_b at a live frame)
    x_nan[mask] = np.nan
    assert _same_bits(_run(gtn, x_nan, ranges, targets, frames, tlens, blank, w, normalize),
                      _run(gtn, x, ranges, targets, frames, tlens, blank, w, normalize))


# ---- 5. the same bits: run to run, sliced, alone, with or without the rows plane ----
@pytest.mark.parametrize("shape", [(24, 12, 5, 6, "mixed"), (3, 2, 2, 4100, "mixed")], ids=str)
def test_runs_slices_neighbours_and_rows_change_no_bit(gtn, shape, monkeypatch):
    x, ranges, targets, frames, tlens, blank, w = fp.case(*shape, True)[:7]
    whole = _run(gtn, x, ranges, targets, frames, tlens, blank, w)
    assert _same_bits(whole, _run(gtn, x, ranges, targets, frames, tlens, blank, w))
    assert _same_bits(whole, _run(gtn, x, ranges, targets, frames, tlens, blank, w, keep_rows=True))
    monkeypatch.setenv(CAP, "1")  # (one utterance per slice)
    assert _same_bits(whole, _run(gtn, x, ranges, targets, frames, tlens, blank, w))
    assert _same_bits(whole, _run(gtn, x, ranges, targets, frames, tlens, blank, w, keep_rows=True))
    monkeypatch.delenv(CAP)
    for b in range(len(frames)):
        one = _run(gtn, *(a[b:b + 1] for a in (x, ranges, targets, frames, tlens)), blank, w[b:b + 1])
        assert _same_bits((whole[0][b:b + 1], whole[1][b:b + 1]), one), b


# ---- 6. the torch entries ----
@pytest.mark.parametrize("normalize", [True, False], ids=["normalised", "as-is"])
def test_torch_score_and_loss(gtn, normalize):
    import gtn_amd.torch_loss as tl
    x, ranges, targets, frames, tlens, blank, w, want_scores, want_grad = fp.case(24, 12, 5, 6, "mixed", normalize)
    xd = _dev(x).requires_grad_(True)
    args = (_dev(ranges).long(), _dev(targets).long(), _dev(frames).long(), _dev(tlens), blank, normalize)
    out = tl.transducer_pruned_score(xd, *args)
    out.backward(_dev(w))
    fp.check("torch", out.detach().cpu().numpy(), xd.grad.cpu().numpy(), want_scores, want_grad, ranges, frames, tlens)
    live = np.flatnonzero(np.isfinite(want_scores))
    assert len(live) >= 3
    for reduction, scale in (("none", None), ("sum", 1.0), ("mean", 1.0 / len(live))):
        xl = _dev(x[live]).requires_grad_(True)
        loss = tl.transducer_pruned_loss(xl, *(a[live] for a in args[:4]), blank, normalize, reduction=reduction)
        if scale is None:
            assert np.abs(loss.detach().cpu().numpy() + want_scores[live]).max() <= 1e-4 * np.abs(want_scores[live]).max()
            continue
        loss.backward()
        want = -scale * want_scores[live].sum()
        unit = fp.reference(x[live], ranges[live], targets[live], frames[live], tlens[live], blank, normalize,
                            np.full(len(live), -scale))
        assert abs(loss.item() - want) <= 1e-4 * max(1.0, abs(want))
        assert np.abs(xl.grad.cpu().numpy() - unit[1]).max() <= 1e-4


def test_occupancy_prune_ranges_and_the_pruned_loss_end_to_end(gtn):
    import torch
    import gtn_amd.torch_loss as tl
    T, U, C, S, B = 12, 9, 8, 4, 4
    rng = np.random.default_rng(44)
    am, lm = rng.standard_normal((B, T, C)).astype(np.float32), rng.standard_normal((B, U + 1, C)).astype(np.float32)
    targets = rng.integers(1, C, (B, U)).astype(np.int32)
    frames, tlens = np.asarray([T, 7, 1, 0], np.int32), np.asarray([U, 4, 0, 3], np.int32)
    dev = [_dev(a) for a in (am, lm, targets, frames, tlens)]
    sc = torch.empty(B, device="cuda:0")
    rows = torch.full((B + 1, T, U + 1, 3), SENTINEL, device="cuda:0")
    gtn.transducer_add_score(*dev, sc, rows[:B], 0)
    occ = tl.transducer_occupancy(rows[:B], dev[3].long(), dev[4])
    gtn.synchronize()
    assert (rows[-1] == SENTINEL).all()
    want = fp.occupancy(rows[:B].cpu().numpy(), frames, tlens)
    print("worst occupancy error", np.abs(occ.cpu().numpy() - want).max())
    assert np.abs(occ.cpu().numpy() - want).max() <= 1e-4 and not occ[3].any() and not occ[1, 7:].any()
    ranges = tl.transducer_prune_ranges(occ, dev[3], dev[4], S)
    joint = dev[0][:, :, None, :] + dev[1][:, None, :, :]                      # the joiner of this test: the plain sum
    idx = (ranges[:, :, None].long() + torch.arange(S, device="cuda:0")).clamp(max=U)
    band = torch.gather(joint, 2, idx[:, :, :, None].expand(-1, -1, -1, C)).contiguous()
    pruned = tl.transducer_pruned_loss(band, ranges, dev[2], dev[3], dev[4], 0, True, reduction="none").cpu().numpy()
    full = tl.transducer_loss(joint.contiguous(), dev[2], dev[3], dev[4], 0, True, reduction="none").cpu().numpy()
    print("pruned", pruned, "full", full)
    assert np.isfinite(pruned[:3]).all() and np.isposinf(pruned[3])
    # (the band holds a subset of the paths: its score is at most the full score, its loss at least the full loss; the
    # gate allows for float32 on either side)
    assert (full[:3] <= pruned[:3] + 1e-4 * np.maximum(1.0, np.abs(full[:3]))).all()
