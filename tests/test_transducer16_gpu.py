"""The transducer score and its pruned form over bfloat16 / float16 logits on the GPU (gtn_amd/csrc/transducer16.hip,
DESIGN section 45) against the float64 yardsticks of tests/transducer_fp.py and tests/transducer_pruned_fp.py.  The seeded
logits are rounded to the dtype with torch and the yardstick runs on those rounded values, so the input rounding is no
error source.  Gates: score 1e-4 max(1, |want|), exactly -inf where wanted (float32 arithmetic on exact inputs: the
float32 entries' gate); gradient 1e-4 + u |want| + 2^-24 with u = 2^-8 (bfloat16) or 2^-11 (float16): the float32 gate plus
one rounding of the output, the last term for float16's subnormals; never-read rows, dead rows and the rows of an
utterance that scores -inf are +0 bits.  Every output carries a guard row of sentinels; the inputs are only read."""
import numpy as np
import pytest

import transducer_fp as fp
import transducer_pruned_fp as pfp

pytestmark = pytest.mark.gpu
SENTINEL = 12288.0  # (exact in both dtypes)
CAP = "GTNX_TRANSDUCER_SCRATCH_BYTES"
UNIT = {"bfloat16": 2.0 ** -8, "float16": 2.0 ** -11}
dtypes = pytest.mark.parametrize("dtype", list(UNIT))


def _round(x, dtype):
    import torch
    return torch.from_numpy(np.array(x, copy=True)).to(getattr(torch, dtype))


def _run(gtn, xt, index, blank, w, normalize=True, keep_rows=False, offset=0):
    """the 16-bit CPU tensor xt [B, T, W, C] through gtn.transducer_score / _score_grad (index: targets, frames, tlens) or
    the pruned pair (index: ranges, targets, frames, tlens) -> (scores [B] numpy, grad [B, T, W, C] CPU tensor of xt's
    dtype).  `offset`: logits and gradient start that many elements into their buffers."""
    import torch
    B, T, W, C = xt.shape
    pruned = len(index) == 4
    score, grad, stats = ((gtn.transducer_pruned_score, gtn.transducer_pruned_score_grad, gtn.debug_transducer_pruned_stats)
                          if pruned else (gtn.transducer_score, gtn.transducer_score_grad, gtn.debug_transducer_stats))
    xd = torch.empty(xt.numel() + offset, dtype=xt.dtype, device="cuda:0")[offset:].view(xt.shape).copy_(xt)
    args = tuple(torch.from_numpy(np.array(a, copy=True)).to("cuda:0") for a in index)
    sc = torch.full((B + 1,), SENTINEL, device="cuda:0")
    g = torch.full(((B + 1) * T * W * C + offset,), SENTINEL, dtype=xt.dtype, device="cuda:0")[offset:].view(B + 1, T, W, C)
    rows = torch.full((B + 1, T, W, 3), SENTINEL, device="cuda:0") if keep_rows else None
    torch.cuda.synchronize()
    c0 = stats()
    score(xd, *args, sc[:B], None if rows is None else rows[:B], blank, normalize)
    grad(xd, *args, torch.from_numpy(np.array(w)).to("cuda:0"), g[:B], None if rows is None else rows[:B], blank, normalize)
    gtn.synchronize()
    c1 = stats()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (2, 2 * B)
    assert torch.equal(xd.cpu().view(torch.int16), xt.view(torch.int16))  # only read
    for guarded in (sc, g, rows):
        assert guarded is None or (guarded[-1] == SENTINEL).all(), "guard row"
    return sc[:B].cpu().numpy(), g[:B].cpu()


def _want(xt, index, blank, normalize, w):
    ref = pfp.reference if len(index) == 4 else fp.reference
    return ref(xt.double().numpy(), *index, blank, normalize, w)


def _zero_rows(xt, index, want_scores):
    """bool [B, T, W]: rows that are never read (every row of an utterance whose counts do not fit) or belong to an
    utterance that scores -inf"""
    frames, tlens = np.asarray(index[-2]), np.asarray(index[-1])
    if len(index) == 4:
        never = pfp.never_read(index[0], frames, tlens, xt.shape[2])
    else:
        never = ((np.arange(xt.shape[1])[None, :, None] >= frames[:, None, None])
                 | (np.arange(xt.shape[2])[None, None, :] > tlens[:, None, None]))
    never = never | (tlens >= index[-3].shape[1] + 1)[:, None, None]
    return never, never | np.isneginf(want_scores)[:, None, None]


def _check(name, got, want_scores, want_grad, zero):
    import torch
    scores, g = got
    grad = g.double().numpy()
    assert not np.isnan(scores).any() and not np.isnan(grad).any(), name
    for b, (have, want) in enumerate(zip(scores, want_scores)):
        print(f"{name} b={b} score {have!r} want {want!r}")
        assert have == want if np.isinf(want) else abs(have - want) <= 1e-4 * max(1.0, abs(want)), (name, b, have, want)
    over = np.abs(grad - want_grad) - (1e-4 + UNIT[str(g.dtype)[6:]] * np.abs(want_grad) + 2.0 ** -24)
    print(f"{name} worst gradient error {np.abs(grad - want_grad).max():.3g}, closest to its bound {over.max():.3g}")
    assert (over <= 0).all(), name
    assert not g.view(torch.int16)[torch.from_numpy(zero)].any(), name  # (+0 bits)


def _same_bits(a, b):
    import torch
    return (a[0].view(np.int32) == b[0].view(np.int32)).all() and torch.equal(a[1].view(torch.int16), b[1].view(torch.int16))


# ---- 1. the full lattice against float64 ----
# (T, U, C): the degenerate rows and 7 / 8 / 9 labels; both sides of every edge of the rows16 table (32, 128, 512, 1024,
# 2048 labels; the gradient's edges are 32 and 128) and of the register / online boundary at 4096, 257 and 4101 for the
# 2-byte path between and above them; two shapes whose sweeps use more than one column per lane
ROWS = [(1, 0, 1), (2, 1, 3), (3, 2, 7), (3, 2, 8), (3, 2, 9), (3, 2, 32), (3, 2, 40), (3, 2, 128), (3, 2, 136),
        (3, 2, 257), (3, 2, 512), (3, 2, 520), (3, 2, 1024), (3, 2, 1032), (3, 2, 2048), (3, 2, 2056), (3, 2, 4096),
        (3, 2, 4104), (3, 2, 4101), (65, 63, 5), (70, 129, 8)]
FULL = [s + (True, True, 0) for s in ROWS] + [(5, 4, 4, False, False, 0), (3, 2, 136, True, False, 0),
                                              (3, 2, 128, True, True, 1)]  # (the last: a base 2 bytes past alignment)


@dtypes
@pytest.mark.parametrize("T,U,C,peaked,normalize,offset", FULL, ids=str)
def test_full_lattice_against_float64(gtn, dtype, T, U, C, peaked, normalize, offset):
    x, targets, frames, tlens, blank, w = fp.case(T, U, C, peaked, normalize)[:6]
    xt, index = _round(x, dtype), (targets, frames, tlens)
    want = _want(xt, index, blank, normalize, w)
    assert np.isfinite(want[0]).any(), "a case without a live utterance shows nothing"
    _check(f"{T, U, C}", _run(gtn, xt, index, blank, w, normalize, offset=offset), *want, _zero_rows(xt, index, want[0])[1])


# ---- 2. the band against float64 ----
@dtypes
@pytest.mark.parametrize("shape", [(24, 12, 5, 6, "mixed"), (7, 4, 5, 6, "zero"), (10, 6, 2, 40, "mixed"),
                                   (3, 2, 2, 4100, "mixed")], ids=str)
def test_pruned_against_float64(gtn, dtype, shape):
    x, ranges, targets, frames, tlens, blank, w = pfp.case(*shape, True)[:7]
    xt, index = _round(x, dtype), (ranges, targets, frames, tlens)
    want = _want(xt, index, blank, True, w)
    assert np.isfinite(want[0]).any(), "a case without a live utterance shows nothing"
    _check(str(shape), _run(gtn, xt, index, blank, w), *want, _zero_rows(xt, index, want[0])[1])


# ---- 3. -inf, never NaN, dead rows, never-read rows; the neighbours keep their bits ----
@dtypes
@pytest.mark.parametrize("entry", ["full", "pruned"])
@pytest.mark.parametrize("name", ["T_b == 0", "U_b > U", "blank token"])
def test_minus_inf_dead_rows_and_never_read_rows(gtn, dtype, entry, name):
    if entry == "full":
        x, targets, frames, tlens, blank, w = (np.array(a) for a in fp.case(6, 4, 8, True, True)[:6])
        index = [targets[[0, 0, 0]], frames[[0, 0, 0]], tlens[[0, 0, 0]]]
        index[1][1], index[2][1] = 5, 3  # (utterance 1 leaves frame 5 and column 4 unread)
    else:
        x, ranges, targets, frames, tlens, blank, w = (np.array(a) for a in pfp.case(24, 12, 5, 6, "mixed", True)[:7])
        assert list(ranges[0, :8]) == [0, 0, 1, 5, 9, 9, 10, 10]  # (paths pass band row (2, 1) by on either side)
        index = [ranges[[0, 0, 0]], targets[[0, 0, 0]], frames[[0, 0, 0]], tlens[[0, 0, 0]]]
    x, w = x[[0, 0, 0]], w[[0, 1, 3]]
    x[0, 2, 1, :] = -np.inf  # a dead row with paths around it
    x[1, 2, 1, 0] = np.nan
    dead = [(0, 2, 1), (1, 2, 1)]
    if dtype == "float16":  # (its own inf encoding)
        x[1, 1, 0, 1] = np.inf
        dead.append((1, 1, 0))
    if name == "T_b == 0":
        index[-2][2] = 0
    elif name == "U_b > U":
        index[-1][2] = index[-3].shape[1] + 1
    else:
        index[-3][2, 0] = blank
    xt = _round(x, dtype)
    want = _want(xt, index, blank, True, w)
    never, zero = _zero_rows(xt, index, want[0])
    for d in dead:
        zero[d] = True
    got = _run(gtn, xt, index, blank, w)
    assert np.isfinite(got[0][:2]).all() and np.isneginf(got[0][2]) and got[1][0].any()
    _check(name, got, *want, zero)
    alone = _run(gtn, xt[:2], [a[:2] for a in index], blank, w[:2])
    assert _same_bits((got[0][:2], got[1][:2]), alone)  # (the neighbours are unaffected)
    assert never[:2].any() and never[2].all() == (name != "blank token")
    x[never] = np.nan
    assert _same_bits(got, _run(gtn, _round(x, dtype), index, blank, w))  # (never-read rows are never read)


# ---- 4. the same bits: run to run, sliced, alone, with or without the rows plane ----
@dtypes
@pytest.mark.parametrize("entry", ["full", "pruned"])
def test_runs_slices_neighbours_and_rows_change_no_bit(gtn, dtype, entry, monkeypatch):
    case = fp.case(5, 4, 40, True, True)[:6] if entry == "full" else pfp.case(24, 12, 5, 6, "mixed", True)[:7]
    xt, index, blank, w = _round(case[0], dtype), case[1:-2], case[-2], case[-1]
    whole = _run(gtn, xt, index, blank, w)
    assert _same_bits(whole, _run(gtn, xt, index, blank, w))
    assert _same_bits(whole, _run(gtn, xt, index, blank, w, keep_rows=True))
    monkeypatch.setenv(CAP, "1")  # (one utterance per slice)
    assert _same_bits(whole, _run(gtn, xt, index, blank, w))
    assert _same_bits(whole, _run(gtn, xt, index, blank, w, keep_rows=True))
    monkeypatch.delenv(CAP)
    for b in range(len(w)):
        one = _run(gtn, xt[b:b + 1], [a[b:b + 1] for a in index], blank, w[b:b + 1])
        assert _same_bits((whole[0][b:b + 1], whole[1][b:b + 1]), one), b


# ---- 5. the torch entries ----
@dtypes
@pytest.mark.parametrize("entry", ["full", "pruned"])
def test_torch_score_loss_and_occupancy(gtn, dtype, entry):
    import torch
    import gtn_amd.torch_loss as tl
    case = fp.case(5, 4, 40, True, True)[:6] if entry == "full" else pfp.case(24, 12, 5, 6, "mixed", True)[:7]
    xt, index, blank, w = _round(case[0], dtype), case[1:-2], case[-2], case[-1]
    score, loss = (tl.transducer_score, tl.transducer_loss) if entry == "full" else (tl.transducer_pruned_score,
                                                                                   tl.transducer_pruned_loss)
    dev = [torch.from_numpy(np.array(a)).to("cuda:0") for a in index]
    xd = xt.to("cuda:0").requires_grad_(True)
    out = score(xd, *(a.long() for a in dev), blank, True)
    out.backward(torch.from_numpy(np.array(w)).to("cuda:0"))
    assert out.dtype == torch.float32 and xd.grad.dtype == xt.dtype
    want = _want(xt, index, blank, True, w)
    _check("torch", (out.detach().cpu().numpy(), xd.grad.cpu()), *want, _zero_rows(xt, index, want[0])[1])
    live = np.flatnonzero(np.isfinite(want[0]))
    xl = xt[live].to("cuda:0").requires_grad_(True)
    mean = loss(xl, *(a[live] for a in dev), blank, True, reduction="mean")
    mean.backward()
    assert mean.dtype == torch.float32 and xl.grad.dtype == xt.dtype
    assert abs(mean.item() + want[0][live].mean()) <= 1e-4 * max(1.0, abs(want[0][live].mean()))
    if entry == "full":  # (the rows plane of a 16-bit score call is the plane transducer_occupancy reads)
        sc, rows = torch.empty(len(w), device="cuda:0"), torch.empty(*xt.shape[:3], 3, device="cuda:0")
        gtn.transducer_score(xd.detach(), *dev, sc, rows, blank, True)
        occ = tl.transducer_occupancy(rows, dev[1], dev[2]).cpu().numpy()
        assert np.abs(occ - pfp.occupancy(rows.cpu().numpy(), index[1], index[2])).max() <= 1e-4
