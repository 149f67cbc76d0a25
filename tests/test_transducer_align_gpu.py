"""The batched transducer forced alignment on the GPU (gtn_amd/csrc/transducer_align.hip): every
output against tests/transducer_align_fp.py -- bit for bit against `transcribe` of the compact plane the kernel read,
and at the project's gate, 1e-4 max(1, |want|), against float64 from the logits -- and the contract's promises about
bits.  Every output carries a guard row of sentinels."""
import math

import numpy as np
import pytest

import transducer_align_fp as afp
import transducer_fp as fp

pytestmark = pytest.mark.gpu
SENTINEL = 12345
CAP = "GTNX_TRANSDUCER_SCRATCH_BYTES"


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True)).to("cuda:0")  # (the cached cases are read-only)


def _align(gtn, B, T, U, call):
    """call(scores, token_frames, token_scores, frame_tokens) on guarded outputs -> the four as numpy"""
    import torch
    outs = [torch.full((B + 1,) + s, SENTINEL, dtype=d, device="cuda:0")
            for s, d in (((), torch.float32), ((U,), torch.int32), ((U,), torch.float32), ((T,), torch.int32))]
    torch.cuda.synchronize()
    c0 = gtn.debug_transducer_align_stats()
    call(*(o[:B] for o in outs))
    gtn.synchronize()
    c1 = gtn.debug_transducer_align_stats()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, B)
    assert all((o[-1] == SENTINEL).all() for o in outs), "guard row"
    got = tuple(o[:B].cpu().numpy() for o in outs)
    assert not np.isnan(got[0]).any() and not np.isnan(got[2]).any()
    return got


def _from_logits(gtn, x, targets, frames, tlens, blank, normalize, rows=None):
    B, T, U1, _ = x.shape
    xd, args = x if hasattr(x, "data_ptr") else _dev(x), (_dev(targets), _dev(frames), _dev(tlens))
    return _align(gtn, B, T, U1 - 1, lambda *o: gtn.transducer_align(xd, *args, *o, rows, blank, normalize))


def _from_rows(gtn, rows, frames, tlens):
    B, T, U1, _ = rows.shape
    return _align(gtn, B, T, U1 - 1, lambda *o: gtn.transducer_align_rows(rows, _dev(frames), _dev(tlens), *o))


def _same_bits(a, b):
    return all((np.array(x).view(np.int32) == np.array(y).view(np.int32)).all() for x, y in zip(a, b))


def _gathered(x, targets, blank):
    """the compact plane of as-is logits: the node's own two entries"""
    B, T, U1, _ = x.shape
    rows = np.zeros((B, T, U1, 3), np.float32)
    rows[..., 0] = x[..., blank]
    rows[:, :, U1 - 1, 1] = -np.inf
    for u in range(U1 - 1):
        rows[:, :, u, 1] = x[np.arange(B), :, u, targets[:, u]]
    return rows


# ---- 1. bits, as-is logits: every K, the lane edges, skew fill and drain, the degenerate lattices ----
@pytest.mark.parametrize("shape", [(65, 63, 5), (64, 64, 5), (63, 128, 5), (70, 129, 8), (3, 255, 2), (3, 300, 2),
                                   (3, 512, 2), (3, 1023, 2), (129, 1, 4), (1, 0, 1), (1, 5, 4), (5, 4, 4)], ids=str)
def test_as_is_logits_bit_for_bit(gtn, shape):
    x, targets, frames, tlens, blank = fp.case(*shape, True, False)[:5]
    got = _from_logits(gtn, x, targets, frames, tlens, blank, False)
    assert _same_bits(got, afp.transcribe(_gathered(x, targets, blank), frames, tlens))


# above 960 rows (480 with K == 16) the bits live in scratch and the walk reads them through a window that long
@pytest.mark.parametrize("T,U", [(1000, 3), (500, 600)], ids=str)
def test_plane_in_scratch_and_a_walk_across_the_window(gtn, T, U):
    rng = np.random.default_rng(T + U)
    rows = -np.abs(rng.standard_normal((2, T, U + 1, 3))).astype(np.float32)
    frames, tlens = np.asarray([T, T - 7], np.int32), np.asarray([U, U // 2], np.int32)
    assert _same_bits(_from_rows(gtn, _dev(rows), frames, tlens), afp.transcribe(rows, frames, tlens))


# ---- 2. ties: multiples of 0.25 make every float32 sum exact, so float64 with the tie rule gives the same bits ----
@pytest.mark.parametrize("shape", [(40, 37, 3), (9, 130, 3)], ids=str)
def test_ties_go_to_the_blank_arc(gtn, shape):
    T, U, C = shape
    rng = np.random.default_rng(200 + T)  # (a seed whose four best paths all pass through a tie: asserted below)
    x = (-0.25 * rng.integers(0, 17, (2, T, U + 1, C))).astype(np.float32)
    targets = rng.integers(1, C, (2, U)).astype(np.int32)
    frames, tlens = np.asarray([T, T - 2], np.int32), np.asarray([U, U - 3], np.int32)
    planes = afp.planes64(x, targets, frames, tlens, 0, False)
    assert all(afp._best(*p)[3] > 0 for p in planes)  # (ties on the best path itself: the rule decides)
    want = afp.reference(x, targets, frames, tlens, 0, False)
    got = _from_logits(gtn, x, targets, frames, tlens, 0, False)
    assert all((g == w).all() for g, w in zip(got, want))


# ---- 3. normalised logits and the three producers of the plane ----
def _add_case(T, U, C):
    B, blank = 4, C // 2
    rng = np.random.default_rng(1000 * T + 10 * U + C)
    am, lm = rng.standard_normal((B, T, C)), rng.standard_normal((B, U + 1, C))
    targets = ((blank + 1 + rng.integers(0, C - 1, (B, U))) % C).astype(np.int32)
    am[:, :, blank] += 3 + math.log(C)
    for u in range(U):
        lm[np.arange(B), u, targets[:, u]] += 3 + math.log(C)
    return am.astype(np.float32), lm.astype(np.float32), targets, blank


@pytest.mark.parametrize("producer", ["float32", "bfloat16", "additive"])
@pytest.mark.parametrize("shape", [(65, 63, 5), (70, 129, 8)], ids=str)
def test_normalised_logits_and_the_three_producers(gtn, shape, producer):
    import torch
    x, targets, frames, tlens, blank = fp.case(*shape, True, True)[:5]
    B, (T, U, _) = len(frames), shape
    rows = torch.full((B + 1, T, U + 1, 3), float(SENTINEL), device="cuda:0")
    sc, args = torch.empty(B, device="cuda:0"), (_dev(targets), _dev(frames), _dev(tlens))
    if producer == "additive":
        am, lm, targets, blank = _add_case(*shape)
        args = (_dev(targets),) + args[1:]
        gtn.transducer_add_score(_dev(am), _dev(lm), *args, sc, rows[:B], blank)
        x64, xd = am.astype(np.float64)[:, :, None] + lm.astype(np.float64)[:, None], None
    else:
        xd = _dev(x).to(getattr(torch, producer))
        gtn.transducer_score(xd, *args, sc, rows[:B], blank, True)
        x64 = xd.double().cpu().numpy()  # (the exactly converted values)
    gtn.synchronize()
    want = afp.transcribe(rows[:B].cpu().numpy(), frames, tlens)
    got = _from_rows(gtn, rows[:B], frames, tlens)
    assert _same_bits(got, want) and (rows[-1] == SENTINEL).all()
    if xd is not None:
        assert _same_bits(got, _from_logits(gtn, xd, targets, frames, tlens, blank, True))
        assert _same_bits(got, _from_logits(gtn, xd, targets, frames, tlens, blank, True, rows[:B]))
    best = afp.reference(x64, targets, frames, tlens, blank, True)[0]
    planes = afp.planes64(x64, targets, frames, tlens, blank, True)
    for b in range(B):
        if np.isinf(best[b]):
            assert got[0][b] == best[b]
            continue
        gate = 1e-4 * max(1.0, abs(best[b]))
        mine = afp.path_score(planes[b], got[1][b])  # (a float32 near-tie may pick another path, not a worse one)
        print(f"{shape} {producer} b={b} score {got[0][b]!r} path {mine!r} want {best[b]!r}")
        assert abs(got[0][b] - best[b]) <= gate and abs(mine - best[b]) <= gate


# ---- 4. -inf, never-read rows, slicing (the inputs of test_transducer_gpu's -inf test) ----
def test_minus_inf_never_read_rows_and_slices(gtn, monkeypatch):
    import torch
    x, targets, frames, tlens, blank, _ = (np.array(a) for a in fp.case(5, 4, 4, True, True)[:6])
    x, targets = np.concatenate([x, x[:3]]), np.concatenate([targets, targets[:3]])
    frames = np.asarray([5, 5, 5, 0, 5, 5, 6], np.int32)  # (3: T_b == 0; 6: T_b > T)
    tlens = np.asarray([4, 4, 2, 3, 4, 4, 4], np.int32)
    x[0, 1, 2, :2] = -np.inf                       # -inf entries: paths remain
    x[0, 2, 1, blank] = -np.inf
    x[1, 2, 1, 0], x[1, 3, 0, :] = np.nan, -np.inf  # dead rows: paths remain around them
    x[2, :, 1, 3] = np.inf                         # a dead column: no path
    targets[4, 2] = 4                              # a token outside 0 .. C - 1
    targets[5, 0] = blank                          # a token equal to blank
    got = _from_logits(gtn, x, targets, frames, tlens, blank, True)
    assert np.isneginf(got[0][2:]).all() and np.isneginf(got[2][2:]).all()
    assert (got[1][2:] == -1).all() and (got[3][2:] == -1).all() and np.isfinite(got[0][:2]).all()
    rows, sc = torch.zeros(2, 5, 5, 3, device="cuda:0"), torch.empty(2, device="cuda:0")
    gtn.transducer_score(_dev(x[:2]), _dev(targets[:2]), _dev(frames[:2]), _dev(tlens[:2]), sc, rows, blank, True)
    gtn.synchronize()
    assert _same_bits([g[:2] for g in got], afp.transcribe(rows.cpu().numpy(), frames[:2], tlens[:2]))
    x_nan = x.copy()
    for b in range(len(frames)):
        x_nan[b, min(frames[b], 5):] = np.nan
        x_nan[b, :, tlens[b] + 1:] = np.nan
    assert _same_bits(got, _from_logits(gtn, x_nan, targets, frames, tlens, blank, True))
    monkeypatch.setenv(CAP, "1")  # (one utterance per slice)
    assert _same_bits(got, _from_logits(gtn, x, targets, frames, tlens, blank, True))
    monkeypatch.delenv(CAP)
    for b in range(2):
        one = _from_logits(gtn, x[b:b + 1], targets[b:b + 1], frames[b:b + 1], tlens[b:b + 1], blank, True)
        assert _same_bits([g[b:b + 1] for g in got], one), b


# ---- 5. the torch entry ----
def test_torch_entry(gtn):
    import torch
    import gtn_amd.torch_loss as tl
    x, targets, frames, tlens, blank = fp.case(65, 63, 5, True, True)[:5]
    args = (_dev(targets).long(), _dev(frames).long(), _dev(tlens))
    scores, token_frames, token_scores, frame_tokens = tl.transducer_align(
        _dev(x), *args, blank, return_token_scores=True, return_frame_tokens=True)
    assert [(t.dtype, tuple(t.shape)) for t in (scores, token_frames, token_scores, frame_tokens)] == [
        (torch.float32, (4,)), (torch.int32, (4, 63)), (torch.float32, (4, 63)), (torch.int32, (4, 65))]
    want = afp.reference(x, targets, frames, tlens, blank, True)
    tf, ft = token_frames.cpu().numpy(), frame_tokens.cpu().numpy()
    for b in range(4):
        Tb, Ub = int(frames[b]), int(tlens[b])
        if np.isinf(want[0][b]):
            assert np.isneginf(scores[b].item()) and (tf[b] == -1).all() and (ft[b] == -1).all()
            continue
        assert abs(scores[b].item() - want[0][b]) <= 1e-4 * max(1.0, abs(want[0][b]))
        assert (ft[b, :Tb] == [(tf[b, :Ub] <= t).sum() for t in range(Tb)]).all() and (ft[b, Tb:] == -1).all()
    sc = torch.empty(4, device="cuda:0")
    rows = torch.empty(4, 65, 64, 3, device="cuda:0")
    gtn.transducer_score(_dev(x), _dev(targets), _dev(frames), _dev(tlens), sc, rows, blank, True)
    again = tl.transducer_align_rows(rows, *args[1:], return_frame_tokens=True)
    assert torch.equal(again[0], scores) and torch.equal(again[1], token_frames) and torch.equal(again[2], frame_tokens)
