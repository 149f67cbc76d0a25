"""The batched ASG full-connect score for up to 1024 labels on the GPU (gtn_amd/csrc/asg_full_wide.hip, DESIGN section
41): scores and both gradients against tests/ctc_fp64.py's asg_fp64 on em[b, :T_b] at the project's gates (scores 1e-4
max(1, |want|), emission gradients 1e-4 absolute with pad rows == 0, table gradient rtol 1e-3 / atol 1e-4), and the
contract's promises about bits: pad rows are never read, the same bits run to run, sliced or not, whatever the group
and whatever the neighbours.  Every output carries a guard row of sentinels."""
import numpy as np
import pytest

import asg_full_score_fp as fp

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0
CAP, GROUP = "GTNX_ASG_FULL_SCORE_SCRATCH_BYTES", "GTNX_ASG_FULL_SCORE_GROUP"


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True)).to("cuda:0")  # (the cached cases are read-only)


def _run(gtn, em, trans, start, frames, w, want=("em", "table")):
    """Batch.asg_full_score and Batch.asg_full_score_grad -> (scores [B], d em or None, d table or None) as numpy"""
    import torch
    B, T, C = em.shape
    x, table = _dev(em), _dev(np.concatenate([start, trans.reshape(-1)]))
    sc = torch.full((B + 1,), SENTINEL, device="cuda:0")
    g = torch.full((B + 1, T, C), SENTINEL, device="cuda:0") if "em" in want else None
    gt = torch.full((C + C * C + 1,), SENTINEL, device="cuda:0") if "table" in want else None
    torch.cuda.synchronize()
    batch = gtn.Batch.linear(B, T, C, x, calc_grad=False, borrow=True)
    c0 = gtn.debug_asg_full_score_stats()
    batch.asg_full_score(table, sc[:B], frames)
    batch.asg_full_score_grad(table, _dev(w), None if g is None else g[:B], None if gt is None else gt[:-1], frames)
    gtn.synchronize()
    c1 = gtn.debug_asg_full_score_stats()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (2, 2 * B)
    assert (x.cpu().numpy().view(np.int32) == np.asarray(em).view(np.int32)).all()  # only read
    for guarded in (sc, g, gt):
        assert guarded is None or (guarded[-1] == SENTINEL).all(), "guard row"
    cpu = lambda t, n: None if t is None else t[:n].cpu().numpy()
    return cpu(sc, B), cpu(g, B), cpu(gt, C + C * C)


def _same_bits(a, b):
    return all(x is y is None or (x.view(np.int32) == y.view(np.int32)).all() for x, y in zip(a, b))


# ---- 1. against float64 ----
@pytest.mark.parametrize("shape", fp.SHAPES, ids=str)
def test_scores_and_gradients_against_float64(gtn, shape, monkeypatch):
    em, trans, start, frames, w, *want = fp.case(shape)
    if shape in fp.GROUPS:
        monkeypatch.setenv(GROUP, "16")  # (the default group of a small batch is 4: these shapes are the edges of 16)
    fp.check(str(shape), *_run(gtn, em, trans, start, frames, w), want, frames)


# ---- 2. pad rows are never read ----
def test_nan_in_the_pad_rows_changes_no_bit(gtn):
    em, trans, start, frames, w = fp.case((4, 9, 129))[:5]
    em_nan = em.copy()
    for b, f in enumerate(frames):
        em_nan[b, f:] = np.nan
    assert np.isnan(em_nan[1]).all()  # (the T_b == 0 utterance)
    assert _same_bits(_run(gtn, em_nan, trans, start, frames, w), _run(gtn, em, trans, start, frames, w))


# ---- 3. -inf is probability 0 ----
def test_minus_inf_in_emissions_start_and_transitions(gtn):
    em, trans, start, _, w = (np.array(a) for a in fp.case((4, 9, 33))[:5])
    frames = np.asarray([9, 9, 5, 9], np.int32)
    w[3] = 1.25
    trans[3, 7] = -np.inf   # a forbidden bigram
    trans[5, :] = -np.inf   # label 5 cannot be entered ...
    start[5] = -np.inf      # ... nor started with: a dead label
    em[0, 2, :4] = -np.inf
    em[1, 4, :] = -np.inf   # a -inf frame: no path
    got = _run(gtn, em, trans, start, frames, w)
    assert got[0][1] == -np.inf and not got[1][1].any()
    assert all(np.isfinite(a).all() for a in got[1:]) and not np.isnan(got[0]).any()
    # (asg_fp64 takes no -inf; exp(-1e5) is 0 in float64 as well.  Utterance 1 has no path: weight 0 there, -inf by hand)
    fin = lambda a: np.where(np.isneginf(a), np.float32(-1e5), a)
    want = fp.reference(fin(em), fin(trans), fin(start), frames, np.where(np.arange(4) == 1, 0, w))
    want[0][1] = -np.inf
    fp.check("-inf", *got, want, frames)
    alone = _run(gtn, em[[0, 2, 3]], trans, start, frames[[0, 2, 3]], w[[0, 2, 3]], want=("em",))
    assert _same_bits((got[0][[0, 2, 3]], got[1][[0, 2, 3]]), alone[:2])  # (the neighbours are unaffected)


# ---- 4. the same bits run to run ----
def test_the_same_call_twice_gives_the_same_bits(gtn):
    args = fp.case((17, 5, 33))[:5]
    assert _same_bits(_run(gtn, *args), _run(gtn, *args))


# ---- 6. only the gradients asked for ----
def test_only_the_gradients_asked_for(gtn):
    args = fp.case((17, 5, 33))[:5]
    both = _run(gtn, *args)
    em_only, table_only = _run(gtn, *args, want=("em",)), _run(gtn, *args, want=("table",))
    assert em_only[2] is None and table_only[1] is None
    assert _same_bits(both[:2], em_only[:2]) and _same_bits((both[0], both[2]), (table_only[0], table_only[2]))


# ---- 5. slices, groups and neighbours change no bit ----
@pytest.mark.parametrize("shape", [(35, 5, 33), (35, 3, 129), (4, 2, 1000)], ids=str)
def test_slices_groups_and_neighbours_change_no_bit(gtn, shape, monkeypatch):
    em, trans, start, frames, w = fp.case(shape)[:5]
    B, T, C = shape
    whole = _run(gtn, em, trans, start, frames, w)
    block = 16 * (2 * 4 * T * ((C + 31) // 32 * 32) + 8 * T)  # the planes of one block of 16 utterances
    for cap in (8 * block, 2 * block, 1):  # one slice, two blocks per slice, a block per slice
        monkeypatch.setenv(CAP, str(cap))
        assert _same_bits(whole, _run(gtn, em, trans, start, frames, w)), cap
    monkeypatch.delenv(CAP)
    for group in ("4", "8", "16"):
        monkeypatch.setenv(GROUP, group)
        assert _same_bits(whole, _run(gtn, em, trans, start, frames, w)), group
    monkeypatch.delenv(GROUP)
    for b in range(B):
        one = _run(gtn, em[b:b + 1], trans, start, frames[b:b + 1], w[b:b + 1], want=("em",))
        assert _same_bits((whole[0][b:b + 1], whole[1][b:b + 1]), one[:2]), b


# ---- 7. the torch entry under a non-uniform grad_out ----
def test_torch_entry_under_a_non_uniform_grad_out(gtn):
    import gtn_amd.torch_loss as tl
    shape = (4, 9, 129)
    em, trans, start, frames, w, *want = fp.case(shape)
    x, tr, st = (_dev(a).requires_grad_(True) for a in (em, trans, start))
    out = tl.asg_full_score(x, tr, st, input_lengths=frames)
    out.backward(_dev(w))
    g_tab = np.concatenate([st.grad.cpu().numpy(), tr.grad.cpu().numpy().reshape(-1)])
    fp.check("torch", out.detach().cpu().numpy(), x.grad.cpu().numpy(), g_tab, want, frames)


# ---- 8. consistency with the shipped launch at C <= 128 ----
@pytest.mark.parametrize("shape", [(4, 9, 33), (4, 9, 128)], ids=str)
def test_consistent_with_asg_full_connect(gtn, shape):
    import gtn_amd.torch_loss as tl
    em, trans, start, frames = fp.case(shape)[:4]
    live = np.flatnonzero(frames > 0)  # (the full-connect term's frame counts are 1 .. T)
    x, tr, st = _dev(em[live]), _dev(trans), _dev(start)
    new = tl.asg_full_score(x, tr, st, input_lengths=frames[live]).cpu().numpy()
    old = tl.asg_full_connect(x, tr, start=st, input_lengths=frames[live]).detach().cpu().numpy()
    for a, b in zip(new, old):
        assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (a, b)
