"""ASG loss over padded batches: every utterance of a [B, T, N] tensor has its own frame count T_b <= T.

Through torch_loss.asg_loss(input_lengths=...) (gtn_asg_loss_frames_n) and through the Batch API (Batch.linear(rows=...)
composed with the transitions graph, which stays symbolic for the launch of asg_full.hip).  The yardstick is
tests/asg_loss_fp.py on em[b, :T_b] -- float64, independent of the engine, pinned to the oracle by
tests/test_asg_frames_cpu.py.  The gate is the project's float64 gate for ASG (BASELINE, test_parity_gpu.py): losses
1e-4 * max(1, |fcc|, |fal|), emission gradients 1e-4 absolute, transitions and start gradients rtol 1e-3 / atol 1e-4;
gradient rows >= T_b are exactly 0 and the pad rows of the emissions are never read (NaN there changes no bit).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from asg_loss_fp import (DEAD_CASE, EDGE_SHAPES, GPU_SHAPES, LONG_SHAPES, MANY_CASE, SECOND_SEED, SEEDS, batch_fp64,
                         kill_emissions, seeded_case, shape_seed)
from ctc_fp64 import asg_fp64

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
MAX_LABELS = 128  # asg_full_max_labels() (gtn_amd/csrc/asg_full.hip): what DESIGN section 19 and README quote
LETTERS = (5, 40, 27, 9)
LIMIT = (2, 20, 128, 6)


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True)).to("cuda:0")  # (the cached cases are read-only)


@functools.lru_cache(maxsize=None)
def _case(shape, em_scale=1.0):
    """(em, em with NaN in every pad row, trans, start, targets, frames, the float64 yardstick over the batch)"""
    B, T, N, Umax = shape
    em, trans, start, targets, frames = seeded_case(shape_seed(shape), B, T, N, Umax, em_scale)
    assert frames[0] == T and 1 in frames.tolist() and any(f == len(t) for f, t in zip(frames, targets))
    em_nan = em.copy()
    for b, f in enumerate(frames):
        em_nan[b, f:] = np.nan
    ref = batch_fp64(em, trans, start, targets, frames)
    assert np.isfinite(ref["loss"]).all()
    for a in (em, em_nan, trans, start, frames) + tuple(ref.values()):
        a.setflags(write=False)
    return em, em_nan, trans, start, targets, frames, ref


def _torch_step(em, trans, start, targets, frames, reduction="sum", weights=None, grad=True, tr_grad=None):
    """asg_loss + backward -> (losses [B] or the reduced value, d em, d trans [N, N], d start [N]) as numpy (None where
    not asked for); weights: upstream gradient of reduction='none' (then only the emissions require a gradient, unless
    tr_grad=True asks for the transitions and start gradients beside them)"""
    import gtn_amd.torch_loss as tl
    tr_grad = weights is None if tr_grad is None else tr_grad
    e = _dev(em).requires_grad_(grad)
    t = _dev(trans).requires_grad_(grad and tr_grad)
    s = _dev(start).requires_grad_(grad and tr_grad)
    loss = tl.asg_loss(e, t, targets, start=s, reduction=reduction, input_lengths=frames)
    if grad:
        if weights is not None:
            loss.backward(_dev(np.asarray(weights, np.float32)))
        else:
            (loss.sum() if reduction == "none" else loss).backward()
    cpu = lambda x: None if x is None or x.grad is None else x.grad.cpu().numpy()
    return loss.detach().cpu().numpy(), cpu(e), cpu(t), cpu(s)


def _loss_tol(ref, b):
    return 1e-4 * max(1.0, abs(ref["fcc"][b]), abs(ref["fal"][b]))


def _check_em(tag, got, want, frames, scale):
    """emission gradients: rows < T_b to 1e-4 absolute, rows >= T_b exactly 0; figures printed before they are judged"""
    for b, f in enumerate(frames):
        assert not got[b, f:].any(), (tag, b, "pad rows of the gradient are not 0")
        w = want[b, :f] * (scale[b] if np.ndim(scale) else scale)
        err = np.abs(got[b, :f] - w).max()
        print(f"{tag} b={b} T_b={f} em grad abs {err:.2e}")
        assert np.isfinite(got[b]).all() and err <= 1e-4, (tag, b, err)


def _check_tr(tag, g_tr, g_st, want, N):
    err = np.abs(np.concatenate([g_st, g_tr.reshape(-1)]) - want).max()
    print(f"{tag} transitions grad abs {err:.2e} of max {np.abs(want).max():.3f}")
    np.testing.assert_allclose(g_st, want[:N], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(g_tr.reshape(-1), want[N:], rtol=1e-3, atol=1e-4)


# ---- 1. parity through asg_loss(input_lengths=) -----------------------------------------------------------------
@pytest.mark.parametrize("reduction", ["sum", "mean", "none"])
@pytest.mark.parametrize("shape", GPU_SHAPES, ids=str)
def test_torch_entry_against_float64(gtn, shape, reduction):
    em, _, trans, start, targets, frames, ref = _case(shape)
    B, T, N, _ = shape
    tag = f"{shape} {reduction}"
    f0, _ = gtn.debug_full_connect_stats()
    if reduction == "none":
        wts = np.linspace(0.5, 1.5, B).astype(np.float32)
        loss, g_em, _, _ = _torch_step(em, trans, start, targets, frames, "none", weights=wts)
        for b in range(B):
            print(f"{tag} b={b} loss {loss[b]:.6f} want {ref['loss'][b]:.6f} tol {_loss_tol(ref, b):.2e}")
            assert abs(loss[b] - ref["loss"][b]) <= _loss_tol(ref, b), (tag, b)
        _check_em(tag, g_em, ref["g_em"], frames, wts.astype(np.float64))
    else:
        k = 1.0 / B if reduction == "mean" else 1.0
        loss, g_em, g_tr, g_st = _torch_step(em, trans, start, targets, frames, reduction)
        want = ref["loss"].sum() * k
        tol = sum(_loss_tol(ref, b) for b in range(B)) * k
        print(f"{tag} loss {float(loss):.6f} want {want:.6f} tol {tol:.2e}")
        assert abs(float(loss) - want) <= tol, tag
        _check_em(tag, g_em, ref["g_em"], frames, k)
        _check_tr(tag, g_tr, g_st, ref["g_tr"].sum(0) * k, N)
    assert gtn.debug_full_connect_stats()[0] - f0 == B, "the launch of asg_full.hip did not take every utterance"


# ---- 2. the Batch API, both argument orders; 3. pad rows and the guard slab ---------------------------------------
def _transitions_graph(gtn, trans, start):
    from test_parity_gpu import asg_transitions
    N = len(start)
    g = asg_transitions(gtn, N, np.asarray(trans, np.float32).reshape(-1))
    w = g.weights_to_numpy().copy()
    w[:N] = start
    g.set_weights(w)
    return g


def _batch_step(gtn, em_dev, trans, start, frames, chain_first, em_grad=True, tr=None, root=None):
    """forward_score(compose(chains, transitions)) and backward through the Batch API; the emission gradient is bound
    into a tensor with one slab more than the batch, which must come back untouched.  em_grad=False: the chains ask
    for no gradient and must hold none afterwards (None is returned for it); tr: a transitions graph to run against
    (its calc_grad as the caller set it: None is returned for a gradient it does not ask for) instead of a fresh one;
    root: what backward starts from, as a function of the scores (gtn.negate: every utterance is seeded with -1)"""
    import torch
    B, T, N = em_dev.shape
    tr = _transitions_graph(gtn, trans, start) if tr is None else tr
    ems = gtn.Batch.linear(B, T, N, em_dev, em_grad, True, rows=frames)
    one = gtn.Batch([tr])
    grad = torch.full((B + 1, T, N), SENTINEL, device="cuda:0")
    off = np.arange(B, dtype=np.int64) * T * N
    if em_grad:
        ems.bind_grads(grad, off)
    score = gtn.forward_score(gtn.compose(ems, one) if chain_first else gtn.compose(one, ems))
    gtn.backward(score if root is None else root(score))
    if em_grad:
        ems.grads_to_device(grad, off)
    else:
        with pytest.raises(RuntimeError, match="Gradient not calculated"):
            ems.grads_to_device(grad, off)
    gtn.synchronize()
    g = grad.cpu().numpy()
    assert (g[B] == SENTINEL).all(), "the slab behind the bound gradient was written"
    assert em_grad or (g == SENTINEL).all(), "an emission gradient nobody asked for was written"
    return (np.asarray(score.items()), g[:B] if em_grad else None,
            tr.grad().weights_to_numpy() if tr.calc_grad else None)


@pytest.mark.parametrize("chain_first", [True, False], ids=["chain_first", "transitions_first"])
@pytest.mark.parametrize("shape", GPU_SHAPES, ids=str)
def test_batch_api_full_connect_term(gtn, shape, chain_first):
    em, em_nan, trans, start, targets, frames, _ = _case(shape)
    B, T, N, _ = shape
    tw = np.concatenate([start, trans.reshape(-1)])
    want = [asg_fp64(em[b, :f], tw)[:3] for b, f in enumerate(frames)]
    f0, b0 = gtn.debug_full_connect_stats()
    out = [_batch_step(gtn, _dev(e), trans, start, frames, chain_first) for e in (em, em_nan)]
    f1, b1 = gtn.debug_full_connect_stats()
    assert (f1 - f0, b1 - b0) == (2 * B, 0), "the launch of asg_full.hip did not take every utterance"
    score, g_em, g_tr = out[0]
    for b, f in enumerate(frames):
        z, w_em, _ = want[b]
        print(f"{shape} b={b} T_b={f} score {score[b]:.6f} want {z:.6f}")
        assert abs(score[b] - z) <= 1e-4 * max(1.0, abs(z)), (shape, b)
    _check_em(str(shape), g_em, np.stack([np.pad(w[1], ((0, T - w[1].shape[0]), (0, 0))) for w in want]), frames, 1.0)
    _check_tr(str(shape), g_tr[N:], g_tr[:N], np.sum([w[2] for w in want], 0), N)
    for x, y in zip(out[0], out[1]):
        assert np.array_equal(x, y), "NaN in the pad rows of the emissions changed an output"


@pytest.mark.parametrize("shape", [(4, 12, 5, 4), LETTERS, LIMIT], ids=str)
def test_pad_rows_are_never_read_and_their_gradient_is_zero(gtn, shape):
    em, em_nan, trans, start, targets, frames, ref = _case(shape)
    a = _torch_step(em, trans, start, targets, frames, "sum")
    b = _torch_step(em_nan, trans, start, targets, frames, "sum")
    for f, g in zip(frames, a[1]):
        assert not g[f:].any()
    for x, y in zip(a[:2], b[:2]):
        assert np.array_equal(x, y), "NaN in the pad rows of the emissions changed an output"
    # (the transitions gradient of the whole loss: bit for bit in test_batch_api_full_connect_term, where the new
    # launch is alone; here the force-align term's share arrives by float atomics -- band.hip: asg_fal_scatter_kernel --
    # whose order is not fixed, so it is held to the yardstick, NaN or not)
    _check_tr(f"{shape} NaN pad", b[2], b[3], ref["g_tr"].sum(0), shape[2])


# ---- 4. no existing behaviour changed ---------------------------------------------------------------------------------
_CHILD = "--full-connect-child"


@pytest.mark.parametrize("shape", [LETTERS, LIMIT], ids=str)
def test_without_lengths_the_old_route_runs_and_full_lengths_agree(gtn, shape, tmp_path):
    em, _, trans, start, targets, _, _ = _case(shape)
    B, T, N, _ = shape
    ref = batch_fp64(em, trans, start, targets, [T] * B)
    s0 = gtn.debug_full_connect_stats()
    none = _torch_step(em, trans, start, targets, None, "sum")
    full = _torch_step(em, trans, start, targets, [T] * B, "sum")  # (row counts all T are stored as no rows)
    assert gtn.debug_full_connect_stats() == s0, "a batch without a pad took the new route"
    out = str(tmp_path / "child.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), _CHILD, out, repr(shape)],
                       env=dict(os.environ, GTNX_FULL_CONNECT="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    z = np.load(out)
    assert int(z["fast"]) == B and int(z["fallback"]) == 0
    tol = sum(_loss_tol(ref, b) for b in range(B))
    for tag, got in (("None", none), ("all T", full), ("GTNX_FULL_CONNECT=1", (z["loss"], z["g_em"], z["g_tr"], z["g_st"]))):
        print(f"{shape} {tag} loss {float(got[0]):.6f} want {ref['loss'].sum():.6f}")
        assert abs(float(got[0]) - ref["loss"].sum()) <= tol, tag
        _check_em(tag, got[1], ref["g_em"], [T] * B, 1.0)
        _check_tr(tag, got[2], got[3], ref["g_tr"].sum(0), N)


def _full_connect_child(out, shape):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import gtn_amd as gtn
    assert os.environ.get("GTNX_FULL_CONNECT") == "1"
    em, _, trans, start, targets, _, _ = _case(shape)
    loss, g_em, g_tr, g_st = _torch_step(em, trans, start, targets, None, "sum")
    fast, fallback = gtn.debug_full_connect_stats()
    np.savez(out, loss=loss, g_em=g_em, g_tr=g_tr, g_st=g_st, fast=fast, fallback=fallback)


# ---- 5. bit-repeatable; 8. nothing carries over between calls -----------------------------------------------------
@pytest.mark.parametrize("shape", [LETTERS, LIMIT], ids=str)
def test_same_call_twice_same_bits(gtn, shape):
    """every output of the new launches twice over (scores, emission gradient, transitions gradient: the Batch API,
    where they are alone), and the loss and emission gradient of asg_loss; asg_loss's transitions gradient also carries
    the force-align term's share, which band.hip scatters with float atomics in no fixed order -- that sum is held to
    the yardstick, not to its own bits"""
    em, _, trans, start, targets, frames, ref = _case(shape)
    x = [_batch_step(gtn, _dev(em), trans, start, frames, True) for _ in range(2)]
    for u, v in zip(x[0], x[1]):
        assert np.array_equal(u, v)
    a = _torch_step(em, trans, start, targets, frames, "sum")
    b = _torch_step(em, trans, start, targets, frames, "sum")
    for u, v in zip(a[:2], b[:2]):
        assert np.array_equal(u, v)
    # (the second call ran on the cached transitions structure: its gradient is the batch's, not twice that)
    _check_tr(str(shape), b[2], b[3], ref["g_tr"].sum(0), shape[2])


# ---- 6. range -----------------------------------------------------------------------------------------------------
def test_forbidden_transitions_and_starts(gtn):
    """-inf start scores and transitions (a label that may not repeat, a pair that may not follow each other): the
    yardstick is finite by construction, and nothing is NaN"""
    B, T, N = 4, 14, 9
    em, trans, start, _, _ = seeded_case(77, B, T, N, 5)
    trans, start = trans.copy(), start.copy()
    trans[3, 3] = trans[5, 5] = trans[1, 6] = -np.inf
    start[[0, 4, 8]] = -np.inf
    targets = [[2, 3, 5, 3], [1, 7], [6], [3, 1, 1, 2, 5]]
    frames = np.asarray([T, 2, 1, 9], np.int32)
    ref = batch_fp64(em, trans, start, targets, frames)
    assert np.isfinite(ref["loss"]).all()
    loss, g_em, g_tr, g_st = _torch_step(em, trans, start, targets, frames, "none")
    for b in range(B):
        print(f"forbidden b={b} loss {loss[b]:.6f} want {ref['loss'][b]:.6f}")
        assert abs(loss[b] - ref["loss"][b]) <= _loss_tol(ref, b), b
    _check_em("forbidden", g_em, ref["g_em"], frames, 1.0)
    assert np.isfinite(g_tr).all() and np.isfinite(g_st).all()
    _check_tr("forbidden", g_tr, g_st, ref["g_tr"].sum(0), N)


@pytest.mark.parametrize("shape", [(4, 12, 5, 4), LETTERS], ids=str)
def test_emissions_scaled_by_30(gtn, shape):
    em, _, trans, start, targets, frames, ref = _case(shape, 30.0)
    B, T, N, _ = shape
    loss, g_em, g_tr, g_st = _torch_step(em, trans, start, targets, frames, "none")
    for b in range(B):
        print(f"x30 {shape} b={b} loss {loss[b]:.4f} want {ref['loss'][b]:.4f} tol {_loss_tol(ref, b):.2e}")
        assert abs(loss[b] - ref["loss"][b]) <= _loss_tol(ref, b), b
    _check_em(f"x30 {shape}", g_em, ref["g_em"], frames, 1.0)
    _check_tr(f"x30 {shape}", g_tr, g_st, ref["g_tr"].sum(0), N)


# ---- 7. an utterance with fewer frames than labels ----------------------------------------------------------------
def test_infeasible_utterance_is_plus_inf_and_its_neighbours_hold(gtn):
    em, _, trans, start, targets, frames, _ = _case(LETTERS)
    targets = [list(t) for t in targets]
    frames = np.array(frames)
    targets[3] = [1, 2, 3, 4, 5, 6]
    frames[3] = 4
    ref = batch_fp64(em, trans, start, targets, frames)
    assert ref["loss"][3] == np.inf and np.isfinite(np.delete(ref["loss"], 3)).all()
    loss, _, _, _ = _torch_step(em, trans, start, targets, frames, "none", grad=False)
    assert loss[3] == np.inf
    for b in (0, 1, 2, 4):
        assert abs(loss[b] - ref["loss"][b]) <= _loss_tol(ref, b), b


# ---- 9. the reference's known answers, padded -----------------------------------------------------------------------
def test_reference_known_answers_in_a_padded_batch(gtn):
    """test/criterion_test.cpp:182-306 with three rows of pad behind every utterance and input_lengths = [5, 5, 5]"""
    import torch
    import gtn_amd.torch_loss as tl
    from test_parity_gpu import ASG_EM_GRADS, ASG_EMISSIONS, ASG_TRANS_GRAD
    T, N = 5, 6
    targets = [[2, 1, 5, 1, 3], [4, 3, 5], [3, 2, 2, 1]]
    expected_loss = [7.7417464256287, 6.4200420379639, 8.2780694961548]
    x = np.full((3, T + 3, N), np.nan, np.float32)
    x[:, :T] = np.asarray(ASG_EMISSIONS, np.float32).reshape(3, T, N)
    em = torch.from_numpy(x).cuda().requires_grad_(True)
    tr = torch.zeros(N, N, device="cuda", requires_grad=True)
    st = torch.zeros(N, device="cuda", requires_grad=True)
    for _ in range(2):  # second pass: cached transitions structure, gradients must not carry over
        em.grad = tr.grad = st.grad = None
        loss = tl.asg_loss(em, tr, targets, start=st, reduction="none", input_lengths=[5, 5, 5])
        loss.sum().backward()
        np.testing.assert_allclose(loss.detach().cpu().numpy(), expected_loss, atol=1e-3)
        g = em.grad.cpu().numpy()
        assert not g[:, T:].any()
        np.testing.assert_allclose(g[:, :T].reshape(3, -1), np.asarray(ASG_EM_GRADS), atol=1e-4)
        np.testing.assert_allclose(tr.grad.cpu().numpy().reshape(-1), ASG_TRANS_GRAD, atol=1e-4)
        assert abs(st.grad.cpu().numpy().sum()) < 1e-4


# ---- 10. an alphabet above the launch's limit -----------------------------------------------------------------------
def test_alphabet_above_the_limit_takes_the_composed_elements(gtn):
    B, T, N = 3, 10, MAX_LABELS + 4
    em, _, trans, start, targets, frames, ref = _case((B, T, N, 4))
    assert len(set(frames.tolist())) == B
    s0 = gtn.debug_full_connect_stats()
    loss, g_em, g_tr, g_st = _torch_step(em, trans, start, targets, frames, "none")
    s1 = gtn.debug_full_connect_stats()
    assert (s1[0] - s0[0], s1[1] - s0[1]) == (0, B), "the fallback did not take the utterances"
    for b in range(B):
        print(f"N={N} b={b} loss {loss[b]:.6f} want {ref['loss'][b]:.6f}")
        assert abs(loss[b] - ref["loss"][b]) <= _loss_tol(ref, b), b
    _check_em(f"N={N}", g_em, ref["g_em"], frames, 1.0)
    _check_tr(f"N={N}", g_tr, g_st, ref["g_tr"].sum(0), N)


# ---- 11. the edges of the launch's layout: N = 3 / 4, 16 / 17, 31 / 32 / 33 ------------------------------------------
def _full_connect_fp64(em, trans, start, frames, skip=()):
    """asg_fp64 per utterance on em[b, :T_b]: (scores [B], d em [B, T, N] with zeros in the pad rows, d transitions
    [B, N + N * N]); utterances in `skip` are not asked (zeros, score nan)"""
    B, T, N = em.shape
    tw = np.concatenate([start, trans.reshape(-1)])
    z, g_em, g_tr = np.full(B, np.nan), np.zeros((B, T, N)), np.zeros((B, N + N * N))
    with np.errstate(divide="ignore", invalid="ignore"):
        for b, f in enumerate(frames):
            if b not in skip:
                z[b], g_em[b, :f], g_tr[b] = asg_fp64(em[b, :f], tw)[:3]
    return z, g_em, g_tr


def _check_scores(tag, score, want, frames, skip=()):
    for b, f in enumerate(frames):
        if b in skip:
            continue
        print(f"{tag} b={b} T_b={f} score {score[b]:.6f} want {want[b]:.6f}")
        assert abs(score[b] - want[b]) <= 1e-4 * max(1.0, abs(want[b])), (tag, b)


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=str)
def test_layout_edges_through_both_entries(gtn, shape):
    em, em_nan, trans, start, targets, frames, ref = _case(shape)
    B, T, N, _ = shape
    f0 = gtn.debug_full_connect_stats()
    loss, g_em, g_tr, g_st = _torch_step(em, trans, start, targets, frames, "sum")
    f1 = gtn.debug_full_connect_stats()
    assert (f1[0] - f0[0], f1[1] - f0[1]) == (B, 0), "the launch of asg_full.hip did not take every utterance"
    want = ref["loss"].sum()
    tol = sum(_loss_tol(ref, b) for b in range(B))
    print(f"{shape} sum loss {float(loss):.6f} want {want:.6f} tol {tol:.2e}")
    assert abs(float(loss) - want) <= tol
    _check_em(f"{shape} sum", g_em, ref["g_em"], frames, 1.0)
    _check_tr(f"{shape} sum", g_tr, g_st, ref["g_tr"].sum(0), N)
    out = []
    for e in (em, em_nan):
        f0 = gtn.debug_full_connect_stats()
        out.append(_batch_step(gtn, _dev(e), trans, start, frames, True))
        f1 = gtn.debug_full_connect_stats()
        assert (f1[0] - f0[0], f1[1] - f0[1]) == (B, 0), "the launch of asg_full.hip did not take every utterance"
    z, w_em, w_tr = _full_connect_fp64(em, trans, start, frames)
    score, g_em, g_tr = out[0]
    _check_scores(str(shape), score, z, frames)
    _check_em(str(shape), g_em, w_em, frames, 1.0)
    _check_tr(str(shape), g_tr[N:], g_tr[:N], w_tr.sum(0), N)
    for x, y in zip(out[0], out[1]):
        assert np.array_equal(x, y), "NaN in the pad rows of the emissions changed an output"


# ---- 12. utterances of production length ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", LONG_SHAPES, ids=str)
def test_long_utterances_through_asg_loss(gtn, shape):
    """the scaled recursion over 1200 and 600 frames beside utterances of 30 / 20 frames and of one: per-utterance
    losses, emission gradients utterance by utterance (pad rows == 0), transitions and start gradients"""
    em, _, trans, start, targets, frames, ref = _case(shape)
    B, T, N, _ = shape
    f0, _ = gtn.debug_full_connect_stats()
    loss, g_em, g_tr, g_st = _torch_step(em, trans, start, targets, frames, "none")
    assert gtn.debug_full_connect_stats()[0] - f0 == B
    for b in range(B):
        print(f"{shape} b={b} T_b={frames[b]} loss {loss[b]:.6f} want {ref['loss'][b]:.6f} tol {_loss_tol(ref, b):.2e}")
        assert abs(loss[b] - ref["loss"][b]) <= _loss_tol(ref, b), (shape, b)
    _check_em(f"{shape} long", g_em, ref["g_em"], frames, 1.0)
    _check_tr(f"{shape} long", g_tr, g_st, ref["g_tr"].sum(0), N)


@pytest.mark.parametrize("shape", LONG_SHAPES, ids=str)
def test_long_utterances_full_connect_term_alone(gtn, shape):
    em, _, trans, start, _, frames, _ = _case(shape)
    N = shape[2]
    z, w_em, w_tr = _full_connect_fp64(em, trans, start, frames)
    score, g_em, g_tr = _batch_step(gtn, _dev(em), trans, start, frames, True)
    _check_scores(f"{shape} long batch", score, z, frames)
    _check_em(f"{shape} long batch", g_em, w_em, frames, 1.0)
    _check_tr(f"{shape} long batch", g_tr[N:], g_tr[:N], w_tr.sum(0), N)


# ---- 13. more utterances than compute units -----------------------------------------------------------------------------
def test_more_utterances_than_compute_units(gtn):
    """300 workgroups, 300 slices for asg_full_reduce_kernel to add in utterance order: scores, emission gradients and
    the transitions gradient against the yardstick's sum, the same bits twice, the guard slab untouched (_batch_step)"""
    em, trans, start, _, frames = seeded_case(*MANY_CASE)
    B, T, N = em.shape
    assert B == 300 and set(frames.tolist()) == set(range(1, T + 1))
    z, w_em, w_tr = _full_connect_fp64(em, trans, start, frames)
    assert np.isfinite(z).all()
    f0 = gtn.debug_full_connect_stats()
    x = [_batch_step(gtn, _dev(em), trans, start, frames, True) for _ in range(2)]
    f1 = gtn.debug_full_connect_stats()
    assert (f1[0] - f0[0], f1[1] - f0[1]) == (2 * B, 0)
    score, g_em, g_tr = x[0]
    err = np.abs(score - z) / np.maximum(1.0, np.abs(z))
    print(f"many: score rel {err.max():.2e}")
    assert (err <= 1e-4).all(), int(err.argmax())
    err = np.abs(g_em - w_em).reshape(B, -1).max(1)
    print(f"many: em grad abs {err.max():.2e}")
    assert np.isfinite(g_em).all() and (err <= 1e-4).all(), int(err.argmax())
    for b, f in enumerate(frames):
        assert not g_em[b, f:].any(), (b, "pad rows of the gradient are not 0")
    _check_tr("many", g_tr[N:], g_tr[:N], w_tr.sum(0), N)
    for u, v in zip(x[0], x[1]):
        assert np.array_equal(u, v)


# ---- 14. -inf emissions and an utterance without a path ---------------------------------------------------------------
def test_dead_emissions_and_an_utterance_without_a_path(gtn):
    """-inf in the emissions is probability 0; an utterance whose every path is -inf has score -inf
    and a gradient of zeros that the backward kernel STORES (its early return), never 0 * inf.  The values asked of
    utterance 1 are stated, not computed: the float64 yardstick is NaN there.  Full-connect term only -- the
    force-align term of such a batch is -inf and the loss +inf."""
    em, trans, start, _, frames = seeded_case(*DEAD_CASE)
    assert frames.tolist() == [12, 4, 1, 5]
    B, T, N = em.shape
    em = kill_emissions(em)
    em_nan = em.copy()
    for b, f in enumerate(frames):
        em_nan[b, f:] = np.nan
    z, w_em, w_tr = _full_connect_fp64(em, trans, start, frames, skip=(1,))
    assert np.isfinite(np.delete(z, 1)).all() and np.isfinite(w_em).all() and np.isfinite(w_tr).all()
    out = [_batch_step(gtn, _dev(e), trans, start, frames, True) for e in (em, em_nan)]
    score, g_em, g_tr = out[0]
    assert score[1] == -np.inf
    assert not np.isnan(score).any() and not np.isnan(g_em).any() and not np.isnan(g_tr).any()
    assert not g_em[1].any(), "the utterance without a path has a gradient"
    assert not g_em[np.isneginf(em)].any(), "an emission of probability 0 has a gradient"
    _check_scores("dead", score, z, frames, skip=(1,))
    _check_em("dead", g_em, w_em, frames, 1.0)  # (utterance 1: zeros against the zeros stated above)
    _check_tr("dead", g_tr[N:], g_tr[:N], w_tr[[0, 2, 3]].sum(0), N)
    for x, y in zip(out[0], out[1]):
        assert np.array_equal(x, y), "NaN in the pad rows of the emissions changed an output"


# ---- 15. which gradients are asked for ----------------------------------------------------------------------------------
def test_only_the_gradients_asked_for(gtn):
    """transitions only (the xi kernel with no emission gradient to store), emissions only (the kernel without xi),
    neither (nothing kept by the forward launch; backward does nothing and raises nothing).  The scores are the
    both-wanted run's bit for bit: one forward kernel, and keeping la / L only adds stores."""
    em, _, trans, start, _, frames, _ = _case(LETTERS)
    N = LETTERS[2]
    z, w_em, w_tr = _full_connect_fp64(em, trans, start, frames)
    both = _batch_step(gtn, _dev(em), trans, start, frames, True)
    _check_scores("both", both[0], z, frames)

    def step(em_grad, tr_grad):
        tr = _transitions_graph(gtn, trans, start)
        tr.calc_grad = tr_grad
        score, g_em, g_tr = _batch_step(gtn, _dev(em), trans, start, frames, True, em_grad=em_grad, tr=tr)
        assert np.array_equal(score, both[0]), (em_grad, tr_grad, "the scores depend on which gradients are wanted")
        assert tr_grad or not tr.is_grad_available()
        return g_em, g_tr

    g_em, g_tr = step(False, True)
    assert g_em is None
    _check_tr("transitions only", g_tr[N:], g_tr[:N], w_tr.sum(0), N)
    assert np.array_equal(g_tr, both[2]), "the transitions gradient depends on whether the emissions want one"
    g_em, g_tr = step(True, False)
    assert g_tr is None
    _check_em("emissions only", g_em, w_em, frames, 1.0)
    assert step(False, False) == (None, None)


# ---- 16. upstream gradients: zero, negative ---------------------------------------------------------------------------
def test_upstream_seeds_zero_and_negative(gtn):
    """reduction='none' with seeds [0, -1.5, 2, 0.5, 1]: the zero-seed utterance's emission rows are exactly 0, the
    others w_b times the yardstick.  asg_loss REFUSES a transitions gradient under per-utterance seeds that differ
    (torch_loss.py: the criterion sums it over the batch with unit seeds; RuntimeError) -- a documented limit, pinned
    here; inside the contract the transitions gradient is held to the yardstick under a uniform negative seed.
    asg_loss hands the launch unit seeds and scales afterwards, so the kernel's own `delta` is reached through the
    Batch API: negate(score) seeds every utterance with -1, subtract(score, score) with 0."""
    em, _, trans, start, targets, frames, ref = _case(LETTERS)
    B, T, N, _ = LETTERS
    w = np.asarray(SEEDS, np.float64)
    loss, g_em, _, _ = _torch_step(em, trans, start, targets, frames, "none", weights=SEEDS)
    for b in range(B):
        assert abs(loss[b] - ref["loss"][b]) <= _loss_tol(ref, b), b
    assert not g_em[0].any(), "a seed of 0 left a gradient"
    _check_em("seeds", g_em, ref["g_em"], frames, w)
    with pytest.raises(RuntimeError, match="uniform upstream"):
        _torch_step(em, trans, start, targets, frames, "none", weights=SEEDS, tr_grad=True)
    _, g_em, g_tr, g_st = _torch_step(em, trans, start, targets, frames, "none", weights=[-1.5] * B, tr_grad=True)
    _check_em("seed -1.5", g_em, ref["g_em"], frames, -1.5)
    _check_tr("seed -1.5", g_tr, g_st, -1.5 * ref["g_tr"].sum(0), N)
    # the kernel's delta
    z, w_em, w_tr = _full_connect_fp64(em, trans, start, frames)
    score, g_em, g_tr = _batch_step(gtn, _dev(em), trans, start, frames, True, root=gtn.negate)
    _check_scores("negate", score, z, frames)
    _check_em("negate", g_em, w_em, frames, -1.0)
    _check_tr("negate", g_tr[N:], g_tr[:N], -w_tr.sum(0), N)
    score, g_em, g_tr = _batch_step(gtn, _dev(em), trans, start, frames, True, root=lambda s: gtn.subtract(s, s))
    _check_scores("x - x", score, z, frames)
    assert not g_em.any() and not g_tr.any(), "a seed of 0 left a gradient"


# ---- 17. a transitions graph that already holds a gradient ----------------------------------------------------------------
def test_transitions_gradient_accumulates_until_zero_grad(gtn):
    """two different padded batches against the SAME transitions graph, backward on each without zero_grad: the
    graph holds the sum (BFullOp: add_grad_device); after zero_grad and one more step, the single one"""
    shape = (4, 12, 5, 4)
    em1, _, trans, start, _, fr1, _ = _case(shape)
    em2, _, _, _, fr2 = seeded_case(SECOND_SEED, *shape)
    N = shape[2]
    w1 = _full_connect_fp64(em1, trans, start, fr1)[2].sum(0)
    w2 = _full_connect_fp64(em2, trans, start, fr2)[2].sum(0)
    tr = _transitions_graph(gtn, trans, start)
    _, _, g = _batch_step(gtn, _dev(em1), trans, start, fr1, True, tr=tr)
    _check_tr("first", g[N:], g[:N], w1, N)
    _, _, g = _batch_step(gtn, _dev(em2), trans, start, fr2, True, tr=tr)
    _check_tr("first + second", g[N:], g[:N], w1 + w2, N)
    tr.zero_grad()
    _, _, g = _batch_step(gtn, _dev(em2), trans, start, fr2, True, tr=tr)
    _check_tr("second after zero_grad", g[N:], g[:N], w2, N)


if __name__ == "__main__" and len(sys.argv) == 4 and sys.argv[1] == _CHILD:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _full_connect_child(sys.argv[2], eval(sys.argv[3]))
