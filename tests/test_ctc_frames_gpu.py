"""CTC loss over padded batches: every utterance of a [B, T, C] tensor has its own frame count T_b <= T.

Through the Batch API (Batch.linear(rows=...), gtnx_batch_linear_rows) and through torch_loss.ctc_loss(input_lengths=...),
native and Python routes.  The yardstick is tests/ctc_fp64.py on em[b, :T_b] -- float64, independent of the engine, and
pinned to torch.nn.functional.ctc_loss(..., input_lengths) on these very inputs by tests/test_ctc_frames_cpu.py.  The
gate is the project's float64 gate: losses 1e-4 relative, emission gradients 1e-4 absolute; gradient rows >= T_b are
exactly 0, and the values of the pad rows are never read (NaN there changes nothing).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from ctc_align_fp import min_frames
from ctc_fp64 import ctc_loss_fp64
from test_ctc_frames_cpu import CASES, frames_case

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
BASE = (11, 4, 60, 12, 7)


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True)).to("cuda:0")  # (the cached cases are read-only)


@functools.lru_cache(maxsize=None)
def _case(key):
    """(em, em with NaN in every pad row, targets, frames, [(loss, grad[T_b, C]) in float64])"""
    em, targets, frames = frames_case(key)
    em_nan = em.copy()
    for b, f in enumerate(frames):
        em_nan[b, f:] = np.nan
    ref = [ctc_loss_fp64(em[b, :f], targets[b])[:2] for b, f in enumerate(frames)]
    for a in (em, em_nan):
        a.setflags(write=False)
    return em, em_nan, targets, frames, ref


def _check(tag, losses, grad, frames, ref, skip=()):
    """the float64 gate on rows < T_b, exact zeros on rows >= T_b; the figures are printed before they are judged"""
    losses, grad = np.asarray(losses), np.asarray(grad)
    for b, f in enumerate(frames):
        assert not grad[b, f:].any(), (tag, b, "pad rows of the gradient are not 0")
        if b in skip:
            continue
        want, wgrad = ref[b]
        lerr = abs(float(losses[b]) - want) / abs(want)
        gerr = np.abs(grad[b, :f] - wgrad).max()
        print(f"{tag} b={b} T_b={f} loss {losses[b]:.6f} want {want:.6f} rel {lerr:.2e} grad abs {gerr:.2e}")
        assert np.isfinite(want) and lerr <= 1e-4, (tag, b, losses[b], want)
        assert gerr <= 1e-4, (tag, b, gerr)


def _batch_step(gtn, em_dev, targets, frames, chain_first=False, guard=True):
    """loss and gradient through the Batch API; the gradient is bound into a tensor with one slab more than the batch,
    which must come back untouched.  -> (losses [B], grad [B, T, C], the batches)"""
    import torch
    B, T, C = em_dev.shape
    ctcs = gtn.Batch.ctc_targets(targets, 0, False)
    ems = gtn.Batch.linear(B, T, C, em_dev, True, True, rows=frames)
    grad = torch.full((B + 1, T, C), SENTINEL, device="cuda:0")
    off = np.arange(B, dtype=np.int64) * T * C
    ems.bind_grads(grad, off)
    prod = gtn.intersect(ems, ctcs) if chain_first else gtn.intersect(ctcs, ems)
    score = gtn.forward_score(prod)
    loss = gtn.subtract(gtn.forward_score(ems), score)
    gtn.backward(loss)
    ems.grads_to_device(grad, off)
    gtn.synchronize()
    g = grad.cpu().numpy()
    if guard:
        assert (g[B] == SENTINEL).all(), "the slab behind the bound gradient was written"
    return np.asarray(loss.items()), g[:B], (ctcs, ems, loss)


def _torch_step(tl, em_dev, targets, frames, native):
    tl._NATIVE = None if native else False
    try:
        if native:
            assert tl._native() and hasattr(tl._native(), "gtn_ctc_loss_frames_n"), "libgtn_criteria.so (build())"
        lp = em_dev.clone().requires_grad_(True)
        loss = tl.ctc_loss(lp, targets, blank=0, reduction="none", input_lengths=frames)
        loss.sum().backward()
        return loss.detach().cpu().numpy(), lp.grad.cpu().numpy()
    finally:
        tl._NATIVE = None


ROUTES = ["batch", "batch_chain_first", "torch_native", "torch_python"]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("key", CASES, ids=str)
def test_values(gtn, key, route):
    """losses and gradient rows < T_b against float64, rows >= T_b exactly 0, and the same bits with NaN in every pad
    row of the emissions"""
    import gtn_amd.torch_loss as tl
    em, em_nan, targets, frames, ref = _case(key)
    out = []
    for e in (em, em_nan):
        if route.startswith("batch"):
            losses, grad, _ = _batch_step(gtn, _dev(e), targets, frames, chain_first=route.endswith("first"))
        else:
            losses, grad = _torch_step(tl, _dev(e), targets, frames, native=route == "torch_native")
        out.append((losses, grad))
    _check(f"{key} {route}", out[0][0], out[0][1], frames, ref)
    assert np.array_equal(out[0][0], out[1][0]), "NaN in the pad rows changed a loss"
    assert np.array_equal(out[0][1], out[1][1]), "NaN in the pad rows changed a gradient"


@pytest.mark.parametrize("key", [BASE, (12, 4, 60, 9, 7)], ids=str)
def test_full_length_rows_are_the_plain_batch(gtn, key):
    """rows = [T] * B is rows = None bit for bit (no pad: no fill launch), through the Batch API and through the torch
    entry's two routes; input_lengths = None never reaches the new symbol, Batch.linear(rows=) or the fill"""
    import gtn_amd.torch_loss as tl
    em, _, targets, _, _ = _case(key)
    B, T, C = em.shape
    em_dev = _dev(em)
    full = [T] * B
    gtn.prof_reset()
    gtn.prof_enable(True)
    l0, g0, _ = _batch_step(gtn, em_dev, targets, None)
    l1, g1, _ = _batch_step(gtn, em_dev, targets, full)
    gtn.prof_enable(False)
    assert "band_forward_score" in gtn.prof_names() and "linear_pad_fill" not in gtn.prof_names()
    assert np.array_equal(l0, l1) and np.array_equal(g0, g1)
    # the torch entry without lengths: today's code path -- the frames symbol and Batch.linear are not touched
    lib = tl._native()
    assert lib, "gtn_amd/lib/libgtn_criteria.so missing (build())"

    def never(*a, **k):
        raise AssertionError("input_lengths=None took the padded route")

    real_sym, real_linear = lib.gtn_ctc_loss_frames_n, gtn.Batch.linear
    none = {}
    gtn.prof_reset()
    gtn.prof_enable(True)
    try:
        lib.gtn_ctc_loss_frames_n = never
        gtn.Batch.linear = never
        for native in (True, False):
            none[native] = _torch_step(tl, em_dev, targets, None, native)
    finally:
        lib.gtn_ctc_loss_frames_n, gtn.Batch.linear = real_sym, real_linear
        gtn.prof_enable(False)
    assert "linear_pad_fill" not in gtn.prof_names()
    # full lengths, native: the same call with a null table underneath -- bit-equal to no lengths
    ln, gn = _torch_step(tl, em_dev, targets, full, True)
    assert np.array_equal(ln, none[True][0]) and np.array_equal(gn, none[True][1])
    # full lengths, Python route: the Batch expression of _batch_step -- bit-equal to it without rows (the route without
    # lengths is the per-graph one of pytorch_loss.py: another expression, held to the float64 gate in test_parity_gpu)
    lpy, gpy = _torch_step(tl, em_dev, targets, full, False)
    assert np.array_equal(lpy, l0) and np.array_equal(gpy, g0)


def test_fill_launch_only_with_a_pad(gtn):
    """one fill launch per backward pass of a ragged batch, of exactly the pad's bytes"""
    em, _, targets, frames, _ = _case(BASE)
    B, T, C = em.shape
    gtn.prof_reset()
    gtn.prof_enable(True)
    _batch_step(gtn, _dev(em), targets, frames)
    gtn.prof_enable(False)
    p = gtn.prof_get("linear_pad_fill")
    assert p["launches"] == 1 and p["algorithmic_bytes"] == 4.0 * C * sum(T - int(f) for f in frames)


def test_infeasible_neighbour(gtn):
    """one utterance a frame short of its target: its loss is +inf and its gradient rows are those of the unpadded
    single-utterance call on em[b:b+1, :T_b]; the others keep the float64 gate; every pad row is 0"""
    import gtn_amd.torch_loss as tl
    em, em_nan, targets, frames, ref = _case(BASE)
    B, T, C = em.shape
    bad = 2
    short = frames.copy()
    short[bad] = min_frames(targets[bad]) - 1
    assert short[bad] >= 1
    e = em_nan.copy()
    e[bad, short[bad]:] = np.nan
    f = int(short[bad])
    alone = np.ascontiguousarray(em[bad:bad + 1, :f])
    for route in ("batch", "torch_native"):
        if route == "batch":
            losses, grad, _ = _batch_step(gtn, _dev(e), targets, short)
            l1, g1, _ = _batch_step(gtn, _dev(alone), [targets[bad]], None)
        else:
            losses, grad = _torch_step(tl, _dev(e), targets, short, True)
            l1, g1 = _torch_step(tl, _dev(alone), [targets[bad]], None, True)
        assert losses[bad] == np.inf and l1[0] == np.inf, (route, losses, l1)
        _check(f"infeasible {route}", losses, grad, short, ref, skip=(bad,))
        np.testing.assert_allclose(grad[bad, :f], g1[0], rtol=1e-5, atol=0, equal_nan=True)


_CHILD = "no_band_child"


def test_fallback_routes_honour_rows(gtn, tmp_path):
    """GTNX_NO_BAND=1 in a fresh process: the Batch expression and the per-graph expression over the elements taken
    out of the ragged batch (ems[b]: linear graphs of T_b rows) both keep the float64 gate; forward_score of the bare
    chains is the float64 sum of T_b row log-sum-exps; element b has T_b + 1 nodes"""
    em, em_nan, targets, frames, ref = _case(BASE)
    B, T, C = em.shape
    em_dev = _dev(em_nan)  # (borrowed by `ems`: held until the end)
    ems = gtn.Batch.linear(B, T, C, em_dev, False, True, rows=frames)
    got = np.asarray(gtn.forward_score(ems).items())
    for b, f in enumerate(frames):
        x = em[b, :f].astype(np.float64)
        m = x.max(1)
        want = float(np.sum(m + np.log(np.exp(x - m[:, None]).sum(1))))
        assert abs(got[b] - want) <= 1e-4 * abs(want), (b, got[b], want)
    for b, f in enumerate(frames):
        assert ems[b].num_nodes() == f + 1 and ems[b].num_arcs() == f * C
    # (elements taken out: the same values through the per-graph route)
    got = np.asarray(gtn.forward_score(ems).items())
    for b, f in enumerate(frames):
        x = em[b, :f].astype(np.float64)
        m = x.max(1)
        want = float(np.sum(m + np.log(np.exp(x - m[:, None]).sum(1))))
        assert abs(got[b] - want) <= 1e-4 * abs(want), (b, got[b], want)
    out = str(tmp_path / "child.npz")
    env = dict(os.environ, GTNX_NO_BAND="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), _CHILD, out], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    z = np.load(out)
    _check("no_band batch", z["l_batch"], z["g_batch"], frames, ref)
    _check("no_band elements", z["l_elem"], z["g_elem"], frames, ref)


def _no_band_child(out):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch
    import gtn_amd as gtn
    import gtn_amd.torch_loss as tl
    assert os.environ.get("GTNX_NO_BAND") == "1"
    em, em_nan, targets, frames, _ = _case(BASE)
    B, T, C = em.shape
    l_batch, g_batch, _ = _batch_step(gtn, _dev(em_nan), targets, frames)
    # the elements as graphs, the targets built on the host: compose / forwardScore / backward per graph, the gradients
    # gathered from the element graphs into the [B][T][C] layout
    em_dev = _dev(em_nan)  # (borrowed by `ems`: held until the end)
    ems = gtn.Batch.linear(B, T, C, em_dev, True, True, rows=frames)
    chains = [ems[b] for b in range(B)]
    tgs = [tl.ctc_target_graph(list(t), 0) for t in targets]
    loss = gtn.subtract(gtn.forward_score(chains), gtn.forward_score(gtn.intersect(tgs, chains)))
    gtn.backward(loss)
    grad = torch.full((B + 1, T, C), SENTINEL, device="cuda:0")
    ems.grads_to_device(grad, np.arange(B, dtype=np.int64) * T * C)
    gtn.synchronize()
    g = grad.cpu().numpy()
    assert (g[B] == SENTINEL).all()
    np.savez(out, l_batch=l_batch, g_batch=g_batch, l_elem=np.asarray(gtn.items(loss)), g_elem=g[:B])


def test_retained_tape(gtn):
    """backward twice over a retained tape: the second pass goes through a scratch block that is folded in -- the pad
    rows stay exactly 0 (whatever the block held) and rows < T_b stay finite; the first pass is test_values'"""
    import torch
    em, em_nan, targets, frames, ref = _case(BASE)
    B, T, C = em.shape
    # (blocks of NaN through the engine's pool first: what a scratch block may hold)
    nan_dev = _dev(np.full((B, T, C), np.nan, np.float32))
    junk = gtn.Batch.linear(B, T, C, nan_dev, False, False)
    gtn.synchronize()
    del junk
    ctcs = gtn.Batch.ctc_targets(targets, 0, False)
    em_dev = _dev(em_nan)  # (borrowed by `ems`: held until the end)
    ems = gtn.Batch.linear(B, T, C, em_dev, True, True, rows=frames)
    score = gtn.forward_score(gtn.intersect(ctcs, ems))
    loss = gtn.subtract(gtn.forward_score(ems), score)
    off = np.arange(B, dtype=np.int64) * T * C
    grads = []
    for _ in range(2):
        gtn.backward(loss, retain_graph=True)
        grad = torch.full((B, T, C), SENTINEL, device="cuda:0")
        ems.grads_to_device(grad, off)
        gtn.synchronize()
        grads.append(grad.cpu().numpy())
    _check("retained first pass", loss.items(), grads[0], frames, ref)
    for b, f in enumerate(frames):
        assert not grads[1][b, f:].any(), b
        assert np.isfinite(grads[1][b, :f]).all(), b
    assert not np.array_equal(grads[0], grads[1])  # (the second pass accumulated)


def test_alignment_takes_the_rows(gtn):
    """viterbi_align without frames on a chain that carries rows is viterbi_align(frames=rows) on the plain chain;
    frames beyond the rows are an error"""
    import torch
    em, em_nan, targets, frames, _ = _case(BASE)
    B, T, C = em.shape
    out = []
    for rows, fr, e in ((frames, None, em_nan), (None, frames, em)):
        ctcs = gtn.Batch.ctc_targets(targets, 0, False)
        em_dev = _dev(e)  # (borrowed by `ems`: held while it is in use)
        ems = gtn.Batch.linear(B, T, C, em_dev, False, True, rows=rows)
        labels = torch.full((B, T), -7, dtype=torch.int32, device="cuda:0")
        tokens = torch.full((B, T), -7, dtype=torch.int32, device="cuda:0")
        scores = torch.full((B,), SENTINEL, device="cuda:0")
        gtn.intersect(ctcs, ems).viterbi_align(labels, tokens, scores, fr)
        gtn.synchronize()
        out.append((labels.cpu().numpy(), tokens.cpu().numpy(), scores.cpu().numpy()))
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    assert np.isfinite(out[0][2]).all()
    for b, f in enumerate(frames):
        assert (out[0][0][b, :f] >= 0).all() and (out[0][0][b, f:] == -1).all()
    ctcs = gtn.Batch.ctc_targets(targets, 0, False)
    em_dev = _dev(em)
    ems = gtn.Batch.linear(B, T, C, em_dev, False, True, rows=frames)
    too_long = frames.copy()
    too_long[1] += 1
    labels = torch.full((B, T), -7, dtype=torch.int32, device="cuda:0")
    with pytest.raises(ValueError):
        gtn.intersect(ctcs, ems).viterbi_align(labels, None, None, too_long)
    gtn.synchronize()
    assert (labels == -7).all().item()


def test_argument_errors(gtn):
    """input_lengths of the wrong length, a count of 0 and a count of T + 1: ValueError from the torch entry and from
    Batch.linear, an error status from the C symbol -- and nothing is written"""
    import torch
    import gtn_amd.torch_loss as tl
    em, _, targets, frames, _ = _case(BASE)
    B, T, C = em.shape
    em_dev = _dev(em)
    bad = [list(frames[:-1]), [0] + list(frames[1:]), list(frames[:-1]) + [T + 1]]
    gtn.prof_reset()
    gtn.prof_enable(True)
    for native in (True, False):
        tl._NATIVE = None if native else False
        for lens in bad:
            lp = em_dev.clone().requires_grad_(True)
            with pytest.raises(ValueError):
                tl.ctc_loss(lp, targets, input_lengths=lens)
            with pytest.raises(ValueError):
                tl.ctc_loss(lp, targets, input_lengths=torch.tensor(lens))
    tl._NATIVE = None
    for lens in bad:
        with pytest.raises(ValueError):
            gtn.Batch.linear(B, T, C, em_dev, True, True, rows=lens)
    gtn.prof_enable(False)
    assert gtn.prof_names() == []
    lib = tl._native()
    assert lib and hasattr(lib, "gtn_ctc_loss_frames_n")
    flat, lens = tl._flat_targets(targets)
    for fr in bad[1:]:
        fr = np.asarray(fr, np.int32)
        loss = torch.full((B,), SENTINEL, device="cuda:0")
        grad = torch.full((B, T, C), SENTINEL, device="cuda:0")
        rc = lib.gtn_ctc_loss_frames_n(em_dev.data_ptr(), flat.ctypes.data, lens.ctypes.data, B, T, C, 0, fr.ctypes.data,
                                       loss.data_ptr(), grad.data_ptr())
        assert rc != 0 and "frame count" in lib.gtn_criteria_last_error().decode()
        gtn.synchronize()
        assert (loss == SENTINEL).all().item() and (grad == SENTINEL).all().item()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == _CHILD:
        _no_band_child(sys.argv[2])
