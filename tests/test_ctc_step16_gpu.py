"""The CTC step on bfloat16 / float16 emissions (gtn_amd/csrc/ctc_step16.hip) against float64 on the very numbers the
kernel sees: 16-bit inputs are exactly representable, so tests/ctc_fp64.py on em16.double()[:T_b] is the yardstick.
Gates: loss 1e-4 relative, float32-output gradient 1e-4 absolute; the 16-bit gradient is torch's round-to-nearest of
the float32 one, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from ctc_fp64 import ctc_loss_fp64

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
RING = 8  # the kernel's K-row block (kCtcStep16Ring)


def make(seed, B, T, C_, U, dtype):
    """emissions [B, T, C] of `dtype` on the device and B targets of U labels without equal neighbours (feasible in U frames)"""
    rng = np.random.default_rng(seed)
    em = torch.from_numpy((2.0 * rng.standard_normal((B, T, C_))).astype(np.float32)).to("cuda", dtype)
    tg = []
    for _ in range(B):
        t = rng.integers(1, C_, size=U)
        for i in range(1, U):
            if t[i] == t[i - 1]:
                t[i] = 1 + t[i] % (C_ - 1)
        tg.append(t.tolist())
    return em, tg


def step(gtn, em, tg, frames=None, grad32=False):
    loss = torch.full((em.shape[0],), 7.0, dtype=torch.float32, device=em.device)
    grad = torch.full(em.shape, 7.0, dtype=torch.float32 if grad32 else em.dtype, device=em.device)
    torch.cuda.synchronize()  # (the call runs on the engine's stream: the emissions and the guard fills come first)
    gtn.ctc_loss_step16(em, tg, loss, grad, input_lengths=frames)
    gtn.synchronize()
    return loss, grad


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


def check(gtn, em, tg, frames=None):
    """both instantiations of one batch against float64 and against each other; returns (loss, 16-bit gradient)"""
    loss, g32 = step(gtn, em, tg, frames, grad32=True)
    loss16, g16 = step(gtn, em, tg, frames)
    assert torch.equal(bits(loss), bits(loss16))
    assert torch.equal(bits(g16), bits(g32.to(em.dtype)))
    em64, got, g = em.double().cpu().numpy(), loss.cpu().numpy(), g32.cpu().numpy()
    for b in range(em.shape[0]):
        Tb = em.shape[1] if frames is None else int(frames[b])
        want, wgrad, _ = ctc_loss_fp64(em64[b, :Tb], tg[b])
        assert not g[b, Tb:].any(), b
        if np.isfinite(want):
            assert abs(got[b] - want) <= 1e-4 * max(1.0, abs(want)), (b, got[b], want)
            assert np.abs(g[b, :Tb] - wgrad).max() <= 1e-4, b
        else:
            assert got[b] == np.inf and not g[b].any(), b
    return loss, g16


# C: one piece, not a power of two, a second piece per streamer lane (264, 520); U: wave and lane-ownership edges and the
# cap; T: 1, around the ring, else what the target needs
CASES = [(8, 0, 1), (8, 1, 1), (24, 1, RING - 1), (24, 0, RING), (24, 1, RING + 1), (264, 31, 33), (264, 32, 40),
         (24, 127, 130), (520, 128, 131), (8, 511, 513), (520, 31, 31)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C_,U,T", CASES)
def test_values(gtn, dtype, C_, U, T):
    em, tg = make(C_ + U + T, 2, T, C_, U, dtype)
    check(gtn, em, tg)


@pytest.mark.parametrize("dtype", DTYPES)
def test_repeated_label_at_its_shortest_length(gtn, dtype):
    em, _ = make(3, 2, 9, 24, 0, dtype)
    check(gtn, em, [[3] * 5, [3] * 5])  # (no skip arcs: 5 labels and 4 blanks between them)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ragged_batch_and_pad_rows(gtn, dtype):
    em, tg = make(5, 3, 12, 24, 4, dtype)
    tg[0], frames = tg[0][:1], [1, 4, 12]
    loss, g = check(gtn, em, tg, frames)
    for b, Tb in enumerate(frames):
        em[b, Tb:] = float("nan")
    loss2, g2 = step(gtn, em, tg, frames)
    assert torch.equal(bits(loss), bits(loss2)) and torch.equal(bits(g), bits(g2))


@pytest.mark.parametrize("dtype", DTYPES)
def test_infeasible_neighbour_and_minus_inf(gtn, dtype):
    em, tg = make(9, 3, 10, 24, 3, dtype)
    free = next(c for c in range(1, 24) if all(c not in t for t in tg))
    em[:, :, free] = float("-inf")       # a column nothing aligns through
    em[0, 2, tg[0][1]] = float("-inf")   # a cell that takes the alignments through it away
    tg[1] = [2, 2, 2, 2, 2, 2, 2]        # 13 frames at least
    loss, g = check(gtn, em, tg)
    assert loss[1].item() == float("inf") and not g[1].any()
    keep = [0, 2]
    loss2, g2 = step(gtn, em[keep].contiguous(), [tg[b] for b in keep])
    assert torch.equal(bits(loss[keep]), bits(loss2)) and torch.equal(bits(g[keep]), bits(g2))


def test_sliced_call_is_the_unsliced_bits(gtn):
    """B = 80, T = 1000, U = 511: the alpha planes are above 256 MiB, so the call runs as two launches"""
    em, tg = make(11, 80, 1000, 8, 511, torch.bfloat16)
    gtn.prof_reset()
    gtn.prof_enable(True)
    loss, g = step(gtn, em, tg)
    launches = gtn.prof_get("ctc_step16")["launches"]
    gtn.prof_enable(False)
    assert launches == 2 and torch.isfinite(loss).all()
    for lo in (0, 40):
        l2, g2 = step(gtn, em[lo:lo + 40].contiguous(), tg[lo:lo + 40])
        assert torch.equal(bits(loss[lo:lo + 40]), bits(l2)) and torch.equal(bits(g[lo:lo + 40]), bits(g2))
    l3, g3 = step(gtn, em, tg)
    assert torch.equal(bits(loss), bits(l3)) and torch.equal(bits(g), bits(g3))


@pytest.mark.parametrize("what", ["same_bits", "cast_route", "float32_untouched", "refusals"])
def test_entry_points(gtn, what):
    import gtn_amd.torch_loss as tl
    lib = tl._native()
    assert lib and hasattr(lib, "gtn_ctc_loss16_n"), "libgtn_criteria.so (build())"
    em, tg = make(13, 3, 20, 24, 5, torch.bfloat16)
    frames = [20, 7, 13]
    flat, lens = tl._flat_targets(tg)
    fr = np.asarray(frames, np.int32)
    if what == "same_bits":
        loss, g = step(gtn, em, tg, frames)
        loss2, g2 = torch.empty_like(loss), torch.empty_like(g)
        torch.cuda.synchronize()
        assert lib.gtn_ctc_loss16_n(em.data_ptr(), 2, flat.ctypes.data, lens.ctypes.data, 3, 20, 24, 0, fr.ctypes.data,
                                    loss2.data_ptr(), g2.data_ptr(), 2) == 0, lib.gtn_criteria_last_error()
        gtn.synchronize()
        x = em.clone().requires_grad_(True)
        loss3 = tl.ctc_loss(x, tg, input_lengths=frames)
        loss3.backward(torch.ones_like(loss3))
        assert loss3.dtype == torch.float32 and x.grad.dtype == torch.bfloat16
        for l, gg in ((loss2, g2), (loss3.detach(), x.grad)):
            assert torch.equal(bits(loss), bits(l)) and torch.equal(bits(g), bits(gg))
    elif what == "cast_route":
        em, tg = make(17, 3, 10, 12, 3, torch.bfloat16)  # C = 12: no 16-byte pieces
        tg[1] = [2] * 7
        x = em.clone().requires_grad_(True)
        loss = tl.ctc_loss(x, tg)
        loss.backward(torch.ones_like(loss))
        assert x.grad.dtype == torch.bfloat16 and loss[1].item() == float("inf") and not x.grad[1].any()
        for b in (0, 2):
            want, wgrad, _ = ctc_loss_fp64(em[b].double().cpu().numpy(), tg[b])
            assert abs(loss[b].item() - want) <= 1e-4 * max(1.0, abs(want))
            assert np.abs(x.grad[b].float().cpu().numpy() - wgrad).max() <= 1e-4 + 2.0 ** -9  # (+ half a bfloat16 ulp below 1)
    elif what == "float32_untouched":
        def never(*a):
            raise AssertionError("a float32 call reached the 16-bit step")
        real = lib.gtn_ctc_loss16_n
        try:
            lib.gtn_ctc_loss16_n = never
            x = em.float().requires_grad_(True)
            tl.ctc_loss(x, tg, input_lengths=frames).sum().backward()
            assert x.grad.dtype == torch.float32
        finally:
            lib.gtn_ctc_loss16_n = real
    else:
        call = gtn._lib.gtnx_batch_ctc_loss_step16
        loss, g = torch.full((3,), 7.0, device="cuda"), torch.full_like(em, 7.0)
        zero = np.asarray([20, 0, 13], np.int32)
        good = [em.data_ptr(), 2, flat.ctypes.data, lens.ctypes.data, fr.ctypes.data, 3, 20, 24, 0, loss.data_ptr(),
                g.data_ptr(), 2]
        torch.cuda.synchronize()
        for i, v in ((1, 3), (1, 0), (11, 1), (0, em.data_ptr() + 2), (10, g.data_ptr() + 8), (4, zero.ctypes.data)):
            a = list(good)
            a[i] = v
            assert call(*a) == 1, (i, v)
        gtn.synchronize()
        assert (loss == 7.0).all() and (g == 7.0).all()
