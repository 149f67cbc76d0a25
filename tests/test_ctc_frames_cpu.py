"""CTC loss over padded batches, the parts that need no GPU.

What "frames" means for the yardstick of tests/test_ctc_frames_gpu.py: ctc_loss_fp64 (tests/ctc_fp64.py) on the first
T_b rows of an utterance is torch.nn.functional.ctc_loss(..., input_lengths) in float64 on log-softmax inputs (where
the loss's own normaliser forwardScore(emissions) is 0) -- and the argument checks of gtnx_batch_linear_rows, which
come before the engine looks for a device.
"""
import ctypes as C

import numpy as np
import pytest

from ctc_align_fp import min_frames, seeded_case
from ctc_fp64 import ctc_loss_fp64

# (seed, B, T, C, Umax) of seeded_case(..., True), frames[0] set to T: a full-length utterance beside padded ones
SEEDED = [(11, 4, 60, 12, 7), (12, 4, 60, 9, 7), (13, 3, 200, 64, 40), (15, 2, 33, 300, 5), (16, 5, 130, 32, 20)]
CASES = SEEDED + ["tight"]


def frames_case(key):
    """(em float32 [B, T, C], targets, frames int32 [B]) of one case; every utterance is feasible in its frame count"""
    if key == "tight":
        # a 281-node target (eight nodes per lane) at full length beside one at its shortest feasible frame count
        rng = np.random.default_rng(17)
        B, T, Cn = 2, 300, 20
        em = rng.normal(0, 2, (B, T, Cn)).astype(np.float32)
        targets = [rng.integers(1, 20, 140).tolist(), rng.integers(1, 20, 100).tolist()]
        frames = np.asarray([T, min_frames(targets[1])], np.int32)
    else:
        seed, B, T, Cn, Umax = key
        em, targets, frames = seeded_case(seed, B, T, Cn, Umax, True)
        frames = frames.copy()
        frames[0] = T
    for t, f in zip(targets, frames):
        assert min_frames(t) <= f <= em.shape[1]
    return em, targets, frames


@pytest.mark.parametrize("key", CASES, ids=str)
def test_fp64_yardstick_on_slices_is_torch_ctc_with_input_lengths(key):
    import torch
    em, targets, frames = frames_case(key)
    B, T, Cn = em.shape
    if key == (15, 2, 33, 300, 5):
        assert frames.tolist() == [33, 8]
    if key == (16, 5, 130, 32, 20):  # (around multiples of the sweeps' row blocks and shift periods)
        assert frames.tolist() == [130, 63, 106, 122, 62]
    lp = torch.log_softmax(torch.from_numpy(em).double(), -1).requires_grad_(True)
    flat = torch.tensor([x for t in targets for x in t], dtype=torch.long)
    want = torch.nn.functional.ctc_loss(lp.transpose(0, 1), flat, torch.tensor(frames.tolist()),
                                        torch.tensor([len(t) for t in targets]), blank=0, reduction="none",
                                        zero_infinity=False)
    want.sum().backward()
    lpn = lp.detach().numpy()
    for b in range(B):
        f = int(frames[b])
        loss, grad, _ = ctc_loss_fp64(lpn[b, :f], targets[b])
        assert np.isfinite(loss)
        np.testing.assert_allclose(loss, want[b].item(), rtol=1e-9)
        # (torch's CTC gradient w.r.t. log-probabilities carries the softmax term of a preceding log_softmax,
        #  exp(lp) - posteriors: on normalised rows that is the yardstick's d forwardScore(emissions) - posteriors)
        np.testing.assert_allclose(grad, lp.grad[b, :f].numpy(), rtol=1e-7, atol=1e-12)
        assert not lp.grad[b, f:].any()


def test_linear_rows_arguments_are_checked_before_the_device():
    """gtnx_batch_linear_rows: a row count outside 1 .. M is GTNX_INVALID_ARGUMENT (ValueError) whatever the machine --
    the check comes before the engine asks for a device, and no batch is handed back"""
    import gtn_amd
    lib = gtn_amd._lib
    for rows in ([3, 0], [5, 2], [-1, 1], [1, 4 + 1]):
        r = np.asarray(rows, np.int32)
        h = C.c_void_p()
        rc = lib.gtnx_batch_linear_rows(2, 4, 3, r.ctypes.data, 0, None, 0, C.byref(h))
        assert rc != 0 and not h.value, rows
        with pytest.raises(ValueError, match="row count"):
            gtn_amd._api.check(rc)
    with pytest.raises(ValueError, match="row counts for a batch"):
        gtn_amd.Batch.linear(2, 4, 3, 0, False, False, rows=[1, 2, 3])
