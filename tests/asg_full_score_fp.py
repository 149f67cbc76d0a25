"""The cases of tests/test_asg_full_score_*.py and their float64 yardstick (TEST INFRASTRUCTURE ONLY): tests/ctc_fp64.py's
asg_fp64 on em[b, :T_b], looped over the batch with the weights applied.  Inputs as in tests/test_asg_frames_gpu.py:
log-softmaxed normal emissions at scale 1, normal transitions and start scores."""
import functools

import numpy as np

from ctc_fp64 import asg_fp64

# (B, T, C): the alphabet edges (tile 32, the old limit 128, the GEMM block 128 / 256 and its padding, the cap) ...
ALPHABETS = [(3, 1, 1), (4, 9, 1), (4, 9, 31), (4, 2, 32), (4, 9, 33), (4, 9, 128), (4, 9, 129), (4, 2, 256), (4, 9, 257),
             (4, 9, 1000), (4, 9, 1024)]
# ... the group edges (one below, at and above the largest group of 16; past two split-K blocks of 16) ...
GROUPS = [(15, 5, 33), (16, 5, 33), (17, 5, 33), (35, 5, 33)]
# ... and a long utterance beside a one-frame neighbour
LONG = [(2, 70, 129)]
SHAPES = ALPHABETS + GROUPS + LONG


def frames_of(B, T, rng):
    """ragged counts that hold M, 0 and 1 (the long case: M beside 1)"""
    fr = [T, 1] if B == 2 else [T, 0, 1] + rng.integers(1, T + 1, B - 3).tolist()
    return np.asarray(fr, np.int32)


@functools.lru_cache(maxsize=None)
def case(shape):
    """(em [B, T, C], trans [C, C], start [C], frames [B], weights [B], scores [B] float64, weighted d em [B, T, C],
    weighted d table [C + C * C]); the weights hold a negative one and, past three utterances, a zero"""
    B, T, C = shape
    rng = np.random.default_rng(4100 + 7 * C + T + B)
    em = rng.normal(0, 1, (B, T, C))
    em = (em - np.log(np.exp(em).sum(-1, keepdims=True))).astype(np.float32)
    trans = rng.normal(0, 1, (C, C)).astype(np.float32)
    start = rng.normal(0, 1, C).astype(np.float32)
    frames = frames_of(B, T, rng)
    w = np.linspace(0.5, 1.5, B).astype(np.float32)
    w[0] = -0.75
    if B > 3:
        w[2] = 0.0  # (the one-frame utterance: the ragged ones keep their share of the table gradient)
    out = (em, trans, start, frames, w) + reference(em, trans, start, frames, w)
    for a in out:
        a.setflags(write=False)
    return out


def reference(em, trans, start, frames, w):
    B, T, C = em.shape
    tw = np.concatenate([start, trans.reshape(-1)])
    Z, g_em, g_tab = np.full(B, -np.inf), np.zeros((B, T, C)), np.zeros(C + C * C)
    for b, f in enumerate(frames):
        if f > 0:
            Z[b], ge, gt = asg_fp64(em[b, :f], tw)[:3]
            if np.isfinite(Z[b]):
                g_em[b, :f] = w[b] * ge
                g_tab += w[b] * gt
    return Z, g_em, g_tab


def check(tag, scores, g_em, g_tab, want, frames, part=1.0):
    """the project's gates (tests/test_asg_frames_gpu.py), times `part`; figures printed before they are judged"""
    Z, w_em, w_tab = want
    for b, f in enumerate(frames):
        if np.isfinite(Z[b]):
            err = abs(float(scores[b]) - Z[b])
            print(f"{tag} b={b} T_b={f} score {scores[b]:.6f} want {Z[b]:.6f} err {err:.2e}")
            assert err <= part * 1e-4 * max(1.0, abs(Z[b])), (tag, b, err)
        else:
            assert scores[b] == -np.inf, (tag, b, scores[b])
        if g_em is not None:
            assert not g_em[b, f:].any(), (tag, b, "pad rows of the gradient are not 0")
            err = np.abs(g_em[b, :f] - w_em[b, :f]).max() if f else 0.0
            print(f"{tag} b={b} em grad abs {err:.2e}")
            assert np.isfinite(g_em[b]).all() and err <= part * 1e-4, (tag, b, err)
    if g_tab is not None:
        print(f"{tag} table grad abs {np.abs(g_tab - w_tab).max():.2e} of max {np.abs(w_tab).max():.3f}")
        np.testing.assert_allclose(g_tab, w_tab, rtol=part * 1e-3, atol=part * 1e-4)
