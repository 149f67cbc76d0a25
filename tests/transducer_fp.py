"""The yardstick of the batched transducer (RNN-T) score (gtnx_batch_transducer_score), on the host:
the recurrences of the contract in float64 numpy, the seeded cases tests/test_transducer_cpu.py and
tests/test_transducer_gpu.py share, and the gates (tests/asg_full_score_fp.py's: score 1e-4 max(1, |want|), gradient
1e-4 absolute, never-read rows == 0).

Float32 stays inside the gates only while |score| <= 100 (the note in tests/ctc_score_fp.py), so the cases peak the
logits: 3 + ln C on the blank and on the target's label at every node; where U > 100, 8 + ln C on the label and ln C on
the blank.  Unpeaked normal logits break the gradient gate from about T + U = 260 on and are used at (5, 4, 4) only."""
import functools
import math

import numpy as np

# (T, U, C, peaked): lane / K edges and skew fill and drain; degenerate; the row paths.  Batches of 4 (C > 4096: 2)
SHAPES = [(65, 63, 5), (64, 64, 5), (63, 128, 5), (70, 129, 8), (3, 512, 2), (3, 1023, 2), (129, 1, 4),
          (1, 0, 1), (1, 5, 4), (2, 1, 3), (5, 4, 4),
          (3, 2, 255), (3, 2, 256), (3, 2, 257), (64, 63, 257), (3, 2, 4096), (3, 2, 4100), (3, 2, 4101)]
CASES = [s + (True,) for s in SHAPES] + [(5, 4, 4, False)]
WEIGHTS = np.asarray([1.25, -0.75, 0.0, 0.5], np.float32)


def reference(x, targets, frames, tlens, blank, normalize, w):
    """(scores [B], grad [B, T, U + 1, C]) in float64; -inf and a zero gradient where the contract says so"""
    B, T, U1, C = x.shape
    scores, grad = np.full(B, -np.inf), np.zeros(x.shape)
    for b in range(B):
        Tb, Ub = int(frames[b]), int(tlens[b])
        y = [int(v) for v in targets[b, :max(Ub, 0)]]
        if not (1 <= Tb <= T and 0 <= Ub < U1) or any(not 0 <= v < C or v == blank for v in y):
            continue
        xs = x[b, :Tb, :Ub + 1].astype(np.float64)
        with np.errstate(invalid="ignore"):
            lse = np.logaddexp.reduce(xs, axis=2) if normalize else np.zeros(xs.shape[:2])
        dead = ~np.isfinite(lse) | (np.isnan(xs) | (xs == np.inf)).any(axis=2)
        lse = np.where(dead, 0.0, lse)
        lpb = np.where(dead, -np.inf, xs[:, :, blank] - lse)
        lpl = np.full((Tb, Ub + 1), -np.inf)
        for u, v in enumerate(y):
            lpl[:, u] = np.where(dead[:, u], -np.inf, xs[:, u, v] - lse[:, u])
        al, be = np.full((Tb, Ub + 1), -np.inf), np.full((Tb + 1, Ub + 2), -np.inf)
        for t in range(Tb):
            for u in range(Ub + 1):
                up = al[t - 1, u] + lpb[t - 1, u] if t else (0.0 if u == 0 else -np.inf)
                left = al[t, u - 1] + lpl[t, u - 1] if u else -np.inf
                al[t, u] = np.logaddexp(up, left)
        be[Tb, Ub] = 0.0  # (the virtual end)
        for t in range(Tb - 1, -1, -1):
            for u in range(Ub, -1, -1):
                be[t, u] = np.logaddexp(be[t + 1, u] + lpb[t, u], be[t, u + 1] + lpl[t, u])
        sc = al[Tb - 1, Ub] + lpb[Tb - 1, Ub]
        if not np.isfinite(sc):
            continue
        scores[b] = sc
        ob = np.exp(al + lpb + be[1:, :-1] - sc)
        ol = np.exp(al + lpl + be[:-1, 1:] - sc)
        g = grad[b, :Tb, :Ub + 1]
        if normalize:
            with np.errstate(invalid="ignore"):
                g -= np.where(dead[:, :, None], 0.0, np.exp(xs - lse[:, :, None]) * (ob + ol)[:, :, None])
        g[:, :, blank] += ob
        for u, v in enumerate(y):
            g[:, u, v] += ol[:, u]
        g *= float(w[b])
    return scores, grad


@functools.lru_cache(maxsize=None)
def case(T, U, C, peaked, normalize):
    """(x, targets, frames, tlens, blank, w, want scores, want grad) of a seeded case, read-only"""
    B = 2 if C > 4096 else 4
    rng = np.random.default_rng(1000 * T + 10 * U + C)
    blank = C // 2
    x = rng.standard_normal((B, T, U + 1, C))
    targets = np.zeros((B, U), np.int32)
    if U:
        targets[:] = (blank + 1 + rng.integers(0, C - 1, (B, U))) % C
    if peaked:
        boost_b, boost_l = (math.log(C), 8 + math.log(C)) if U > 100 else (3 + math.log(C),) * 2
        x[:, :, :, blank] += boost_b
        for u in range(U):
            x[np.arange(B), :, u, targets[:, u]] += boost_l
    x = x.astype(np.float32)
    if not normalize:  # (the float32 log-softmax of the same logits)
        x64 = x.astype(np.float64)
        x = (x64 - np.logaddexp.reduce(x64, axis=3, keepdims=True)).astype(np.float32)
    # the full value; a random value; one frame and no label; no frame
    frames = np.asarray([T, rng.integers(1, T + 1), 1, 0], np.int32)[:B]
    tlens = np.asarray([U, rng.integers(0, U + 1), 0, rng.integers(0, U + 1)], np.int32)[:B]
    w = WEIGHTS[:B]
    out = (x, targets, frames, tlens, blank, w) + reference(x, targets, frames, tlens, blank, normalize, w)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def check(name, scores, grad, want_scores, want_grad, frames, tlens, part=1.0):
    """the gates; `part` scales them (a transcription is asked to stay within a share of them)"""
    assert not np.isnan(scores).any() and not np.isnan(grad).any(), name
    for b, (got, want) in enumerate(zip(scores, want_scores)):
        print(f"{name} b={b} score {got!r} want {want!r}")
        assert got == want if np.isinf(want) else abs(got - want) <= part * 1e-4 * max(1.0, abs(want)), (name, b, got, want)
    print(f"{name} worst gradient error {np.abs(grad - want_grad).max():.3g}")
    assert np.abs(grad - want_grad).max() <= part * 1e-4, name
    for b in range(len(scores)):
        Tb, Ub = int(frames[b]), int(tlens[b])
        live = 0 <= Tb <= grad.shape[1] and 0 <= Ub < grad.shape[2]
        assert not grad[b, Tb if live else 0:].any() and not grad[b, :, Ub + 1 if live else 0:].any(), (name, b)
