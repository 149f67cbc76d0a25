"""The yardstick of the batched token-and-duration transducer (TDT) score (gtnx_batch_transducer_tdt_score, DESIGN
section 47), on the host: the recurrences of the contract and the closed-form gradient in float64 numpy, the seeded cases
tests/test_transducer_tdt_cpu.py and tests/test_transducer_tdt_gpu.py share, and the gates of tests/transducer_fp.py
(score 1e-4 max(1, |want|), gradient 1e-4 absolute, never-read rows == 0, no NaN).

Float32 stays inside the gates only while |score| <= 100, which `case` asserts.  The tokens are peaked as
transducer_fp.case peaks them; the duration logits are left as they are, except where U > 4 T -- there most labels must
take duration 0 and 8 + ln D is added to it."""
import functools
import math

import numpy as np

from transducer_fp import WEIGHTS, check  # noqa: F401  (the gates are the classical transducer's)

# (T, U, C, D): lane / K edges U + 1 = 64 / 65 / 130 / 513 / 1024; D = 2 and 8, T < D, U = 0; a segment boundary inside a
# vector; rows of 256 / 257 / 4096 / 4100 / 4101 entries.  Batches of 4 (C + D > 4096: 2)
SHAPES = [(65, 63, 5, 5), (64, 64, 5, 5), (70, 129, 8, 4), (3, 512, 2, 2), (3, 1023, 2, 2), (129, 1, 4, 8),
          (1, 0, 1, 2), (2, 1, 3, 5), (1, 5, 4, 8), (5, 4, 4, 3), (64, 63, 252, 5), (3, 2, 4091, 5), (3, 2, 4096, 5),
          (3, 2, 251, 5), (3, 2, 252, 4), (3, 2, 4095, 5),
          (3, 2, 1024, 4), (3, 2, 1025, 5)]  # (rows just above a power of two: the ladder's in-between rungs)


def _scan(base, step, reverse):
    """out[u] = logaddexp(base[u], out[u -/+ 1] + step[u -/+ 1 or u]): the d = 0 label arcs inside one frame"""
    out, prev = np.empty_like(base), -np.inf
    for u in (range(len(base) - 1, -1, -1) if reverse else range(len(base))):
        out[u] = prev = np.logaddexp(base[u], prev + step[u] if reverse else prev)
        if not reverse:
            prev = prev + step[u]
    return out


def reference(x, targets, frames, tlens, C, blank, sigma, w):
    """(scores [B], grad [B, T, U + 1, C + D]) in float64; -inf and a zero gradient where the contract says so"""
    B, T, U1, CD = x.shape
    D = CD - C
    scores, grad = np.full(B, -np.inf), np.zeros(x.shape)
    for b in range(B):
        Tb, Ub = int(frames[b]), int(tlens[b])
        y = [int(v) for v in targets[b, :max(Ub, 0)]]
        if not (1 <= Tb <= T and 0 <= Ub < U1) or any(not 0 <= v < C or v == blank for v in y):
            continue
        xs = x[b, :Tb, :Ub + 1].astype(np.float64)
        with np.errstate(invalid="ignore"):
            lse_t, lse_d = np.logaddexp.reduce(xs[:, :, :C], axis=2), np.logaddexp.reduce(xs[:, :, C:], axis=2)
        dead = ~np.isfinite(lse_t) | ~np.isfinite(lse_d) | (np.isnan(xs) | (xs == np.inf)).any(axis=2)
        lse_t, lse_d = np.where(dead, 0.0, lse_t), np.where(dead, 0.0, lse_d)
        ld = np.where(dead[:, :, None], -np.inf, xs[:, :, C:] - lse_d[:, :, None])
        lpb = np.where(dead, -np.inf, xs[:, :, blank] - lse_t - sigma)
        lpl = np.full((Tb, Ub + 1), -np.inf)
        for u, v in enumerate(y):
            lpl[:, u] = np.where(dead[:, u], -np.inf, xs[:, u, v] - lse_t[:, u] - sigma)
        wb, wl = lpb[:, :, None] + ld, lpl[:, :, None] + ld  # arc weights [Tb, Ub + 1, D]
        wb[:, :, 0] = -np.inf                                # (no blank of duration 0)
        minus = np.full(1, -np.inf)
        al = np.full((Tb, Ub + 1), -np.inf)
        for t in range(Tb):
            terms = [np.where(np.arange(Ub + 1) == 0, 0.0 if t == 0 else -np.inf, -np.inf)]
            for d in range(1, min(D - 1, t) + 1):
                terms += [al[t - d] + wb[t - d, :, d], np.concatenate([minus, (al[t - d] + wl[t - d, :, d])[:-1]])]
            al[t] = _scan(np.logaddexp.reduce(terms, axis=0), wl[t, :, 0], False)
        be = np.full((Tb, Ub + 2), -np.inf)  # (column U_b + 1: nothing)
        end = np.where(np.arange(Ub + 1) == Ub, 0.0, -np.inf)  # the virtual end, reached by blank arcs only
        # tb[t][d] / tl[t][d]: beta of the node a blank / label arc of duration d out of row t lands on, per column
        tb = [[be[t + d, :-1] if t + d < Tb else (end if t + d == Tb else end - np.inf) for d in range(D)]
              for t in range(Tb)]
        tl = [[be[t + d, 1:] if t + d < Tb else end - np.inf for d in range(D)] for t in range(Tb)]
        for t in range(Tb - 1, -1, -1):
            terms = [wb[t, :, d] + tb[t][d] for d in range(1, D)] + [wl[t, :, d] + tl[t][d] for d in range(1, D)]
            be[t, :-1] = _scan(np.logaddexp.reduce(terms, axis=0), wl[t, :, 0], True)
        sc = np.logaddexp.reduce([al[Tb - d, Ub] + wb[Tb - d, Ub, d] for d in range(1, min(D - 1, Tb) + 1)])
        if not np.isfinite(sc):
            continue
        scores[b] = sc
        ob = np.stack([np.stack([np.exp(al[t] + wb[t, :, d] + tb[t][d] - sc) for d in range(D)], -1) for t in range(Tb)])
        ol = np.stack([np.stack([np.exp(al[t] + wl[t, :, d] + tl[t][d] - sc) for d in range(D)], -1) for t in range(Tb)])
        OB, OL = ob.sum(axis=2), ol.sum(axis=2)
        g = grad[b, :Tb, :Ub + 1]
        with np.errstate(invalid="ignore"):
            g[:, :, :C] -= np.where(dead[:, :, None], 0.0, np.exp(xs[:, :, :C] - lse_t[:, :, None]) * (OB + OL)[:, :, None])
        g[:, :, blank] += OB
        for u, v in enumerate(y):
            g[:, u, v] += OL[:, u]
        g[:, :, C:] = ob + ol - np.exp(ld) * (OB + OL)[:, :, None]
        g *= float(w[b])
    return scores, grad


@functools.lru_cache(maxsize=None)
def case(T, U, C, D, sigma=0.0):
    """(x, targets, frames, tlens, blank, w, want scores, want grad) of a seeded case, read-only"""
    B = 2 if C + D > 4096 else 4
    rng = np.random.default_rng(1000 * T + 10 * U + C + 7 * D)
    blank = C // 2
    x = rng.standard_normal((B, T, U + 1, C + D))
    targets = np.zeros((B, U), np.int32)
    if U:
        targets[:] = (blank + 1 + rng.integers(0, C - 1, (B, U))) % C
    boost_b, boost_l = (math.log(C), 8 + math.log(C)) if U > 100 else (3 + math.log(C),) * 2
    x[:, :, :, blank] += boost_b
    for u in range(U):
        x[np.arange(B), :, u, targets[:, u]] += boost_l
    if U > 4 * T:
        x[:, :, :, C] += 8 + math.log(D)
    x = x.astype(np.float32)
    # the full value; a random value; one frame and no label; no frame
    frames = np.asarray([T, rng.integers(1, T + 1), 1, 0], np.int32)[:B]
    tlens = np.asarray([U, rng.integers(0, U + 1), 0, rng.integers(0, U + 1)], np.int32)[:B]
    w = WEIGHTS[:B]
    out = (x, targets, frames, tlens, blank, w) + reference(x, targets, frames, tlens, C, blank, sigma, w)
    assert all(abs(s) <= 100 for s in out[6] if np.isfinite(s)), out[6]  # (the stated domain of the float32 gates)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
