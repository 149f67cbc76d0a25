"""The yardstick of the pruned (banded) transducer score (gtnx_batch_transducer_pruned_score), on the
host: the band is scattered into a full [B, T, U + 1, C] tensor whose other rows hold -inf -- rows the dense float64
recurrences of tests/transducer_fp.py treat as nodes no path leaves, which is the full lattice with the nodes outside
the band removed -- and the gradient is gathered back.  What the contract adds by fiat comes on top: ranges that
decrease before T_b score -inf.  The seeded cases are shared by the CPU and GPU tests; the gates are that file's."""
import functools
import itertools
import math

import numpy as np

import transducer_fp as fp

B = 9  # (at S = 5 one wave carries eight utterances of different lengths and a second wave one)
# (T, U, S, C, plane): S = 1, 2, 5, a full group, a group plus one, 33, a whole wave; S = U + 1 under zero ranges; T = 1;
# U = 0; a wide row that is no multiple of 4; rows above 4096 labels
SHAPES = [(6, 2, 1, 5), (10, 6, 2, 5), (24, 12, 5, 6), (14, 20, 8, 4), (14, 20, 9, 4), (12, 60, 33, 3), (10, 70, 64, 3),
          (1, 3, 4, 5), (5, 0, 1, 3), (3, 2, 2, 257), (3, 2, 2, 4100)]
CASES = [s + (p,) for s in SHAPES for p in ("mixed", "flat")] + [(7, 4, 5, 6, "zero")]
WEIGHTS = np.asarray([1.25, -0.75, 0.0, 0.5, 1.0, -1.5, 2.0, 0.25, -0.5], np.float32)


def scatter(x, ranges, U):
    """the band [B, T, S, C] in a full [B, T, U + 1, C] float64 tensor of -inf, and the (b, t, s) -> u map (-1: none)"""
    Bn, T, S, C = x.shape
    r = np.asarray(ranges, np.int64)[:, :, None]
    u = np.where((r >= 0) & (r <= U) & (r + np.arange(S) <= U), r + np.arange(S), -1)
    full = np.full((Bn, T, U + 1, C), -np.inf)
    b, t, s = np.nonzero(u >= 0)
    full[b, t, u[b, t, s]] = x[b, t, s]
    return full, u


def reference(x, ranges, targets, frames, tlens, blank, normalize, w):
    """(scores [B], grad [B, T, S, C]) in float64; -inf and a zero gradient where the contract says so"""
    U = targets.shape[1]
    full, u = scatter(x, ranges, U)
    scores, gfull = fp.reference(full, targets, frames, tlens, blank, normalize, w)
    grad = np.zeros(x.shape)
    b, t, s = np.nonzero(u >= 0)
    grad[b, t, s] = gfull[b, t, u[b, t, s]]
    for i in range(len(scores)):
        if 1 <= frames[i] <= x.shape[1] and (np.diff(np.asarray(ranges[i, :frames[i]], np.int64)) < 0).any():
            scores[i], grad[i] = -np.inf, 0.0
    return scores, grad


def plane(Tb, Ub, S, kind, T):
    """one utterance's ranges: steps of 0, 1 and S - 1 in turn towards U_b - 1, so that the band sticks out past U_b;
    "flat": every step after the first one of S - 1 is 0; "zero": all 0.  Frames t >= T_b repeat the last entry."""
    r, jumped = [0], False
    for step in itertools.islice(itertools.cycle([0, 1, S - 1, S - 1, 0, 1]), max(Tb - 1, 0)):
        step = 0 if kind == "zero" or (kind == "flat" and jumped) else min(step, S - 1, max(Ub - 1 - r[-1], 0))
        jumped |= S > 1 and step == S - 1
        r.append(r[-1] + step)
    return (r + [r[-1]] * T)[:T]


@functools.lru_cache(maxsize=None)
def case(T, U, S, C, kind, normalize):
    """(x, ranges, targets, frames, tlens, blank, w, want scores, want grad) of a seeded case, read-only"""
    rng = np.random.default_rng(100000 * T + 1000 * U + 10 * S + C)
    blank = C // 2
    targets = ((blank + 1 + rng.integers(0, C - 1, (B, U))) % C).astype(np.int32)
    # full; random; one frame; no label; no frame; then random ones (a band of S columns needs U_b < S at T_b == 1)
    frames = np.asarray([T, rng.integers(1, T + 1), 1, T, 0] + list(rng.integers(1, T + 1, B - 5)), np.int32)
    tlens = np.asarray([U, rng.integers(0, U + 1), min(U, S - 1), 0] + list(rng.integers(0, U + 1, B - 4)), np.int32)
    ranges = np.asarray([plane(int(f), int(l), S, kind, T) for f, l in zip(frames, tlens)], np.int32)
    x = rng.standard_normal((B, T, S, C))
    x[:, :, :, blank] += 3 + math.log(C)  # (peaked as tests/transducer_fp.py's: |score| stays below 100)
    u = ranges[:, :, None] + np.arange(S)
    b, t, s = np.nonzero(u < U)
    x[b, t, s, targets[b, u[b, t, s]]] += 3 + math.log(C)
    x = x.astype(np.float32)
    if not normalize:
        x64 = x.astype(np.float64)
        x = (x64 - np.logaddexp.reduce(x64, axis=3, keepdims=True)).astype(np.float32)
    w = WEIGHTS[:B]
    out = (x, ranges, targets, frames, tlens, blank, w) + reference(x, ranges, targets, frames, tlens, blank, normalize, w)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def never_read(ranges, frames, tlens, S):
    """bool [B, T, S]: band rows with t >= T_b or u outside 0 .. U_b (every row of an utterance whose T_b is 0)"""
    T = ranges.shape[1]
    u = np.asarray(ranges, np.int64)[:, :, None] + np.arange(S)
    return (np.arange(T)[None, :, None] >= frames[:, None, None]) | (u < 0) | (u > tlens[:, None, None])


def check(name, scores, grad, want_scores, want_grad, ranges, frames, tlens):
    """the gates: score 1e-4 max(1, |want|), gradient 1e-4 absolute, never-read rows exactly 0, no NaN"""
    assert not np.isnan(scores).any() and not np.isnan(grad).any(), name
    for b, (got, want) in enumerate(zip(scores, want_scores)):
        print(f"{name} b={b} score {got!r} want {want!r}")
        assert got == want if np.isinf(want) else abs(got - want) <= 1e-4 * max(1.0, abs(want)), (name, b, got, want)
    print(f"{name} worst gradient error {np.abs(grad - want_grad).max():.3g}")
    assert np.abs(grad - want_grad).max() <= 1e-4, name
    assert not grad[never_read(ranges, frames, tlens, grad.shape[2])].any(), name


def occupancy(rows, frames, tlens):
    """float64 occupancies [B, T, U + 1] of the full lattice whose compact plane (lp_blank, lp_label, lse) is `rows`"""
    Bn, T, U1, _ = rows.shape
    occ = np.zeros((Bn, T, U1))
    for b in range(Bn):
        Tb, Ub = int(frames[b]), int(tlens[b])
        if not (1 <= Tb <= T and 0 <= Ub < U1):
            continue
        lpb, lpl = rows[b, :Tb, :Ub + 1, 0].astype(np.float64), rows[b, :Tb, :Ub + 1, 1].astype(np.float64)
        lpl[:, Ub] = -np.inf
        al, be = np.full((Tb, Ub + 1), -np.inf), np.full((Tb + 1, Ub + 2), -np.inf)
        for t, u in itertools.product(range(Tb), range(Ub + 1)):
            up = al[t - 1, u] + lpb[t - 1, u] if t else (0.0 if u == 0 else -np.inf)
            al[t, u] = np.logaddexp(up, al[t, u - 1] + lpl[t, u - 1] if u else -np.inf)
        be[Tb, Ub] = 0.0
        for t, u in itertools.product(range(Tb - 1, -1, -1), range(Ub, -1, -1)):
            be[t, u] = np.logaddexp(be[t + 1, u] + lpb[t, u], be[t, u + 1] + lpl[t, u])
        if np.isfinite(be[0, 0]):
            occ[b, :Tb, :Ub + 1] = np.exp(al + be[:Tb, :Ub + 1] - be[0, 0])
    return occ
