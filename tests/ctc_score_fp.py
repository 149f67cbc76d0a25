"""CTC scores of given hypotheses and their weighted gradient (TEST INFRASTRUCTURE ONLY).

Three things live here, shared by test_ctc_score_cpu.py and test_ctc_score_gpu.py:
  * the float64 yardstick: score(em, y) = log sum over the alignments of y of the summed emissions -- the alpha
    recursion over the states of ctc_target_graph, nothing subtracted -- and sum_k w_k d score_k / d em by alpha-beta;
  * a float32 transcription of gtn_amd/csrc/ctc_score.hip: the same recurrences with float32 arithmetic in the
    kernel's order of sums (the even states by lane, the xor tree of the wave, the waves ascending; a token's chain by
    ascending index; the pairs of an utterance in k order), so that the float32 error of the METHOD can be measured
    against the gate before a GPU is involved;
  * the generated cases, computed once per process and left unchanged.
The contract: len = clamp(length, 0, L); -inf when no alignment fits, len > max_length, a token
inside the length outside 0 .. C - 1, or T_b == 0; a -inf score or a weight of exactly 0 adds nothing to the gradient.
"""
import collections
import functools

import numpy as np

from ctc_fp64 import _lse
from ctc_beam_fp import continuous_case, holes_case

NEG = -np.inf
SCORE_GATE = 1e-4  # * max(1, |score|)
GRAD_GATE = 1e-4   # absolute, weights in [-1, 1]


# ---- the states of ctc_target_graph ----
def states(y, blank):
    """(label[S], skip_in[S]): skip_in[s] says the arc s - 2 -> s exists"""
    y = np.asarray(y, dtype=np.int64)
    S = 2 * y.size + 1
    lab = np.full(S, blank, dtype=np.int64)
    lab[1::2] = y
    skip = np.zeros(S, dtype=bool)
    if y.size > 1:
        skip[3::2] = y[1:] != y[:-1]
    return lab, skip


def hypothesis(tokens_row, length, L, C, max_length):
    """the hypothesis the contract reads out of a row, or None when the pair scores -inf by its tokens or length"""
    n = min(max(int(length), 0), L)
    if n > max_length:
        return None
    y = np.asarray(tokens_row[:n], dtype=np.int64)
    if ((y < 0) | (y >= C)).any():
        return None
    return y


def _up(a, k, fill=NEG):
    """a[s + k], `fill` where there is no such state"""
    return np.concatenate([a, np.full(k, fill, dtype=a.dtype)])[k:]


def band(S, T, t):
    """the states [lo, hi) that lie on an alignment at frame t: an arc advances two states at most, so state s is reached
    only with s <= 2 t + 1 and reaches an accepting state only with S - 2 - s <= 2 (T - 1 - t).  The states below lo
    never feed one inside a later band and those outside carry no occupancy, so both recursions below work on the band
    alone; with T well above the length the band is everything"""
    return max(0, S - 2 - 2 * (T - 1 - t)), min(S, 2 * t + 2)


# ---- float64 ----
def pair_fp64(em, y, blank, want_grad=True):
    """(score, d score / d em [T, C] or None) of one hypothesis under em [T, C], float64"""
    x = np.asarray(em, dtype=np.float64)
    T, C = x.shape
    if T == 0:
        return NEG, None
    lab, skip = states(y, blank)
    S = lab.size
    skip_out = _up(skip, 2, False)
    P = np.full((T, S + 2), NEG)  # alpha of state s in column s + 2
    P[0, 2:2 + min(S, 2)] = x[0, lab[:2]]
    for t in range(1, T):
        lo, hi = band(S, T, t)
        if lo >= hi:
            continue
        prev = P[t - 1]
        a = np.logaddexp(prev[lo + 2:hi + 2], prev[lo + 1:hi + 1])
        a = np.logaddexp(a, np.where(skip[lo:hi], prev[lo:hi], NEG))
        P[t, lo + 2:hi + 2] = a + x[t, lab[lo:hi]]
    last = P[T - 1, 2:]
    z = float(last[0] if S == 1 else np.logaddexp(last[S - 1], last[S - 2]))
    if np.isnan(z):
        z = NEG
    if not np.isfinite(z) or not want_grad:
        return z, None
    grad = np.zeros((T, C))
    beta = np.full(S + 2, NEG)
    beta[[S - 1] if S == 1 else [S - 1, S - 2]] = 0.0
    for t in range(T - 1, -1, -1):
        lo, hi = band(S, T, t)
        if lo >= hi:
            break
        with np.errstate(invalid="ignore"):
            occ = np.exp(P[t, lo + 2:hi + 2] + beta[lo:hi] - z)
        occ[~np.isfinite(occ)] = 0.0
        grad[t] = np.bincount(lab[lo:hi], weights=occ, minlength=C)
        if t == 0:
            break
        q = np.full(S + 2, NEG)
        q[lo:hi] = beta[lo:hi] + x[t, lab[lo:hi]]
        lo, hi = band(S, T, t - 1)
        beta = np.full(S + 2, NEG)
        if lo < hi:
            b = np.logaddexp(q[lo:hi], q[lo + 1:hi + 1])
            beta[lo:hi] = np.logaddexp(b, np.where(skip_out[lo:hi], q[lo + 2:hi + 2], NEG))
    return z, grad


# ---- float32, as the kernel does it ----
def config(U):
    """(workgroup width, states per lane): ctc_score_config of ctc_score.hip"""
    SM = 2 * U + 1
    for bound, cfg in ((64, (64, 1)), (256, (256, 1)), (768, (256, 3)), (1024, (1024, 1)), (2048, (1024, 2)),
                       (4096, (1024, 4))):
        if SM <= bound:
            return cfg
    return 1024, 9


def logadd32(x, y):
    """m + log1p(exp(n - m)) in float32, the -inf cases explicit"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    m, n = np.maximum(x, y), np.minimum(x, y)
    with np.errstate(invalid="ignore", over="ignore"):
        r = (m + np.log1p(np.exp(n - m, dtype=np.float32), dtype=np.float32)).astype(np.float32)
    return np.where(x == NEG, y, np.where(y == NEG, x, r)).astype(np.float32)


def forward_f32(em, y, blank):
    """(score, alpha [T, S + 2], state s in column s + 2) in float32: the kernel's recurrence.  The kernel works on every
    state; what it holds outside the band never reaches a state inside and has no occupancy (band), so it is left
    out here"""
    T = em.shape[0]
    lab, skip = states(y, blank)
    S = lab.size
    x = np.asarray(em, dtype=np.float32)
    P = np.full((T, S + 2), NEG, dtype=np.float32)
    P[0, 2:2 + min(S, 2)] = x[0, lab[:2]]
    for t in range(1, T):
        lo, hi = band(S, T, t)
        if lo >= hi:
            continue
        prev = P[t - 1]
        a = logadd32(prev[lo + 2:hi + 2], prev[lo + 1:hi + 1])
        a = np.where(skip[lo:hi], logadd32(a, prev[lo:hi]), a)
        with np.errstate(invalid="ignore"):
            P[t, lo + 2:hi + 2] = np.where(a == NEG, np.float32(NEG), a + x[t, lab[lo:hi]])
    last = P[T - 1, 2:]
    score = last[0] if S == 1 else logadd32(last[S - 1], last[S - 2])
    return np.float32(score), P


def backward_f32(grad, em, y, blank, U, w, score, P):
    """adds w * d score / d em into grad [T, C] (float32) in the kernel's order"""
    T = em.shape[0]
    WG, PER = config(U)
    NW = WG // 64
    lab, skip = states(y, blank)
    S, n = lab.size, len(y)
    x = np.asarray(em, dtype=np.float32)
    skip_out = _up(skip, 2, False)
    # the chains of equal tokens, ascending index: rounds[r] = (heads that have an r-th follower, that follower)
    chains = collections.OrderedDict()
    for i, v in enumerate(np.asarray(y).tolist()):
        chains.setdefault(v, []).append(i)
    lists = list(chains.values())
    heads = np.array([c[0] for c in lists], dtype=np.int64)
    head_lab = np.array(list(chains.keys()), dtype=np.int64)
    rounds = []
    for r in range(1, max((len(c) for c in lists), default=0)):
        sel = [h for h, c in enumerate(lists) if len(c) > r]
        rounds.append((np.array(sel, dtype=np.int64), np.array([lists[h][r] for h in sel], dtype=np.int64)))
    blank_head = np.nonzero(head_lab == blank)[0]
    lane_idx = np.arange(64)
    beta = np.full(S + 2, NEG, dtype=np.float32)
    beta[[S - 1] if S == 1 else [S - 1, S - 2]] = 0.0
    w, sc = np.float32(w), np.float32(score)
    for t in range(T - 1, -1, -1):
        lo, hi = band(S, T, t)
        if lo >= hi:
            break
        av, bv = P[t, lo + 2:hi + 2], beta[lo:hi]
        g = np.zeros(PER * WG, dtype=np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            g[lo:hi] = np.where((av > NEG) & (bv > NEG), np.exp((av + bv) - sc, dtype=np.float32), np.float32(0))
        # the even states: by lane (ascending state), the xor tree of the wave, the waves ascending
        lanes = g.reshape(PER, WG)
        ev = np.zeros(WG, dtype=np.float32)
        for j in range(PER):
            ev[0::2] = ev[0::2] + lanes[j, 0::2]
        v = ev.reshape(NW, 64)
        for off in (32, 16, 8, 4, 2, 1):
            v = v + v[:, lane_idx ^ off]
        evs = v[0, 0]
        for q in range(1, NW):
            evs = np.float32(evs + v[q, 0])
        go = g[1::2]
        if n:
            sums = go[heads].copy()
            if blank_head.size:
                sums[blank_head] = evs + sums[blank_head]
            for sel, follower in rounds:
                sums[sel] = sums[sel] + go[follower]
            grad[t, head_lab] = grad[t, head_lab] + w * sums
        if not blank_head.size:
            grad[t, blank] = grad[t, blank] + w * evs
        if t == 0:
            break
        m = np.full(S + 2, NEG, dtype=np.float32)
        with np.errstate(invalid="ignore"):
            m[lo:hi] = np.where(bv == NEG, np.float32(NEG), bv + x[t, lab[lo:hi]])
        lo, hi = band(S, T, t - 1)
        beta = np.full(S + 2, NEG, dtype=np.float32)
        if lo < hi:
            b = logadd32(m[lo:hi], m[lo + 1:hi + 1])
            beta[lo:hi] = np.where(skip_out[lo:hi], logadd32(b, m[lo + 2:hi + 2]), b)


# ---- a batch, both ways ----
Case = collections.namedtuple("Case", "em tokens lengths blank frames max_length weights")
Result = collections.namedtuple("Result", "scores grad scores32 grad32")


def default_max_length(case):
    return max(1, min(case.tokens.shape[-1], case.em.shape[1], 4096))


def evaluate(case, f32=True):
    """Result of a case: float64 scores [B, N] and gradient [B, T, C], and the float32 transcription's"""
    em = case.em
    B, T, C = em.shape
    tokens = case.tokens.reshape(B, -1, case.tokens.shape[-1])
    N, L = tokens.shape[1:]
    lengths = np.asarray(case.lengths).reshape(B, N)
    weights = np.asarray(case.weights, dtype=np.float32).reshape(B, N)
    U = case.max_length if case.max_length is not None else default_max_length(case)
    scores = np.full((B, N), NEG)
    grad = np.zeros((B, T, C))
    scores32 = np.full((B, N), NEG, dtype=np.float32)
    grad32 = np.zeros((B, T, C), dtype=np.float32)
    for b in range(B):
        Tb = T if case.frames is None else int(case.frames[b])
        x = em[b, :Tb]
        for k in range(N):
            y = hypothesis(tokens[b, k], lengths[b, k], L, C, U)
            if y is None or Tb == 0:
                continue
            z, g = pair_fp64(x, y, case.blank)
            scores[b, k] = z
            if g is not None and weights[b, k] != 0:
                grad[b, :Tb] += float(weights[b, k]) * g
            if f32:
                z32, alpha = forward_f32(x, y, case.blank)
                scores32[b, k] = z32
                if z32 > NEG and weights[b, k] != 0:
                    backward_f32(grad32[b, :Tb], x, y, case.blank, U, weights[b, k], z32, alpha)
    return Result(scores, grad, scores32, grad32)


def score_ok(got, want):
    """every score inside the gate; -inf exactly where the yardstick has it"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    if not (np.isneginf(got[~fin]).all() and np.isfinite(got[fin]).all()):
        return False
    return bool((np.abs(got[fin] - want[fin]) <= SCORE_GATE * np.maximum(1.0, np.abs(want[fin]))).all())


def score_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    return float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin])), initial=0.0))


def grad_err(got, want):
    d = np.abs(np.asarray(got, np.float64) - want)
    return float(np.max(d, initial=0.0)) if np.isfinite(d).all() else np.inf


# ---- the cases ----
def tokens_of(rng, n, C, blank, mode):
    labels = np.array([c for c in range(C) if c != blank])
    if mode == "repeat" or labels.size == 1:
        return np.full(n, labels[rng.integers(labels.size)], dtype=np.int32)
    y = rng.choice(labels, n).astype(np.int32)
    if mode == "norepeat":
        for i in range(1, n):
            while y[i] == y[i - 1]:
                y[i] = labels[rng.integers(labels.size)]
    return y


def frames_needed(y):
    y = np.asarray(y)
    return int(y.size + np.count_nonzero(y[1:] == y[:-1]))


def pack(hyps, B, N, L, lengths_dtype=np.int32):
    """tokens [B, N, L] (-1 from each length on) and lengths [B, N] of B * N label sequences"""
    tokens = np.full((B, N, L), -1, dtype=np.int32)
    lengths = np.zeros((B, N), dtype=lengths_dtype)
    for p, y in enumerate(hyps):
        tokens[p // N, p % N, :len(y)] = y
        lengths[p // N, p % N] = len(y)
    return tokens, lengths


def weights_of(rng, B, N):
    return rng.uniform(-1.0, 1.0, (B, N)).astype(np.float32)


def near_path_case(seed, hyps_per_utt, T, C, blank, peak=6.0, frames=None):
    """emissions [B, T, C], log-softmax of small noise with a peak along one alignment of each utterance's FIRST
    hypothesis: scores of small magnitude whatever T is"""
    rng = np.random.default_rng(seed)
    B = len(hyps_per_utt)
    x = rng.normal(0.0, 0.5, (B, T, C))
    for b, y in enumerate(hyps_per_utt):
        lab, _ = states(y, blank)
        path = []  # one alignment: every label once, a blank between repeats, blanks to fill
        for i, v in enumerate(y):
            if i and y[i - 1] == v:
                path.append(blank)
            path.append(int(v))
        Tb = T if frames is None else frames[b]
        extra = Tb - len(path)
        where = np.sort(rng.integers(0, len(path) + 1, max(extra, 0)))
        full, j = [], 0
        for i in range(len(path) + 1):
            while j < len(where) and where[j] == i:
                full.append(blank)
                j += 1
            if i < len(path):
                full.append(path[i])
        x[b, np.arange(Tb), np.array(full[:Tb])] += peak
    x = x - x.max(axis=2, keepdims=True)
    return (x - np.log(np.exp(x).sum(axis=2, keepdims=True))).astype(np.float32)


def flat_case(seed, B, T, C, sigma=0.5):
    """scores around 0, not normalised (any scores are emissions)"""
    return np.random.default_rng(seed).normal(0.0, sigma, (B, T, C)).astype(np.float32)


# What float32 can give.  Every step of the recursions rounds to an ulp of |alpha|, which grows to |score|; alpha + beta
# - score then carries about sqrt(2 T) ulp(|score|) / 4 into an occupancy of up to 1.  The gate of 1e-4 on gradients is
# therefore within reach of ANY float32 log-domain recursion only while |score| stays within a few hundred at these T
# (ulp(256) = 3e-5): the cases keep their scores there -- emissions around 0, or peaked along an alignment of the
# hypotheses -- instead of, say, log-softmax rows of 37 labels over 1200 frames (|score| about 4000, ulp 2.4e-4).
LENS = (0, 1, 31, 32, 33, 127, 128, 129, 5)


def _lens_case(C, blank, max_length=None):
    rng = np.random.default_rng(11 + C)
    B, N, L = 3, 3, 129
    hyps = [tokens_of(rng, n, C, blank, "random") for n in LENS]
    T = max(frames_needed(y) for y in hyps) + 2
    tokens, lengths = pack(hyps, B, N, L)
    em = flat_case(21 + C, B, T, C)
    return Case(em, tokens, lengths, blank, None, max_length, weights_of(rng, B, N))


def _c2_case():
    """C = 2: every hypothesis is all repeats.  B = 7, N = 1; the longest fits exactly, utterance 4 is short by a frame"""
    rng = np.random.default_rng(5)
    lens = (0, 1, 2, 3, 8, 5, 13)
    hyps = [np.full(n, 1, dtype=np.int32) for n in lens]
    T = 25
    frames = (25, 3, 3, 5, 14, 25, 25)
    tokens, lengths = pack(hyps, 7, 1, 13)
    return Case(continuous_case(3, 7, T, 2), tokens, lengths, 0, frames, None, weights_of(rng, 7, 1))


def _c37_case():
    rng = np.random.default_rng(37)
    B, N, L, T, C, blank = 3, 4, 48, 60, 37, 36
    hyps = [tokens_of(rng, int(n), C, blank, "random") for n in rng.integers(0, 41, B * N)]
    tokens, lengths = pack(hyps, B, N, L, np.int64)
    em = flat_case(8, B, T, C)
    em[np.isneginf(holes_case(8, B, T, C, p=0.2))] = NEG  # (never a whole row)
    return Case(em, tokens, lengths, blank, None, None, weights_of(rng, B, N))


def _c256_case():
    rng = np.random.default_rng(256)
    B, N, L, T, C, blank = 1, 4, 72, 80, 256, 0
    hyps = [tokens_of(rng, n, C, blank, "random") for n in (60, 64, 70, 3)]
    tokens, lengths = pack(hyps, B, N, L)
    em = flat_case(256, B, T, C)
    return Case(em, tokens, lengths, blank, None, None, weights_of(rng, B, N))


def _edges_case(max_length=None):
    """C = 5, blank = 2, T = 9, L = 8: the contract's edges one per slot"""
    C, blank, T, L = 5, 2, 9, 8
    rng = np.random.default_rng(99)
    tokens = np.full((3, 4, L), -1, dtype=np.int32)
    lengths = np.zeros((3, 4), dtype=np.int32)

    def put(b, k, row, n):
        tokens[b, k, :len(row)] = row
        lengths[b, k] = n
    put(0, 0, [1, 1, 1, 1, 1], 5)           # all repeats: 9 frames, fits exactly
    put(0, 1, [1, 1, 1, 1, 1, 3], 6)        # needs 10: short by one frame
    put(0, 2, [0, 2, 2, 4], 4)              # a token equal to blank, twice in a row
    put(0, 3, [], 0)                        # a beam slot without a hypothesis
    put(1, 0, [1, -1, 3], 3)                # -1 inside the length
    put(1, 1, [1, 5, 3], 3)                 # C inside the length
    put(1, 2, [3, 4, 0], -3)                # a negative length: the empty sequence
    put(1, 3, [0, 1, 0, 3, 4, 3, 1, 0], 100)  # a length above L: the row's width counts
    put(2, 0, [4, 3, 4, 3], 4)
    put(2, 1, [1, 5, -1, 7], 1)             # no labels past the length are looked at
    put(2, 2, [2], 1)                       # the blank alone
    put(2, 3, [0, 1, 3, 4, 0, 1, 3], 7)
    w = weights_of(rng, 3, 4)
    w[0, 1] = 0.0  # an exact 0 on a -inf pair
    w[2, 0] = 0.0  # ... and on a finite one
    return Case(continuous_case(17, 3, T, C), tokens, lengths, blank, None, max_length, w)


def _holes_case():
    """-inf holes; utterance 1 has a row without anything: no path for any hypothesis"""
    rng = np.random.default_rng(41)
    B, N, L, T, C, blank = 3, 3, 10, 20, 5, 0
    em = holes_case(12, B, T, C, p=0.3).copy()
    em[1, T // 2] = NEG
    hyps = [tokens_of(rng, int(n), C, blank, "random") for n in rng.integers(0, 9, B * N)]
    tokens, lengths = pack(hyps, B, N, L)
    return Case(em, tokens, lengths, blank, None, None, weights_of(rng, B, N))


RAGGED_FRAMES = (40, 1, 0, 39, 33, 2, 40)


def _ragged_case(pad=np.nan):
    """input_lengths from 0 to T, the pad rows filled with `pad`"""
    rng = np.random.default_rng(77)
    B, N, L, T, C, blank = 7, 3, 24, 40, 5, 4
    em = continuous_case(9, B, T, C).copy()
    for b, f in enumerate(RAGGED_FRAMES):
        em[b, f:] = pad
    hyps = [tokens_of(rng, int(n), C, blank, "random") for n in rng.integers(0, 16, B * N)]
    hyps[3] = hyps[3][:1]   # utterance 1 has one frame: one label fits
    hyps[15] = hyps[15][:2]  # utterance 5 has two
    tokens, lengths = pack(hyps, B, N, L)
    return Case(em, tokens, lengths, blank, RAGGED_FRAMES, None, weights_of(rng, B, N))


def _drift_case():
    """T = 1200, len about 100, B = N = 2: the rounding of 1200 float32 log-adds in a row"""
    rng = np.random.default_rng(1200)
    B, N, L, T, C, blank = 2, 2, 112, 1200, 37, 0
    hyps = []
    for b in range(B):
        y = tokens_of(rng, 100 + 4 * b, C, blank, "random")
        z = y.copy()
        z[50] = z[50] % (C - 1) + 1  # the second hypothesis: one other label
        hyps += [y, z]
    tokens, lengths = pack(hyps, B, N, L)
    em = near_path_case(1201, [hyps[0], hyps[2]], T, C, blank, peak=9.0)
    return Case(em, tokens, lengths, blank, None, None, weights_of(rng, B, N))


# the widths above 256 states: max_length -> the lengths at which the states a lane works on change
WIDE = {383: (383, 256, 255), 511: (511, 385, 384), 1023: (1023, 512, 511), 2047: (2047, 1536, 1535, 1024),
        4096: (4096, 4095, 3584, 3583, 3072, 3071, 2560, 2559, 2048)}


def _wide_case(U):
    """B utterances of one hypothesis each, T_b = len + 1: a lane owns several states"""
    rng = np.random.default_rng(U)
    lens = WIDE[U]
    B, C, blank = len(lens), 37, 0
    hyps = [tokens_of(rng, n, C, blank, "norepeat") for n in lens]
    frames = tuple(n + 1 for n in lens)
    T = max(frames)
    tokens, lengths = pack(hyps, B, 1, U)
    em = near_path_case(U + 1, hyps, T, C, blank, peak=10.0, frames=frames)
    for b, f in enumerate(frames):
        em[b, f:] = np.nan
    return Case(em, tokens, lengths, blank, frames, U, weights_of(rng, B, 1))


BUILDERS = {
    "lens-c5": lambda: _lens_case(5, 0),
    "lens-c5-u31": lambda: _lens_case(5, 0, 31),    # one wave; the longer ones are above max_length
    "lens-c5-u32": lambda: _lens_case(5, 0, 32),    # 65 states: the first width above a wave
    "lens-c5-u127": lambda: _lens_case(5, 0, 127),  # 255 states: one per lane of 256
    "lens-c5-u128": lambda: _lens_case(5, 0, 128),  # 257 states: three per lane
    "c2-repeats": _c2_case,
    "c37-holes": _c37_case,
    "c256": _c256_case,
    "edges": _edges_case,
    "edges-u7": lambda: _edges_case(7),
    "holes-dead": _holes_case,
    "ragged": _ragged_case,
    "drift": _drift_case,
}
BUILDERS.update({f"wide-u{U}": (lambda U=U: _wide_case(U)) for U in WIDE})
ALL_GPU_CASES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def result(name, f32=True):
    """the Result of a named case, computed once per process and left unchanged"""
    return evaluate(case(name), f32)
