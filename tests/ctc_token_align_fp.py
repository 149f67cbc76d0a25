"""The yardstick of the batched CTC token alignment (gtnx_batch_ctc_token_align, ctc_token_align.hip) and its cases.

`align_pair` is a numpy FLOAT32 transcription of the contract: the states of ctcGraph(y, blank), a
candidate alpha[source] + e(t, label(s)) by one float32 addition, the exact maximum, and of the candidates that reach it
the one whose source state has the smallest rank in the order

    0 | (2i, 2i-1) for i = 1..p | S-1 | for i = U-1 down to p+1: (2i, 2i+1) if y[i] != y[i-1] else (2i+1, 2i) | 2p+1

(U = len, S = 2 U + 1, p leading strict ascents), the smaller of two equal end states, token scores summed in ascending
frame order from the first frame's value.  The rank order is built here as the list above, not by the kernel's closed
form.  The contract makes every output reproducible bit for bit, so the GPU tests compare bits and there is no
tolerance; tests/test_ctc_token_align_cpu.py pins this file to the oracle's shortest_path on tie-heavy inputs, to
ctc_align_fp64 on continuous ones and to an enumeration."""
import collections
import functools

import numpy as np

from ctc_score_fp import config, frames_needed, pack, tokens_of  # noqa: F401  (config: the kernel's widths)

NEG = np.float32(-np.inf)
BIG = 0x7FFFFFFF

Case = collections.namedtuple("Case", "em tokens lengths blank frames max_length")
Result = collections.namedtuple("Result", "scores starts ends token_scores frame_tokens")
Pair = collections.namedtuple("Pair", "score starts ends token_scores frame_tokens")


def rank_order(y):
    """the states in the order of their ranks"""
    U = len(y)
    if U == 0:
        return [0]
    p = 0
    while p + 1 < U and y[p] < y[p + 1]:
        p += 1
    order = [0]
    for i in range(1, p + 1):
        order += [2 * i, 2 * i - 1]
    order.append(2 * U)
    for i in range(U - 1, p, -1):
        order += [2 * i, 2 * i + 1] if y[i] != y[i - 1] else [2 * i + 1, 2 * i]
    order.append(2 * p + 1)
    assert sorted(order) == list(range(2 * U + 1))
    return order


def no_path(L, M):
    return Pair(NEG, np.full(L, -1, np.int32), np.full(L, -1, np.int32), np.full(L, NEG, np.float32),
                np.full(M, -1, np.int32))


def align_pair(em, row, length, blank, T, max_length):
    """one pair: em float32 [M, C] (rows from T on are not looked at), row int32 [L], the pair's length as stored"""
    em = np.asarray(em)
    assert em.dtype == np.float32
    M, C = em.shape
    L = len(row)
    T = min(max(int(T), 0), M)
    n = min(max(int(length), 0), L)
    dead = no_path(L, M)
    if n > max_length or T == 0:
        return dead
    y = np.asarray(row[:n], dtype=np.int64)
    if ((y < 0) | (y >= C)).any():
        return dead
    S = 2 * n + 1
    lab = np.full(S, blank, dtype=np.int64)
    lab[1::2] = y
    skip = np.zeros(S, dtype=bool)
    if n > 1:
        skip[3::2] = y[1:] != y[:-1]
    rank = np.empty(S, dtype=np.int64)
    rank[rank_order(y.tolist())] = np.arange(S)
    r0 = rank
    r1 = np.concatenate(([BIG - 1], rank[:-1]))
    r2 = np.concatenate(([BIG - 1, BIG - 1], rank[:-2]))[:S]
    alpha = np.full(S, NEG, dtype=np.float32)
    alpha[0] = np.float32(0.0)
    bp = np.zeros((T, S), dtype=np.int8)
    ar = np.arange(S)
    with np.errstate(invalid="ignore"):
        for t in range(T):
            e = em[t, lab]
            c0 = alpha + e
            c1 = np.concatenate(([NEG], alpha[:-1])).astype(np.float32) + e
            c2 = np.where(skip, np.concatenate(([NEG, NEG], alpha[:-2]))[:S].astype(np.float32) + e, NEG).astype(np.float32)
            best = np.maximum(np.maximum(c0, c1), c2)
            q = np.stack([np.where(c0 == best, r0, BIG), np.where(c1 == best, r1, BIG), np.where(c2 == best, r2, BIG)])
            k = np.argmin(q, axis=0)  # (the first minimum: ranks of different states differ)
            bp[t] = np.where(best == NEG, 0, k)
            alpha = best.astype(np.float32)
            assert alpha.dtype == np.float32 and c0.dtype == np.float32
    if S == 1:
        score, node = alpha[0], 0
    else:
        score = max(alpha[S - 1], alpha[S - 2])
        node = S - 2 if alpha[S - 2] == score else S - 1
    if not score > NEG:
        return dead
    ft = np.full(M, -1, np.int32)
    for t in range(T - 1, -1, -1):
        ft[t] = (node - 1) // 2 if node % 2 else -1
        node -= int(bp[t, node])
    assert node == 0
    starts, ends, ts = dead.starts.copy(), dead.ends.copy(), dead.token_scores.copy()
    for i in range(n):
        on = np.flatnonzero(ft[:T] == i)
        assert on.size and (np.diff(on) == 1).all()
        starts[i], ends[i] = on[0], on[-1] + 1
        s = em[on[0], y[i]]
        for t in on[1:]:
            s = np.float32(s + em[t, y[i]])
        ts[i] = s
    return Pair(np.float32(score), starts, ends, ts, ft)


def default_max_length(case):
    L, T = case.tokens.shape[-1], case.em.shape[1]
    return max(1, min(L, T, 4096))


def evaluate(case):
    B, M, C = case.em.shape
    N, L = case.tokens.shape[1:]
    U = case.max_length if case.max_length is not None else default_max_length(case)
    out = Result(np.empty((B, N), np.float32), np.empty((B, N, L), np.int32), np.empty((B, N, L), np.int32),
                 np.empty((B, N, L), np.float32), np.empty((B, N, M), np.int32))
    for b in range(B):
        T = M if case.frames is None else int(case.frames[b])
        for k in range(N):
            r = align_pair(case.em[b], case.tokens[b, k], case.lengths[b, k], case.blank, T, U)
            out.scores[b, k] = r.score
            for dst, src in zip(out[1:], r[1:]):
                dst[b, k] = src
    return out


# ---- emissions ----
def continuous(seed, B, T, C):
    return np.random.default_rng(seed).normal(0, 2, (B, T, C)).astype(np.float32)


def integer(seed, B, T, C, lo, hi):
    return np.random.default_rng(seed).integers(lo, hi + 1, (B, T, C)).astype(np.float32)


# ---- the cases ----
WIDTHS = (31, 32, 127, 128, 383, 384, 511, 512, 1023, 1024, 2047, 2048, 4096)


def _width_case(U):
    """a hypothesis of max_length tokens without repeats and a shorter one (a token shorter; half as long at the widest,
    to keep the yardstick quick) with a repeat every 64 tokens or so, T just above what they need"""
    rng = np.random.default_rng(U)
    C, blank = 6, 0
    hyps = [tokens_of(rng, U, C, blank, "norepeat"), tokens_of(rng, U - 1 if U <= 1024 else U // 2, C, blank, "norepeat")]
    for i in rng.integers(1, hyps[1].size, U // 64 + 1):
        hyps[1][i] = hyps[1][i - 1]
    need = [frames_needed(h) for h in hyps]
    T = max(need) + 3
    tokens, lengths = pack(hyps, 1, 2, U)
    # half-integer emissions with a continuous part: exact ties among many states and none, both
    em = (continuous(U + 1, 1, T, C) * (rng.random((1, T, 1)) < 0.5) + integer(U + 2, 1, T, C, -2, 2)).astype(np.float32)
    return Case(em, tokens, lengths, blank, None, U)


WORD_FRAMES = (1, 15, 16, 17, 63, 64, 65, 129)


def _word_case():
    """every T_b at which the last word of a row, or the 64 frames of a store, is full, one short or one over; lengths 0
    and 1, where the path never descends, next to ones that fill the frames"""
    rng = np.random.default_rng(11)
    C, blank, M = 5, 2, 129
    hyps = []
    for T in WORD_FRAMES:
        hyps += [np.zeros(0, np.int32), tokens_of(rng, 1, C, blank, "random"), tokens_of(rng, min(T, 40), C, blank, "norepeat"),
                 tokens_of(rng, min(max(1, T // 3), 40), C, blank, "random")]
    tokens, lengths = pack(hyps, len(WORD_FRAMES), 4, 40)
    em = continuous(12, len(WORD_FRAMES), M, C)
    return Case(em, tokens, lengths, blank, np.asarray(WORD_FRAMES, np.int32), 40)


DESCENT_LENS = (16, 17, 33, 64)


def _descent_case():
    """all-distinct tokens with T_b == len: every step descends two states, the 32-state reach of a word row; ascending
    tokens (every state in the first group of the rank order) and a permutation"""
    rng = np.random.default_rng(13)
    C, blank = 70, 0
    hyps = []
    for n in DESCENT_LENS:
        hyps += [np.arange(1, n + 1, dtype=np.int32), (rng.permutation(C - 1)[:n] + 1).astype(np.int32)]
    tokens, lengths = pack(hyps, len(DESCENT_LENS), 2, 64)
    return Case(continuous(14, len(DESCENT_LENS), 64, C), tokens, lengths, blank, np.asarray(DESCENT_LENS, np.int32), 64)


TIE_LENS = (5, 40, 200)


def _ties_case(blank_tokens=False):
    """all-zero and {0, 1} emissions, hypotheses with repeats: every maximum is a tie somewhere"""
    rng = np.random.default_rng(17)
    C, blank, T = 4, 0, 300
    hyps = []
    for _ in range(2):
        for n in TIE_LENS:
            y = rng.integers(0 if blank_tokens else 1, C, n).astype(np.int32)
            hyps.append(y)
    assert all(frames_needed(h) <= T - 20 for h in hyps)
    tokens, lengths = pack(hyps, 2, 3, 200)
    em = np.zeros((2, T, C), np.float32)
    em[1] = integer(18, 1, T, C, 0, 1)[0]
    return Case(em, tokens, lengths, blank, np.asarray([T, T - 20], np.int32), 200)


def _align_case(zero):
    """tokens above blank, lengths up to 255: what ctc_forced_align takes too"""
    rng = np.random.default_rng(19)
    C, blank, T = 12, 0, 300
    hyps = [tokens_of(rng, n, C, blank, "random") for n in (1, 7, 31, 32, 100, 255)]
    frames = np.asarray([T, 20, 64, 65, 160, T], np.int32)
    assert all(frames_needed(h) <= f for h, f in zip(hyps, frames))
    tokens, lengths = pack(hyps, 6, 1, 255)
    em = np.zeros((6, T, C), np.float32) if zero else continuous(20, 6, T, C)
    return Case(em, tokens, lengths, blank, frames, 255)


NOPATH_FRAMES = (30, 0, 9, 30, 30, 12)


def _nopath_case(pad=np.nan, garbage=None):
    """pairs without a path next to good ones.  Utterance 1 has no frames; 2 has one frame too few for its first two
    hypotheses; in 3 a -inf column cuts every path of the hypotheses that use label 3; 4 carries tokens that are no
    label and lengths outside 0 .. L; 5 is ordinary.  `pad` fills the emission rows from T_b on, `garbage` the token
    elements from each length on"""
    rng = np.random.default_rng(23)
    C, blank, M, L, N = 7, 1, 30, 12, 4
    B = len(NOPATH_FRAMES)
    em = continuous(24, B, M, C)
    hyps = [[tokens_of(rng, n, C, blank, "random") for n in (3, 8, 0, 11)] for _ in range(B)]
    hyps[5][3] = tokens_of(rng, 12, C, blank, "norepeat")          # fits 12 frames, but lies above max_length 11
    hyps[2][0] = np.asarray([2, 2, 3, 3, 4, 4, 5], np.int32)     # needs 10 frames, has 9
    hyps[2][1] = np.asarray([0, 2, 3, 4, 5, 6, 0, 2, 3, 4], np.int32)  # needs 10
    hyps[2][3] = np.asarray([2, 3, 4, 5, 6, 0, 2, 3, 4], np.int32)  # needs 9: fits exactly
    hyps[3][0] = np.asarray([2, 3, 2], np.int32)
    hyps[3][1] = np.asarray([2, 4, 2, 5], np.int32)
    em[3, :, 3] = -np.inf
    hyps[4][0] = np.asarray([2, -1, 3], np.int32)
    hyps[4][1] = np.asarray([2, C, 3], np.int32)
    tokens, lengths = pack([h for u in hyps for h in u], B, N, L)
    lengths[4, 2] = -3     # (counts as 0: the empty sequence)
    lengths[4, 3] = L + 5  # (counts as L, which is above max_length)
    if garbage is not None:
        past = np.arange(L)[None, None, :] >= np.clip(lengths, 0, L)[:, :, None]
        tokens[past] = np.random.default_rng(garbage).integers(-5, 10 ** 6, int(past.sum()))
    for b, f in enumerate(NOPATH_FRAMES):
        em[b, f:] = pad
    return Case(em, tokens, lengths, blank, np.asarray(NOPATH_FRAMES, np.int32), 11)


def _flat_case():
    """N == 1, the [B, L] form"""
    rng = np.random.default_rng(29)
    C, blank, T = 9, 8, 50
    hyps = [tokens_of(rng, n, C, blank, "random") for n in (4, 0, 17, 30, 9)]
    tokens, lengths = pack(hyps, 5, 1, 30)
    lengths[1, 0] = -7  # (counts as 0)
    lengths[3, 0] = 35  # (counts as L = 30, the hypothesis's length)
    return Case(continuous(30, 5, T, C), tokens, lengths, blank, np.asarray([50, 3, 40, 50, 9], np.int32), None)


def _slices_case():
    rng = np.random.default_rng(31)
    C, blank, T = 10, 0, 70
    hyps = [tokens_of(rng, int(n), C, blank, "random") for n in rng.integers(0, 30, 12)]
    tokens, lengths = pack(hyps, 4, 3, 32)
    return Case(integer(32, 4, T, C, -1, 1), tokens, lengths, blank, np.asarray([70, 33, 64, 17], np.int32), 32)


BUILDERS = {f"width-{U}": functools.partial(_width_case, U) for U in WIDTHS}
BUILDERS.update({
    "words": _word_case,
    "descent": _descent_case,
    "ties": _ties_case,
    "ties-blank-tokens": functools.partial(_ties_case, True),
    "align-continuous": functools.partial(_align_case, False),
    "align-zero": functools.partial(_align_case, True),
    "nopath": _nopath_case,
    "flat": _flat_case,
    "slices": _slices_case,
})
ALL_GPU_CASES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def result(name):
    return evaluate(case(name))
