"""The yardstick of the batched ASG token alignment (gtnx_batch_asg_token_align, asg_token_align.hip) and its cases.

`align_pair` is a numpy FLOAT32 transcription of the contract: position i = 0 .. len - 1 carries
y[i]; with w_self[i] = tr[y_i][y_i], w_step[i] = tr[y_i][y_{i-1}] and w_step[0] = start[y_0]

    alpha_0[0] = 0.0f + (w_step[0] + e(0, y_0)), every other alpha_0[i] = -inf
    c0 = alpha_{t-1}[i] + (w_self[i] + e(t, y_i)),  c1 = alpha_{t-1}[i-1] + (w_step[i] + e(t, y_i))
    alpha_t[i] = max(c0, c1), of two equal candidates the step (c1 >= c0)

the score is alpha_{T-1}[len - 1], token scores are summed in ascending frame order from the first frame's value.  The
contract makes every output reproducible bit for bit, so the GPU tests compare bits and there is no tolerance;
tests/test_asg_token_align_cpu.py pins this file to the oracle's shortest_path on integer-valued inputs and to the
float64 forms (`align_pair64` here, asg_align_fp64 of tests/asg_align_fp.py) on continuous ones."""
import collections
import functools

import numpy as np

from asg_score_fp import CONFIGS, config, pack, table_of  # noqa: F401  (config: the kernel's widths)

NEG = np.float32(-np.inf)

Case = collections.namedtuple("Case", "em trans start tokens lengths frames max_length")
Result = collections.namedtuple("Result", "scores starts ends token_scores frame_tokens")
Pair = collections.namedtuple("Pair", "score starts ends token_scores frame_tokens")


def no_path(L, M):
    return Pair(NEG, np.full(L, -1, np.int32), np.full(L, -1, np.int32), np.full(L, NEG, np.float32),
                np.full(M, -1, np.int32))


def _sweep(em, table, y, T, dtype):
    """the alpha recursion in `dtype`: (score, back-pointer bits [T, n]); bit 1 is the step"""
    C = em.shape[1]
    n = len(y)
    tr = table[C:].reshape(C, C)
    w_self = tr[y, y].astype(dtype)
    w_step = np.concatenate(([table[y[0]]], tr[y[1:], y[:-1]])).astype(dtype)
    ninf = dtype(-np.inf)
    bp = np.ones((T, n), dtype=np.int8)
    with np.errstate(invalid="ignore"):
        alpha = np.full(n, ninf, dtype=dtype)
        alpha[0] = dtype(0.0) + (w_step[0] + em[0, y[0]].astype(dtype))
        for t in range(1, T):
            e = em[t, y].astype(dtype)
            c0 = alpha + (w_self + e)
            c1 = np.concatenate(([ninf], alpha[:-1])).astype(dtype) + (w_step + e)
            bp[t] = c1 >= c0
            alpha = np.maximum(c0, c1)
            assert alpha.dtype == dtype
    return alpha[n - 1], bp


def _walk(bp, T, n, M):
    """the position of every frame: from len - 1 behind frame T - 1 down, never below 0"""
    ft = np.full(M, -1, np.int32)
    node = n - 1
    for t in range(T - 1, -1, -1):
        ft[t] = node
        node -= min(int(bp[t, node]), node)
    return ft, node


def align_pair(em, table, row, length, T, max_length):
    """one pair: em float32 [M, C] (rows from T on are not looked at), table float32 [C + C * C], row int32 [L], the
    pair's length as stored"""
    em = np.asarray(em)
    table = np.asarray(table)
    assert em.dtype == np.float32 and table.dtype == np.float32
    M, C = em.shape
    L = len(row)
    T = min(max(int(T), 0), M)
    n = min(max(int(length), 0), L)
    dead = no_path(L, M)
    if n == 0 or n > max_length or T < n:
        return dead
    y = np.asarray(row[:n], dtype=np.int64)
    if ((y < 0) | (y >= C)).any():
        return dead
    score, bp = _sweep(em, table, y, T, np.float32)
    if not score > NEG:
        return dead
    ft, node = _walk(bp, T, n, M)
    assert node == 0 and ft[0] == 0
    starts, ends, ts = dead.starts.copy(), dead.ends.copy(), dead.token_scores.copy()
    first = np.flatnonzero(np.diff(ft[:T], prepend=-1))  # the first frame of every token, ascending
    assert first.size == n
    starts[:n] = first
    ends[:n] = np.concatenate((first[1:], [T]))
    for i in range(n):
        s = em[starts[i], y[i]]
        for t in range(starts[i] + 1, ends[i]):
            s = np.float32(s + em[t, y[i]])
        ts[i] = s
    return Pair(np.float32(score), starts, ends, ts, ft)


def align_pair64(em, table, row, length, T):
    """the float64 form of a pair that has a path by its shape: (score, frame tokens [T])"""
    em = np.asarray(em, np.float64)
    table = np.asarray(table, np.float64)
    y = np.asarray(row[:length], dtype=np.int64)
    score, bp = _sweep(em, table, y, T, np.float64)
    ft, _ = _walk(bp, T, len(y), T)
    return float(score), ft


def default_max_length(case):
    L, T = case.tokens.shape[-1], case.em.shape[1]
    return max(1, min(L, T, 4096))


def max_length_of(case):
    return case.max_length if case.max_length is not None else default_max_length(case)


def evaluate(case):
    B, M, C = case.em.shape
    N, L = case.tokens.shape[1:]
    U = max_length_of(case)
    table = table_of(case.start, case.trans)
    out = Result(np.empty((B, N), np.float32), np.empty((B, N, L), np.int32), np.empty((B, N, L), np.int32),
                 np.empty((B, N, L), np.float32), np.empty((B, N, M), np.int32))
    for b in range(B):
        T = M if case.frames is None else int(case.frames[b])
        for k in range(N):
            r = align_pair(case.em[b], table, case.tokens[b, k], case.lengths[b, k], T, U)
            out.scores[b, k] = r.score
            for dst, src in zip(out[1:], r[1:]):
                dst[b, k] = src
    return out


# ---- inputs ----
def continuous(seed, *shape):
    return np.random.default_rng(seed).normal(0, 2, shape).astype(np.float32)


def integer(seed, shape, lo, hi):
    return np.random.default_rng(seed).integers(lo, hi + 1, shape).astype(np.float32)


def model(seed, B, T, C):
    """continuous emissions [B, T, C], transitions [C, C] and start [C]"""
    return continuous(seed, B, T, C), continuous(seed + 1000, C, C) / 2, continuous(seed + 2000, C) / 2


def labels_of(rng, n, C, rep=0.3):
    """n labels, a share `rep` of them equal to the one before"""
    y = rng.integers(0, C, n).astype(np.int32)
    for i in range(1, n):
        if rng.random() < rep:
            y[i] = y[i - 1]
    return y


# ---- the cases ----
WIDTHS = (1, 2, 63, 64, 65, 255, 256, 257, 768, 769, 1024, 1025, 2048, 2049, 4096)


def _width_case(U):
    """max_length U, one hypothesis of that length and one a label shorter, T_b = len + 3, C = 5, B = 1, N = 2; half-
    integer emissions and table with a continuous part: exact ties among many positions and none, both"""
    rng = np.random.default_rng(U)
    C = 5
    hyps = [labels_of(rng, U, C), labels_of(rng, U - 1, C)]
    T = U + 3
    tokens, lengths = pack(hyps, 1, 2, U)
    em = (continuous(U + 1, 1, T, C) * (rng.random((1, T, 1)) < 0.5) + integer(U + 2, (1, T, C), -2, 2)).astype(np.float32)
    trans = (integer(U + 3, (C, C), -1, 1) + continuous(U + 4, C, C) * (rng.random((C, 1)) < 0.5)).astype(np.float32)
    return Case(em, trans, integer(U + 5, (C,), -1, 1), tokens, lengths, None, U)


WORD_FRAMES = (1, 31, 32, 33, 63, 64, 65, 129)


def _word_case():
    """every T_b at which the last word of a row, or the 64 frames of a store, is full, one short or one over, with
    hypotheses of about 7 labels, of one label and of as many as fit"""
    rng = np.random.default_rng(11)
    C, M = 5, 129
    hyps = []
    for T in WORD_FRAMES:
        hyps += [labels_of(rng, min(T, 7), C), labels_of(rng, 1, C), labels_of(rng, min(T, 40), C), labels_of(rng, min(T, 6), C, 0.0)]
    tokens, lengths = pack(hyps, len(WORD_FRAMES), 4, 40)
    em, trans, start = model(12, len(WORD_FRAMES), M, C)
    return Case(em, trans, start, tokens, lengths, np.asarray(WORD_FRAMES, np.int32), 40)


DESCENT_LENS = (32, 33, 64, 65, 129)


def _descent_case():
    """T_b == len: one position a frame, the 32-position reach of a word row; random labels and one label throughout"""
    rng = np.random.default_rng(13)
    C = 6
    hyps = []
    for n in DESCENT_LENS:
        hyps += [labels_of(rng, n, C), np.full(n, 2, np.int32)]
    tokens, lengths = pack(hyps, len(DESCENT_LENS), 2, 129)
    em, trans, start = model(14, len(DESCENT_LENS), 129, C)
    return Case(em, trans, start, tokens, lengths, np.asarray(DESCENT_LENS, np.int32), 129)


STEADY_FRAMES = (100, 37, 64, 1)


def _steady_case():
    """len == 1: one label held for all frames, the path never descends"""
    rng = np.random.default_rng(15)
    C = 4
    hyps = [labels_of(rng, 1, C) for _ in STEADY_FRAMES]
    tokens, lengths = pack(hyps, len(STEADY_FRAMES), 1, 3)
    em, trans, start = model(16, len(STEADY_FRAMES), 100, C)
    return Case(em, trans, start, tokens, lengths, np.asarray(STEADY_FRAMES, np.int32), 3)


TIE_LENS = (5, 40, 200)


def _ties_case(ones):
    """all-zero, or {0, 1}, emissions and table; hypotheses with equal neighbours: every maximum is a tie somewhere"""
    rng = np.random.default_rng(17 + ones)
    C, T = 4, 300
    hyps = [labels_of(rng, n, C, 0.5) for _ in range(2) for n in TIE_LENS]
    tokens, lengths = pack(hyps, 2, 3, 200)
    if ones:
        em, trans, start = integer(18, (2, T, C), 0, 1), integer(19, (C, C), 0, 1), integer(20, (C,), 0, 1)
    else:
        em, trans, start = np.zeros((2, T, C), np.float32), np.zeros((C, C), np.float32), np.zeros(C, np.float32)
    return Case(em, trans, start, tokens, lengths, np.asarray([T, T - 20], np.int32), 200)


ALIGN_LENS = (1, 64, 128, 511)  # U + 1 nodes of the existing aligner: 2, 65, 129, 512


def _align_case(C, zero=False):
    """what asg_forced_align's launch takes too: C a multiple of 4, at most 511 labels"""
    rng = np.random.default_rng(21 + C)
    T = 520
    hyps = [labels_of(rng, n, C) for n in ALIGN_LENS]
    frames = np.asarray([9, 64, T, T - 3], np.int32)
    tokens, lengths = pack(hyps, len(ALIGN_LENS), 1, 511)
    em, trans, start = model(22 + C, len(ALIGN_LENS), T, C)
    if zero:
        em, trans, start = np.zeros_like(em), np.zeros_like(trans), np.zeros_like(start)
    return Case(em, trans, start, tokens, lengths, frames, 511)


NOPATH_FRAMES = (30, 0, 9, 30, 30, 12, 30, 30)


def _nopath_case(pad=np.nan, garbage=None):
    """pairs without a path next to good ones, every kind.  Utterance 1 has no frames; 2 has one frame too few for its
    first hypothesis and exactly enough for its second; in 3 a -inf emission column cuts every path through label 3; 4
    carries tokens that are no label (at position 0, where only the owner sees it, and further on, where the position
    behind gathers through it) and lengths outside 0 .. L; 5 has a hypothesis above max_length; in 6 a -inf transition
    (label 4 followed by label 3) and in 7 a -inf start entry (label 5) cut their paths.  `pad` fills the emission rows
    from T_b on, `garbage` the token elements from each length on"""
    rng = np.random.default_rng(23)
    C, M, L, N = 7, 30, 12, 4
    B = len(NOPATH_FRAMES)
    em, trans, start = model(24, B, M, C)
    hyps = [[labels_of(rng, n, C) for n in (3, 8, 0, 11)] for _ in range(B)]
    hyps[2][0] = labels_of(rng, 10, C)                          # needs 10 frames, has 9
    hyps[2][1] = labels_of(rng, 9, C)                           # fits exactly
    hyps[2][3] = labels_of(rng, 11, C)                          # too long again
    em[3, :, 3] = -np.inf
    hyps[3][0] = np.asarray([2, 3, 2], np.int32)                # through label 3: cut
    hyps[3][1] = np.asarray([2, 4, 2, 5], np.int32)             # spared
    hyps[3][3] = np.asarray([0, 1, 2, 4, 5, 6, 0, 1, 2, 4, 5], np.int32)
    hyps[4][0] = np.asarray([-1, 2, 3], np.int32)
    hyps[4][1] = np.asarray([2, C, 3], np.int32)
    hyps[5][3] = labels_of(rng, 12, C)                          # fits 12 frames, but lies above max_length 11
    trans[3, 4] = -np.inf
    start[5] = -np.inf
    for b in range(B):                                          # (the two holes touch utterances 6 and 7 only)
        for k in range(N):
            y = hyps[b][k]
            if b not in (4, 6, 7) and len(y):
                y[y == 5] = 6
                for i in range(1, len(y)):
                    if y[i - 1] == 4 and y[i] == 3:
                        y[i] = 2
    hyps[6][0] = np.asarray([1, 4, 3, 0], np.int32)             # 4 -> 3: cut
    hyps[6][1] = np.asarray([1, 3, 4, 0], np.int32)             # 3 -> 4: spared
    hyps[6][3] = np.asarray([4, 4, 3, 3], np.int32)             # cut
    hyps[7][0] = np.asarray([5, 1, 2], np.int32)                # starts in label 5: cut
    hyps[7][1] = np.asarray([1, 5, 2], np.int32)                # label 5 later: spared
    hyps[7][3] = np.asarray([5], np.int32)                      # cut
    tokens, lengths = pack([h for u in hyps for h in u], B, N, L)
    lengths[4, 2] = -3     # (counts as 0: no path)
    lengths[4, 3] = L + 5  # (counts as L, which is above max_length)
    if garbage is not None:
        past = np.arange(L)[None, None, :] >= np.clip(lengths, 0, L)[:, :, None]
        tokens[past] = np.random.default_rng(garbage).integers(-5, 10 ** 6, int(past.sum()))
    for b, f in enumerate(NOPATH_FRAMES):
        em[b, f:] = pad
    return Case(em, trans, start, tokens, lengths, np.asarray(NOPATH_FRAMES, np.int32), 11)


ALPHABETS = (1, 2, 5, 33, 257, 300)


def _alphabet_case(C):
    rng = np.random.default_rng(40 + C)
    B, N, L, T = 2, 3, 20, 30
    hyps = [labels_of(rng, int(n), C) for n in rng.integers(1, L + 1, B * N)]
    tokens, lengths = pack(hyps, B, N, L)
    em, trans, start = model(41 + C, B, T, C)
    return Case(em, trans, start, tokens, lengths, np.asarray([T, 21], np.int32), None)


def _flat_case():
    """N == 1, the [B, L] form"""
    rng = np.random.default_rng(29)
    C, T = 9, 50
    hyps = [labels_of(rng, n, C) for n in (4, 0, 17, 30, 9)]
    tokens, lengths = pack(hyps, 5, 1, 30)
    lengths[1, 0] = -7  # (counts as 0)
    lengths[3, 0] = 35  # (counts as L = 30, the hypothesis's length)
    em, trans, start = model(30, 5, T, C)
    return Case(em, trans, start, tokens, lengths, np.asarray([50, 3, 40, 50, 9], np.int32), None)


def _slices_case():
    rng = np.random.default_rng(31)
    C, T = 10, 70
    hyps = [labels_of(rng, int(n), C) for n in rng.integers(0, 30, 12)]
    tokens, lengths = pack(hyps, 4, 3, 32)
    em = integer(32, (4, T, C), -1, 1)
    return Case(em, integer(33, (C, C), -1, 1), integer(34, (C,), -1, 1), tokens, lengths,
                np.asarray([70, 33, 64, 17], np.int32), 32)


BUILDERS = {f"width-{U}": functools.partial(_width_case, U) for U in WIDTHS}
BUILDERS.update({
    "words": _word_case,
    "descent": _descent_case,
    "steady": _steady_case,
    "ties-zero": functools.partial(_ties_case, 0),
    "ties-01": functools.partial(_ties_case, 1),
    "align-c8": functools.partial(_align_case, 8),
    "align-c300": functools.partial(_align_case, 300),
    "align-c8-zero": functools.partial(_align_case, 8, True),
    "nopath": _nopath_case,
    "flat": _flat_case,
    "slices": _slices_case,
})
BUILDERS.update({f"alphabet-{C}": functools.partial(_alphabet_case, C) for C in ALPHABETS})
ALL_GPU_CASES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def result(name):
    """the Result of a named case, computed once per process and left unchanged"""
    return evaluate(case(name))
