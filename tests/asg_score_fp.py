"""ASG force-align scores of given hypotheses and their weighted gradients (TEST INFRASTRUCTURE ONLY).

Three things live here, shared by test_asg_score_cpu.py and test_asg_score_gpu.py:
  * the float64 yardstick: tests/asg_loss_fp.py: fal_fp64 (imported, not copied) per pair, summed under the weights;
  * a float32 transcription of gtn_amd/csrc/asg_score.hip: the same recurrences with float32 arithmetic in the kernel's
    order of sums (a token's chain by ascending index; the pairs of an utterance in k order; the occupancy sums over the
    frames from the last frame down; the table entries over the pairs in p order and the positions ascending, a
    position's self sum before its step sum), so that the float32 error of the METHOD can be measured against the gates
    before a GPU is involved;
  * the generated cases, computed once per process and left unchanged.
The contract: len = clamp(length, 0, L); -inf when len == 0, T_b < len, len > max_length, a token
inside the length outside 0 .. C - 1, or no alignment stays above -inf; a -inf score or a weight of exactly 0 adds
nothing to either gradient.
"""
import collections
import functools

import numpy as np

from asg_loss_fp import fal_fp64

NEG = -np.inf
SCORE_GATE = 1e-4  # * max(1, |score|)
GRAD_GATE = 1e-4   # absolute, weights in [-1, 1]
TABLE_GATE = 1e-4  # * max(1, |want|) per entry: an entry is a sum over pairs and frames
MAX_U, MAX_C = 4096, 16384
# asg_score_config of asg_score.hip: max_length up to the bound -> (workgroup width, positions per lane)
CONFIGS = ((64, (64, 1)), (256, (256, 1)), (768, (256, 3)), (1024, (1024, 1)), (2048, (1024, 2)), (4096, (1024, 4)))


def config(U):
    for bound, cfg in CONFIGS:
        if U <= bound:
            return cfg
    raise ValueError(U)


def table_of(start, trans):
    """[C + C * C] in the arc order of asgTransitions: start, then entry C + i * C + j = trans[i, j]"""
    return np.concatenate([np.asarray(start, np.float32).reshape(-1), np.asarray(trans, np.float32).reshape(-1)])


def hypothesis(tokens_row, length, L, C, max_length):
    """the hypothesis the contract reads out of a row, or None when the pair scores -inf by its tokens or length"""
    n = min(max(int(length), 0), L)
    if n == 0 or n > max_length:
        return None
    y = np.asarray(tokens_row[:n], dtype=np.int64)
    if ((y < 0) | (y >= C)).any():
        return None
    return y


# ---- float32, as the kernel does it ----
def logadd32(x, y):
    """m + log1p(exp(n - m)) in float32, the -inf cases explicit"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    m, n = np.maximum(x, y), np.minimum(x, y)
    with np.errstate(invalid="ignore", over="ignore"):
        r = (m + np.log1p(np.exp(n - m, dtype=np.float32), dtype=np.float32)).astype(np.float32)
    return np.where(x == NEG, y, np.where(y == NEG, x, r)).astype(np.float32)


def gathered(table, y, C):
    """(w_self, w_step) of the positions of y, float32"""
    y = np.asarray(y, np.int64)
    w_self = table[C + y * C + y]
    w_step = np.concatenate([table[y[:1]], table[C + y[1:] * C + y[:-1]]])
    return w_self.astype(np.float32), w_step.astype(np.float32)


def _down(a, fill):
    """a[i - 1], `fill` at position 0"""
    return np.concatenate([np.array([fill], dtype=a.dtype), a[:-1]])


def forward_f32(em, y, table):
    """(score, alpha [T, len]) in float32: the kernel's recurrence"""
    T, C = em.shape
    x = np.asarray(em, dtype=np.float32)
    w_self, w_step = gathered(table, y, C)
    n = len(y)
    P = np.full((T, n), NEG, dtype=np.float32)
    P[0, 0] = w_step[0] + x[0, y[0]]
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            prev = P[t - 1]
            a = logadd32(prev + w_self, _down(prev, np.float32(NEG)) + w_step)
            P[t] = a + x[t, y]
    return np.float32(P[T - 1, n - 1]), P


def backward_f32(grad, em, y, table, w, score, P):
    """adds w * d score / d em into grad [T, C] (float32) in the kernel's order; returns the pair's occupancy sums
    (w * sum_t p_self [len], w * sum_t p_step [len]), float32"""
    T, C = em.shape
    x = np.asarray(em, dtype=np.float32)
    y = np.asarray(y, np.int64)
    n = y.size
    w_self, w_step = gathered(table, y, C)
    # the chains of equal tokens, ascending index: rounds[r] = (heads that have an r-th follower, that follower)
    chains = collections.OrderedDict()
    for i, v in enumerate(y.tolist()):
        chains.setdefault(v, []).append(i)
    lists = list(chains.values())
    heads = np.array([c[0] for c in lists], dtype=np.int64)
    head_lab = np.array(list(chains.keys()), dtype=np.int64)
    rounds = []
    for r in range(1, max(len(c) for c in lists)):
        sel = [h for h, c in enumerate(lists) if len(c) > r]
        rounds.append((np.array(sel, dtype=np.int64), np.array([lists[h][r] for h in sel], dtype=np.int64)))
    beta = np.full(n, NEG, dtype=np.float32)
    beta[n - 1] = 0.0
    w, sc = np.float32(w), np.float32(score)
    sum_self = np.zeros(n, dtype=np.float32)
    sum_step = np.zeros(n, dtype=np.float32)
    first = np.full(n, NEG, dtype=np.float32)
    first[0] = 0.0  # (the start, before frame 0)
    none = np.full(n, NEG, dtype=np.float32)
    zero = np.float32(0)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T - 1, -1, -1):
            a_self = P[t - 1] if t else none
            a_prev = _down(P[t - 1], np.float32(NEG)) if t else first
            q = beta + x[t, y]
            xs = (a_self + w_self) + q
            xp = (a_prev + w_step) + q
            ps = np.where(xs > NEG, np.exp(xs - sc, dtype=np.float32), zero)
            pt = np.where(xp > NEG, np.exp(xp - sc, dtype=np.float32), zero)
            sum_self = sum_self + ps
            sum_step = sum_step + pt
            g = ps + pt
            sums = g[heads].copy()
            for sel, follower in rounds:
                sums[sel] = sums[sel] + g[follower]
            grad[t, head_lab] = grad[t, head_lab] + w * sums
            m = q + w_step
            beta = logadd32(q + w_self, np.concatenate([m[1:], np.array([NEG], dtype=np.float32)]))
    return w * sum_self, w * sum_step


def table_f32(acc, y, C, occ_self, occ_step):
    """adds a pair's occupancy sums into acc [C + C * C] (float32) in the table kernel's order: the positions ascending,
    a position's self sum first, then its step sum (every row of the table has a workgroup of its own, so the order
    within a row is all that counts; np.add.at adds one element after the other)"""
    y = np.asarray(y, np.int64)
    idx = np.empty(2 * y.size, dtype=np.int64)
    val = np.empty(2 * y.size, dtype=np.float32)
    idx[0::2] = C + y * C + y
    idx[1::2] = np.concatenate([y[:1], C + y[1:] * C + y[:-1]])
    val[0::2] = occ_self
    val[1::2] = occ_step
    np.add.at(acc, idx, val)


# ---- a batch, both ways ----
Case = collections.namedtuple("Case", "em trans start tokens lengths frames max_length weights")
Result = collections.namedtuple("Result", "scores grad gtable scores32 grad32 gtable32")


def default_max_length(case):
    return max(1, min(case.tokens.shape[-1], case.em.shape[1], MAX_U))


def max_length_of(case):
    return case.max_length if case.max_length is not None else default_max_length(case)


def evaluate(case, f32=True):
    """Result of a case: float64 scores [B, N], emission gradient [B, T, C] and table gradient [C + C * C], and the
    float32 transcription's"""
    em = case.em
    B, T, C = em.shape
    tokens = case.tokens.reshape(B, -1, case.tokens.shape[-1])
    N, L = tokens.shape[1:]
    lengths = np.asarray(case.lengths).reshape(B, N)
    weights = np.asarray(case.weights, dtype=np.float32).reshape(B, N)
    U = max_length_of(case)
    table = table_of(case.start, case.trans)
    scores = np.full((B, N), NEG)
    grad = np.zeros((B, T, C))
    gtable = np.zeros(C + C * C)
    scores32 = np.full((B, N), NEG, dtype=np.float32)
    grad32 = np.zeros((B, T, C), dtype=np.float32)
    gtable32 = np.zeros(C + C * C, dtype=np.float32)
    for b in range(B):
        Tb = T if case.frames is None else int(case.frames[b])
        x = em[b, :Tb]
        for k in range(N):
            y = hypothesis(tokens[b, k], lengths[b, k], L, C, U)
            if y is None or Tb < y.size:
                continue
            z, g_em, g_tr = fal_fp64(x, case.trans, case.start, y)
            if np.isnan(z):
                z = NEG
            scores[b, k] = z
            if np.isfinite(z) and weights[b, k] != 0:
                grad[b, :Tb] += float(weights[b, k]) * g_em
                gtable += float(weights[b, k]) * g_tr
            if f32:
                z32, alpha = forward_f32(x, y, table)
                scores32[b, k] = z32
                if z32 > NEG and weights[b, k] != 0:
                    occ = backward_f32(grad32[b, :Tb], x, y, table, weights[b, k], z32, alpha)
                    table_f32(gtable32, y, C, *occ)
    return Result(scores, grad, gtable, scores32, grad32, gtable32)


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


def table_err(got, want):
    """the largest error of an entry in units of max(1, |want|)"""
    d = np.abs(np.asarray(got, np.float64) - want) / np.maximum(1.0, np.abs(want))
    return float(np.max(d, initial=0.0)) if np.isfinite(d).all() else np.inf


# ---- the cases ----
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


def model_of(rng, B, T, C, sigma=0.5):
    """emissions [B, T, C], transitions [C, C] and start [C] around 0, not normalised (any scores are emissions)"""
    return (rng.normal(0.0, sigma, (B, T, C)).astype(np.float32), rng.normal(0.0, sigma, (C, C)).astype(np.float32),
            rng.normal(0.0, sigma, C).astype(np.float32))


def _edges_case(max_length=None):
    """C = 5, T = 9, L = 8: the contract's edges one per slot"""
    C, T, L = 5, 9, 8
    rng = np.random.default_rng(99)
    em, trans, start = model_of(rng, 3, T, C)
    trans[3, 4] = NEG  # label 4 followed by label 3 is forbidden
    tokens = np.full((3, 4, L), -1, dtype=np.int32)
    lengths = np.zeros((3, 4), dtype=np.int32)

    def put(b, k, row, n):
        tokens[b, k, :len(row)] = row
        lengths[b, k] = n
    put(0, 0, [1, 1, 1], 3)                  # a run of equal tokens
    put(0, 1, [0, 1, 0, 1], 4)               # a bigram that repeats inside one hypothesis
    put(0, 2, [], 0)                         # length 0: no score
    put(0, 3, [2], 1)                        # length 1
    put(1, 0, [1, -1, 3], 3)                 # -1 inside the length
    put(1, 1, [1, 5, 3], 3)                  # C inside the length
    put(1, 2, [0, 1], 2)                     # length 2; the bigram 0 -> 1 of (0, 1), another utterance
    put(1, 3, [3, 0, 1, 4], 4)               # ... and in another k of this one
    put(2, 0, [0, 1, 2], 3)
    put(2, 1, [2, 4, 3], 3)                  # crosses the -inf table entry: killed
    put(2, 2, [2, 3, 4], 3)                  # the same labels the other way round: spared
    put(2, 3, [0, 1, 3, 4, 0, 1, 3, 2], 100)  # a length above L: the row's width counts
    w = weights_of(rng, 3, 4)
    w[0, 2] = 0.0  # an exact 0 on a -inf pair
    w[2, 0] = 0.0  # ... and on a finite one
    return Case(em, trans, start, tokens, lengths, None, max_length, w)


FRAMES_LEN = 5
FRAMES = (5, 6, 4, 0, 9, 1)


def _frames_case(pad=np.nan):
    """T_b == len (one alignment), len + 1, len - 1, 0, T and 1 against hypotheses of 5 labels (k = 0) and of 1 (k = 1);
    the pad rows filled with `pad`"""
    rng = np.random.default_rng(77)
    B, N, L, T, C = 6, 2, 6, 9, 4
    em, trans, start = model_of(rng, B, T, C)
    for b, f in enumerate(FRAMES):
        em[b, f:] = pad
    hyps = []
    for b in range(B):
        hyps += [rng.integers(0, C, FRAMES_LEN), rng.integers(0, C, 1)]
    tokens, lengths = pack(hyps, B, N, L)
    return Case(em, trans, start, tokens, lengths, FRAMES, None, weights_of(rng, B, N))


def _random_case(C, seed, B=3, N=4, L=24, T=40, holes=0.0, lengths_dtype=np.int32, start=True):
    rng = np.random.default_rng(seed)
    em, trans, st = model_of(rng, B, T, C)
    if holes:
        em[rng.random(em.shape) < holes] = NEG
        trans[rng.random(trans.shape) < holes / 2] = NEG
    hyps = [rng.integers(0, C, int(n)) for n in rng.integers(0, L + 1, B * N)]
    tokens, lengths = pack(hyps, B, N, L, lengths_dtype)
    return Case(em, trans, st if start else np.zeros(C, np.float32), tokens, lengths, None, None, weights_of(rng, B, N))


# max_length -> the lengths of the hypotheses (one utterance each, T_b = len + 1): one below, at and one above the wave
# and every workgroup width, the multiples of the width where a lane owns several positions, max_length itself and
# max_length + 1 (which scores -inf: the rows are one wider than max_length)
WIDE = {64: (63, 64, 65), 65: (65, 64), 256: (255, 256, 257), 257: (257, 256), 768: (513, 768, 769, 512),
        769: (769,), 1024: (1023, 1024, 1025), 1025: (1025,), 2048: (2047, 2048, 2049), 2049: (2049,), 4096: (4096, 3073, 3072, 4097)}


def _wide_case(U):
    """Values of a small spread keep |alpha| within tens over thousands of frames, where an ulp is 2e-6: a float32
    log-domain recursion of sqrt(2 T) roundings then stays well inside 1e-4 on an occupancy.  33 labels keep the chains
    of equal tokens near len / 33."""
    rng = np.random.default_rng(U)
    lens = WIDE[U]
    B, C = len(lens), 33
    hyps = [rng.integers(0, C, n) for n in lens]
    frames = tuple(n + 1 for n in lens)
    T = max(frames)
    em, trans, start = model_of(rng, B, T, C, sigma=0.05)
    for b, f in enumerate(frames):
        em[b, f:] = np.nan
    tokens, lengths = pack(hyps, B, 1, U + 1)
    return Case(em, trans, start, tokens, lengths, frames, U, weights_of(rng, B, 1))


BUILDERS = {
    "edges": _edges_case,
    "edges-u7": lambda: _edges_case(7),      # the row of 8 labels is above max_length
    "frames": _frames_case,
    "c4": lambda: _random_case(4, 4, start=False),
    "c5-holes": lambda: _random_case(5, 7, B=4, N=3, L=12, T=30, holes=0.05),  # -inf emissions and a -inf transition
    "c33": lambda: _random_case(33, 33, B=2, N=4, L=60, T=80, lengths_dtype=np.int64),
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
