"""A float64 numpy Viterbi over emissions o (ASG transitions): the yardstick of the ASG decode tests.

The product the reference builds from a linear emission graph and the transitions graph of examples/asg.cpp:36-47 is the
full-connect trellis: after frame t the path sits on label i with

    alpha_0[i] = start[i] + em[0, i]
    alpha_t[i] = max_j(alpha_{t-1}[j] + trans[i, j]) + em[t, i]

Exact ties: of equal maxima the SMALLEST j wins, and of equal final scores the smallest label.  That is the reference's
viterbiPath on the built lattice -- the label nodes of a layer leave its queue in node order, and only a strictly
greater candidate replaces the first one -- and tests/test_asg_decode_cpu.py pins it to the oracle on integer-valued
inputs, in both argument orders, transitions arc-sorted and not.
"""
import numpy as np


# (seed, T, N labels) of seeded_case(): continuous inputs, one utterance each.  tests/test_asg_decode_cpu.py pins
# asg_decode_fp64 to the oracle on these
FP_CASES = [(11, 1, 2), (12, 2, 3), (13, 3, 5), (14, 7, 8), (15, 13, 4), (16, 9, 7), (17, 12, 6), (18, 5, 2)]

# kinds of tie_case(): "zero" all weights 0, "01" 0/1 emissions and zero transitions, "int" small-integer emissions,
# transitions and start weights
TIE_KINDS = ("zero", "01", "int")
# (seed, T, N labels, kind): N = 2 .. 8, T = 1 .. 13, every kind at every N
TIE_CASES = [(200 + k, 1 + (5 * k + k // 13) % 13, 2 + k % 7, TIE_KINDS[(k // 7) % 3]) for k in range(63)]


def collapse(labels):
    """runs of equal consecutive labels merged"""
    out = []
    for x in labels:
        if not out or out[-1] != x:
            out.append(int(x))
    return out


def asg_decode_fp64(em, trans, start, frames=None, dtype=np.float64):
    """em [T, N]; trans [N, N] with trans[i, j] the score of label j followed by label i; start [N]; returns
    (labels [T] int32, score, collapsed list).  The first `frames` rows are decoded and entries past them are -1;
    without a frame: rows of -1, score -inf, nothing collapsed.
    dtype=np.float32 evaluates the same recursion in the association the device uses -- fl(fl(alpha + w) + e), the
    maximum taken over fl(alpha + w) (rounding is monotone: the same winner) -- to vet continuous seeds on the host."""
    em = np.asarray(em, dtype=dtype)
    trans = np.asarray(trans, dtype=dtype)
    start = np.asarray(start, dtype=dtype)
    T_full, N = em.shape
    T = T_full if frames is None else int(frames)
    labels = np.full(T_full, -1, np.int32)
    if T < 1:
        return labels, -np.inf, []
    alpha = (start + em[0]).astype(dtype)
    bp = np.zeros((T, N), np.int64)
    for t in range(1, T):
        cand = (alpha[None, :] + trans).astype(dtype)   # [i, j]
        x = (cand + em[t][:, None]).astype(dtype)       # the comparison the back-trace makes
        bp[t] = np.argmax(x, axis=1)                    # first maximum = smallest j
        alpha = x[np.arange(N), bp[t]]
    node = int(np.argmax(alpha))                        # first maximum = smallest label
    score = float(alpha[node])
    if not score > -np.inf:
        return labels, -np.inf, []
    for t in range(T - 1, -1, -1):
        labels[t] = node
        node = int(bp[t, node])
    return labels, score, collapse(labels[:T])


def seeded_case(seed, T, N, B=None):
    """continuous random inputs: (em float32 [T, N] -- or [B, T, N] --, trans float32 [N, N], start float32 [N])"""
    rng = np.random.default_rng(seed)
    em = rng.normal(0, 2, (T, N) if B is None else (B, T, N)).astype(np.float32)
    trans = rng.normal(0, 1, (N, N)).astype(np.float32)
    start = rng.normal(0, 1, N).astype(np.float32)
    return em, trans, start


def tie_case(seed, T, N, kind, B=None):
    """integer-valued inputs, exact ties everywhere: (em float32 [T, N] -- or [B, T, N] --, trans [N, N], start [N])"""
    rng = np.random.default_rng(seed)
    shape = (T, N) if B is None else (B, T, N)
    if kind == "int":
        trans = rng.integers(-1, 2, (N, N)).astype(np.float32)
        start = rng.integers(-1, 2, N).astype(np.float32)
    else:
        trans = np.zeros((N, N), np.float32)
        start = np.zeros(N, np.float32)
    if kind == "zero":
        em = np.zeros(shape, np.float32)
    elif kind == "01":
        em = rng.integers(0, 2, shape).astype(np.float32)
    else:
        em = rng.integers(-2, 3, shape).astype(np.float32)
    return em, trans, start


def float32_agrees(em, trans, start, frames=None):
    """True when the recursion in the device's float32 association picks the float64 path on this utterance -- the test
    a continuous seed has to pass BEFORE it is used on the device (a seed that fails is replaced, not tolerated)"""
    a = asg_decode_fp64(em, trans, start, frames)
    b = asg_decode_fp64(em, trans, start, frames, dtype=np.float32)
    return bool((a[0] == b[0]).all())
