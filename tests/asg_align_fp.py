"""A float64 numpy Viterbi over the ASG force-alignment trellis: the yardstick of the ASG forced-alignment tests.

The trellis is the product the reference builds from compose(forceAlign(target), transitions) (examples/asg.cpp:50-68)
and a linear emission graph: node n of U + 1 means "the first n labels are consumed"; a frame enters node n >= 1 from n
itself (weight trans[l, l] with l = target[n - 1]) or from n - 1 (weight trans[l, target[n - 2]], the start weight
start[l] for n = 1), and emits em[t, l].  Paths start at node 0 and end at node U.

Exact ties: of two equal candidates the STEP (from n - 1) wins.  That is the reference's viterbiPath on the built
lattice -- node n - 1 leaves the queue before node n in every layer and only a strictly greater candidate replaces the
first one -- and tests/test_asg_align_cpu.py pins it to the oracle on integer-valued inputs.
"""
import numpy as np


# (seed, B, T, N labels, Umax, ragged frames) of seeded_case(): continuous inputs.  tests/test_asg_align_cpu.py pins
# asg_align_fp64 to the oracle on these, tests/test_asg_align_gpu.py judges the entry points by it on the same ones
FP_CASES = [(5, 6, 40, 12, 9, False), (6, 4, 75, 32, 20, True), (7, 3, 120, 8, 40, True)]

# (seed, B, T max, U max, labels, share of repeated labels, kind) of tie_case(): integer-valued inputs, exact ties
# everywhere.  kind: "zero" all weights 0, "01" 0/1 emissions and zero transitions, "int" small-integer emissions,
# transitions and start weights
TIE_CASES = [
    (101, 12, 10, 5, 2, 0.5, "zero"),
    (102, 12, 10, 5, 3, 0.3, "01"),
    (103, 12, 12, 5, 5, 0.3, "int"),
    (104, 8, 60, 40, 2, 0.7, "01"),
    (105, 8, 60, 40, 8, 0.0, "int"),
    (106, 8, 33, 20, 4, 0.7, "int"),
    (107, 6, 60, 40, 8, 0.4, "zero"),
    (108, 8, 17, 16, 3, 0.5, "int"),
]


def asg_align_fp64(em, trans, start, target, frames=None):
    """em [T, N]; trans [N, N] with trans[i, j] the score of label j followed by label i; start [N]; returns
    (labels [T] int32, tokens [T] int32, score float64).  The first `frames` rows are aligned and entries past them
    are -1; without an accepting path (fewer frames than labels; no labels but a frame): rows of -1 and score -inf.
    tokens[t] is the index into `target` of frame t's label -- never -1 inside a path."""
    em = np.asarray(em, dtype=np.float64)
    trans = np.asarray(trans, dtype=np.float64)
    start = np.asarray(start, dtype=np.float64)
    T_full = em.shape[0]
    T = T_full if frames is None else int(frames)
    target = np.asarray([int(x) for x in target], dtype=np.int64)
    U = len(target)
    labels = np.full(T_full, -1, np.int32)
    tokens = np.full(T_full, -1, np.int32)
    ninf = -np.inf
    if U == 0:
        return labels, tokens, (0.0 if T == 0 else ninf)
    if T < U:
        return labels, tokens, ninf
    w_self = trans[target, target]                                   # into node n = 1 .. U from itself
    w_step = np.concatenate(([start[target[0]]], trans[target[1:], target[:-1]]))  # ... from node n - 1
    alpha = np.full(U + 1, ninf)
    alpha[0] = 0.0
    bp = np.zeros((T, U + 1), dtype=np.int8)
    for t in range(T):
        e = em[t, target]
        c0 = alpha[1:] + (w_self + e)
        c1 = alpha[:-1] + (w_step + e)
        k = c1 >= c0  # the step wins exact ties
        bp[t, 1:] = k
        alpha = np.concatenate(([ninf], np.where(k, c1, c0)))
    if not np.isfinite(alpha[U]):
        return labels, tokens, ninf
    node = U
    for t in range(T - 1, -1, -1):
        labels[t] = target[node - 1]
        tokens[t] = node - 1
        node -= int(bp[t, node])
    assert node == 0
    return labels, tokens, float(alpha[U])


def seeded_case(seed, B, T, N, Umax, ragged_frames=False):
    """continuous random inputs, targets with repeats, every utterance feasible in its frame count:
    (em float32 [B, T, N], trans float32 [N, N], start float32 [N], targets, frames int32 [B])"""
    rng = np.random.default_rng(seed)
    em = rng.normal(0, 2, (B, T, N)).astype(np.float32)
    trans = rng.normal(0, 1, (N, N)).astype(np.float32)
    start = rng.normal(0, 1, N).astype(np.float32)
    targets, frames = [], []
    for _ in range(B):
        t = rng.integers(0, N, int(rng.integers(1, min(Umax, T) + 1))).tolist()
        targets.append(t)
        frames.append(int(rng.integers(len(t), T + 1)) if ragged_frames else T)
    return em, trans, start, targets, np.asarray(frames, np.int32)


def tie_case(seed, B, Tmax, Umax, nlab, rep, kind, N=None):
    """integer-valued utterances of one alphabet (N >= nlab columns, labels drawn from the first nlab), each of its
    own length: a list of (em float32 [T, N], target) and the shared (trans [N, N], start [N])"""
    rng = np.random.default_rng(seed)
    N = nlab if N is None else N
    if kind == "int":
        trans = rng.integers(-1, 2, (N, N)).astype(np.float32)
        start = rng.integers(-1, 2, N).astype(np.float32)
    else:
        trans = np.zeros((N, N), np.float32)
        start = np.zeros(N, np.float32)
    utts = []
    for _ in range(B):
        U = int(rng.integers(1, Umax + 1))
        T = int(rng.integers(U, Tmax + 1))
        t = [int(rng.integers(0, nlab))]
        while len(t) < U:
            t.append(t[-1] if rng.random() < rep else int(rng.integers(0, nlab)))
        if kind == "zero":
            em = np.zeros((T, N), np.float32)
        elif kind == "01":
            em = rng.integers(0, 2, (T, N)).astype(np.float32)
        else:
            em = rng.integers(-2, 3, (T, N)).astype(np.float32)
        utts.append((em, t))
    return utts, trans, start


def tokens_from_labels(labels, target):
    """the token row that `labels` determines, or None where it does not (adjacent equal labels in the target: a
    run of that label can be cut in more than one place)"""
    target = list(target)
    if any(target[i] == target[i - 1] for i in range(1, len(target))):
        return None
    out, n = [], -1
    for i, l in enumerate(labels):
        if i == 0 or l != labels[i - 1]:
            n += 1
        out.append(n)
    return out
