"""A float64 numpy Viterbi over the CTC trellis: the third implementation the forced-alignment tests lean on.

The trellis is the product the reference builds from ctcGraph(target) (benchmarks/ctc.cpp:40-58) and a linear
emission graph: node m of 2U+1 carries the blank (m even) or label (m-1)/2 (m odd); a frame enters node m from m
itself, from m-1, and -- for a label node whose label differs from the previous label -- from m-2; paths start at
node 0 and end at one of the last two nodes.  Of equal candidates the FIRST in the order (m, m-1, m-2) wins and of
equal end nodes the smaller, which is not the reference's rule for exact ties: use it on continuous random inputs
only (tests/test_align_cpu.py pins it to the oracle on such inputs).
"""
import numpy as np


# (seed, B, T, C, Umax, ragged frames) of seeded_case(): tests/test_align_cpu.py pins ctc_align_fp64 to the oracle on
# these, tests/test_align_gpu.py judges the torch entry point by it on the same ones
FP_CASES = [(5, 6, 40, 12, 9, False), (6, 4, 75, 32, 20, True), (7, 3, 120, 8, 40, True)]


def repeats(target):
    """adjacent equal labels: a blank frame is forced between them"""
    return sum(1 for i in range(1, len(target)) if target[i] == target[i - 1])


def min_frames(target):
    """a CTC path for `target` exists in exactly the frame counts >= this"""
    return len(target) + repeats(target)


def ctc_align_fp64(em, target, blank=0, frames=None):
    """em [T, C]; returns (labels [T] int32, tokens [T] int32, score float64); the first `frames` rows are aligned
    and entries past them are -1; without a path: rows of -1 and score -inf"""
    em = np.asarray(em, dtype=np.float64)
    T_full = em.shape[0]
    T = T_full if frames is None else int(frames)
    target = [int(x) for x in target]
    U = len(target)
    N = 2 * U + 1
    lab = np.array([target[(m - 1) // 2] if m % 2 else blank for m in range(N)], dtype=np.int64)
    skip = np.zeros(N, dtype=bool)
    for m in range(3, N, 2):
        skip[m] = target[(m - 1) // 2] != target[(m - 3) // 2]
    labels = np.full(T_full, -1, np.int32)
    tokens = np.full(T_full, -1, np.int32)
    ninf = -np.inf
    alpha = np.full(N, ninf)
    alpha[0] = 0.0
    bp = np.zeros((T, N), dtype=np.int8)
    for t in range(T):
        e = em[t, lab]
        c0 = alpha
        c1 = np.concatenate(([ninf], alpha[:-1]))
        c2 = np.where(skip, np.concatenate(([ninf, ninf], alpha[:-2])), ninf)
        cand = np.stack([c0, c1, c2])
        k = np.argmax(cand, axis=0)  # (first maximum)
        bp[t] = k
        alpha = cand[k, np.arange(N)] + e
    ends = [N - 1] if N == 1 else [N - 2, N - 1]
    best = max(alpha[m] for m in ends)
    if not np.isfinite(best):
        return labels, tokens, ninf
    node = min(m for m in ends if alpha[m] == best)
    for t in range(T - 1, -1, -1):
        labels[t] = lab[node]
        tokens[t] = (node - 1) // 2 if node % 2 else -1
        node -= int(bp[t, node])
    assert node == 0
    return labels, tokens, float(best)


def seeded_case(seed, B, T, C, Umax, ragged_frames=False):
    """continuous random emissions, targets with repeats, every utterance feasible in its frame count:
    (em float32 [B, T, C], targets, frames int32 [B])"""
    rng = np.random.default_rng(seed)
    em = rng.normal(0, 2, (B, T, C)).astype(np.float32)
    targets, frames = [], []
    for _ in range(B):
        while True:
            t = rng.integers(1, C, int(rng.integers(1, Umax + 1))).tolist()
            if min_frames(t) <= T:
                break
        targets.append(t)
        frames.append(int(rng.integers(min_frames(t), T + 1)) if ragged_frames else T)
    return em, targets, np.asarray(frames, np.int32)
