"""The yardstick of the CTC best-path decode tests: what shortestPath (reference gtn/functions/shortest.cpp:190-272)
gives on linearGraph(T, C), in numpy, followed by the CTC collapse.

  label   frame t takes the first arc whose weight is strictly greater than everything before it, starting from -inf:
          the smallest label among equal maxima; NaN and -inf are never chosen
  score   ((0 + m_0) + m_1) + ... + m_{T-1} in float32, in frame order
  no path a frame without an entry above -inf: labels -1, score -inf, nothing collapsed
  T = 0   no path either: linearGraph(0, C) is one start node that does not accept (creations.cpp:22)

tests/test_ctc_decode_cpu.py pins these rules to the oracle; tests/test_ctc_decode_gpu.py judges the kernels by them.
"""
import numpy as np


def first_max(row):
    """(label, maximum): `v > m` from (-1, -inf) in label order"""
    m, lab = np.float32(-np.inf), -1
    for c, v in enumerate(np.asarray(row, np.float32)):
        if v > m:  # (False for NaN)
            m, lab = v, c
    return lab, m


def first_max_rows(em):
    """first_max of every row of em [T, C] at once: NaN can never win and so counts as -inf, np.argmax takes the
    first of equal maxima, and a maximum of -inf means nothing was chosen (test_ctc_decode_cpu.py holds this against
    the loop above)"""
    x = np.asarray(em, np.float32)
    x = np.where(np.isnan(x), np.float32(-np.inf), x)
    if x.shape[0] == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    lab, m = x.argmax(axis=1), x.max(axis=1)
    lab[m == -np.inf] = -1
    return lab, m


def collapse(labels, blank=-1):
    """merge repeats, then drop `blank` (negative: nothing is dropped): (tokens, first frame of each)"""
    tokens, starts = [], []
    for t, v in enumerate(labels):
        if (t == 0 or v != labels[t - 1]) and v != blank:
            tokens.append(int(v))
            starts.append(t)
    return tokens, starts


def ctc_decode_ref(em, frames=None, blank=-1):
    """em [M, C] float32 -> (labels int [M] (-1 from `frames` on), score np.float32, tokens, starts); without a path
    every label is -1, the score -inf and the lists empty"""
    em = np.asarray(em, np.float32)
    M = em.shape[0]
    T = M if frames is None else int(frames)
    labels = np.full(M, -1, np.int64)
    lab, m = first_max_rows(em[:T])
    if T == 0 or (lab < 0).any():
        return labels, np.float32(-np.inf), [], []
    labels[:T] = lab
    score = np.float32(0.0)
    for t in range(T):  # (the association is the contract: no np.sum)
        score = np.float32(score + m[t])
    tokens, starts = collapse(labels[:T].tolist(), blank)
    return labels, score, tokens, starts


def decode_batch(em, frames=None, blank=-1):
    """the four dense arrays the device call fills, for em [B, M, C]: labels [B, M], scores [B], tokens [B, M],
    starts [B, M], lengths [B]"""
    B, M, _ = em.shape
    labels = np.full((B, M), -1, np.int32)
    tokens = np.full((B, M), -1, np.int32)
    starts = np.full((B, M), -1, np.int32)
    scores = np.zeros(B, np.float32)
    lengths = np.zeros(B, np.int32)
    for b in range(B):
        l, s, tk, st = ctc_decode_ref(em[b], None if frames is None else frames[b], blank)
        labels[b], scores[b], lengths[b] = l, s, len(tk)
        tokens[b, :len(tk)] = tk
        starts[b, :len(st)] = st
    return labels, scores, tokens, starts, lengths


# ---- seeded case generators -------------------------------------------------------------------------------------
def continuous_case(seed, B, T, C):
    """log-softmax-like scores without structure"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, T, C)) * 3.0 - 5.0).astype(np.float32)


def planted_case(seed, B, T, C, blank):
    """continuous scores with a planted best path that has structure: runs of a label, runs of the blank, and repeats
    of one label separated by a blank, so that collapsed lengths are neither 0 nor T by accident.  The planted label
    of a frame gets +20, far above the noise: no exact ties."""
    rng = np.random.default_rng(seed)
    em = (rng.standard_normal((B, T, C)) - 5.0).astype(np.float32)
    bl = blank if blank >= 0 else 0
    for b in range(B):
        t, prev = 0, None
        while t < T:
            kind = rng.integers(0, 4)
            run = int(rng.integers(1, 6))
            if kind == 0:
                lab = bl
            elif kind == 1 and prev is not None and prev != bl and t + 1 < T:
                em[b, t, bl] += 20.0  # one blank, then the label before it again
                t += 1
                lab = prev
            else:
                lab = int(rng.integers(0, C))
            em[b, t:t + run, lab] += 20.0
            t += run
            prev = lab
    return em


def tie_case(seed, B, T, C, kind):
    """integer-valued emissions, so that maxima tie exactly and float32 sums are exact: 'zero' all 0, '01' 0 / 1,
    'int' small integers, 'late' zeros with the maximum 1 planted at every 64th label and at the last (ties between
    lanes and between trips of a row loop)"""
    rng = np.random.default_rng(seed)
    if kind == "zero":
        return np.zeros((B, T, C), np.float32)
    if kind == "01":
        return rng.integers(0, 2, (B, T, C)).astype(np.float32)
    if kind == "int":
        return rng.integers(-3, 4, (B, T, C)).astype(np.float32)
    assert kind == "late"
    em = np.zeros((B, T, C), np.float32)
    first = rng.integers(0, C, (B, T))
    for b in range(B):
        for t in range(T):
            em[b, t, first[b, t]::64] = 1.0
            em[b, t, C - 1] = 1.0
    return em


def holes_case(seed, B, T, C, p=0.3):
    """integer-valued emissions with -inf entries; some rows may be all -inf (then the utterance has no path)"""
    rng = np.random.default_rng(seed)
    em = rng.integers(-3, 4, (B, T, C)).astype(np.float32)
    em[rng.random((B, T, C)) < p] = -np.inf
    return em
