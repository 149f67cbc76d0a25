"""The ASG loss of a padded batch in float64 (TEST INFRASTRUCTURE ONLY): the yardstick of tests/test_asg_frames_*.py.

loss_b = forwardScore(em_b[:T_b] o transitions) - forwardScore(em_b[:T_b] o (forceAlign(target_b) o transitions))
(examples/asg.cpp:30-68).  The full-connect term is tests/ctc_fp64.py: asg_fp64 on the first T_b rows; the force-align
term is a forward-backward over the U + 1 nodes of the alignment trellis (node n: "the first n labels are consumed"; a
frame enters node n >= 1 from n itself with trans[l, l], l = target[n - 1], or from n - 1 with trans[l, target[n - 2]]
-- start[l] for n = 1 -- and emits em[t, l]).  Entries of -inf are probability 0.  Gradients are d loss / d: the
emissions ([T, N], rows >= T_b zero) and the transitions in the arc order of gtn::criteria::asgTransitions
([N + N * N]: N start arcs, then arc N + i * N + j = j -> i).
"""
import numpy as np

from ctc_fp64 import asg_fp64

# (B, T, N, Umax): the shapes of tests/test_asg_frames_gpu.py -- one label, tiny N, N not a multiple of 4, letters,
# the launcher's switch from 32 to 64 entries per lane (64 / 65), the limit of the launch (127 / 128)
GPU_SHAPES = [(2, 9, 1, 3), (3, 7, 2, 3), (4, 12, 5, 4), (5, 40, 27, 9), (3, 33, 64, 10), (3, 33, 65, 10),
              (2, 20, 127, 6), (2, 20, 128, 6)]
# the other edges of asg_full.hip's layout (N <= 2 * JH labels, JH = 16 / 32 / 64 entries per lane at N <= 32 / <= 64 /
# else, read from LDS four at a time): a float4 with three live entries and with exactly four (3 / 4), the first label
# owned by the second half's lanes at JH = 16 (16 / 17), the switch from JH = 16 to 32 (31 / 32 / 33)
EDGE_SHAPES = [(3, 9, 3, 3), (3, 9, 4, 3), (4, 11, 16, 5), (4, 11, 17, 5), (4, 11, 31, 5), (4, 11, 32, 5),
               (4, 11, 33, 5)]
# utterances of production length (T = 1000): frames [1200, 30, 1, 234] and [600, 20, 1]
LONG_SHAPES = [(4, 1200, 27, 30), (3, 600, 128, 20)]
# seeded_case arguments: more utterances than the card has compute units, every length 1 .. 6 among them
MANY_CASE = (5, 300, 6, 5, 3)
# seeded_case arguments of the batch that kill_emissions turns into the -inf case: frames [12, 4, 1, 5]
DEAD_CASE = (91, 4, 12, 9, 4)
# upstream gradients of reduction="none" on (5, 40, 27, 9): a zero and a negative one among them
SEEDS = [0.0, -1.5, 2.0, 0.5, 1.0]
# the seed of a second (4, 12, 5, 4) batch run against the transitions graph of the first (gradient accumulation)
SECOND_SEED = 4242


def shape_seed(shape):
    """the seed under which tests/test_asg_frames_*.py draw the batch of a (B, T, N, Umax)"""
    _, T, N, _ = shape
    return 1000 + 7 * N + T


def kill_emissions(em):
    """a copy of DEAD_CASE's emissions with -inf in them: label 4 everywhere, labels 0 .. 6 of one frame of utterance 0,
    every label but 0 in the first frame of utterance 3 -- utterances 0, 2 and 3 keep finite scores -- and the whole of
    frame 1 of utterance 1, which leaves that utterance without a path"""
    em = np.array(em, copy=True)
    em[:, :, 4] = -np.inf
    em[0, 3, :7] = -np.inf
    em[3, 0, 1:] = -np.inf
    em[1, 1, :] = -np.inf
    return em


def fal_fp64(em, trans, start, target):
    """the force-align term on em [T, N]: (score, d score / d em [T, N], d score / d transitions [N + N * N])"""
    em = np.asarray(em, np.float64)
    trans = np.asarray(trans, np.float64)
    start = np.asarray(start, np.float64)
    T, N = em.shape
    tg = np.asarray([int(x) for x in target], np.int64)
    U = tg.size
    g_em, g_tr = np.zeros((T, N)), np.zeros(N + N * N)
    ninf = -np.inf
    if U == 0 or T < U:
        return ninf, g_em, g_tr
    w_self = trans[tg, tg]
    w_step = np.concatenate(([start[tg[0]]], trans[tg[1:], tg[:-1]]))
    i_self = N + tg * N + tg
    i_step = np.concatenate(([tg[0]], N + tg[1:] * N + tg[:-1]))
    with np.errstate(invalid="ignore"):
        alpha = np.full((T + 1, U + 1), ninf)
        alpha[0, 0] = 0.0
        for t in range(T):
            e = em[t, tg]
            alpha[t + 1, 1:] = np.logaddexp(alpha[t, 1:] + w_self, alpha[t, :-1] + w_step) + e
        Z = alpha[T, U]
        if not np.isfinite(Z):
            return ninf, g_em, g_tr
        beta = np.full((T + 1, U + 1), ninf)
        beta[T, U] = 0.0
        for t in range(T - 1, -1, -1):
            q = em[t, tg] + beta[t + 1, 1:]          # consume frame t into node n = 1 .. U, then finish
            beta[t, 1:] = q + w_self
            beta[t, :-1] = np.logaddexp(beta[t, :-1], q + w_step)
        for t in range(T):
            q = em[t, tg] + beta[t + 1, 1:]
            p_self = np.exp(alpha[t, 1:] + w_self + q - Z)
            p_step = np.exp(alpha[t, :-1] + w_step + q - Z)
            np.add.at(g_em[t], tg, p_self + p_step)
            np.add.at(g_tr, i_self, p_self)
            np.add.at(g_tr, i_step, p_step)
    return float(Z), g_em, g_tr


def asg_terms_fp64(em, trans, start, target, frames=None):
    """-> dict(loss, fcc, fal, g_em [T, N], g_tr [N + N * N]) on the first `frames` rows of em [T, N]"""
    em = np.asarray(em, np.float64)
    T_full, N = em.shape
    T = T_full if frames is None else int(frames)
    assert 1 <= T <= T_full
    tw = np.concatenate([np.asarray(start, np.float64).reshape(-1), np.asarray(trans, np.float64).reshape(-1)])
    with np.errstate(divide="ignore", invalid="ignore"):
        fcc, f_em, f_tr = asg_fp64(em[:T], tw)[:3]
    fal, a_em, a_tr = fal_fp64(em[:T], trans, start, target)
    g_em = np.zeros((T_full, N))
    g_em[:T] = f_em - a_em
    return {"loss": float(fcc - fal), "fcc": float(fcc), "fal": float(fal), "g_em": g_em, "g_tr": f_tr - a_tr}


def asg_loss_fp64(em, trans, start, target, frames=None):
    """-> (loss, d loss / d em [T, N], d loss / d transitions [N + N * N]) in float64; an utterance with fewer frames
    than labels has loss +inf and the full-connect term's gradient alone"""
    r = asg_terms_fp64(em, trans, start, target, frames)
    return r["loss"], r["g_em"], r["g_tr"]


def seeded_case(seed, B, T, N, Umax, em_scale=1.0):
    """(em float32 [B, T, N], trans float32 [N, N], start float32 [N], targets, frames int32 [B]): utterance 0 at full
    length, utterance 1 at len(target) frames (exactly one alignment; for B = 2 that is the one-label target at one
    frame), utterance 2 a one-label target at one frame, the others anywhere in len(target) .. T"""
    rng = np.random.default_rng(seed)
    em = (rng.normal(0, 1, (B, T, N)) * em_scale).astype(np.float32)
    trans = rng.normal(0, 1, (N, N)).astype(np.float32)
    start = rng.normal(0, 1, N).astype(np.float32)
    targets, frames = [], []
    for b in range(B):
        one = (b == 2) or (B == 2 and b == 1)
        U = 1 if one else (min(Umax, T) if b == 1 else int(rng.integers(1, min(Umax, T) + 1)))
        t = rng.integers(0, N, U).tolist()
        targets.append(t)
        frames.append(T if b == 0 else (U if (b == 1 or one) else int(rng.integers(U, T + 1))))
    return em, trans, start, targets, np.asarray(frames, np.int32)


def batch_fp64(em, trans, start, targets, frames):
    """the yardstick over a batch: dict(loss [B], fcc [B], fal [B], g_em [B, T, N], g_tr [B, N + N * N])"""
    rs = [asg_terms_fp64(em[b], trans, start, targets[b], frames[b]) for b in range(len(targets))]
    return {k: np.asarray([r[k] for r in rs]) for k in ("loss", "fcc", "fal", "g_em", "g_tr")}
