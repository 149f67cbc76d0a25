"""The recursion of gtn_amd/csrc/asg_full.hip in numpy float32 (TEST INFRASTRUCTURE ONLY).

What asg_full_forward_kernel and asg_full_backward_kernel compute for ONE utterance, statement by statement, in the
number formats the kernels use: float32 for everything a lane holds (E, q, la, bq, f, c, X, gamma), float64 for the
running sums of the per-step maxima (L, LB) and for the score Z.  It separates "float32 in this design cannot meet the
gate at this shape" from "the kernel is wrong" when a GPU test fails, and it is what tests/test_asg_frames_cpu.py
holds to asg_fp64 at every shape tests/test_asg_frames_gpu.py launches.

Not bit-identical to the device: the sums over a row are numpy's float32 pairwise sums where the kernel has two FMA
chains per half and one cross-lane add, and exp / log are the host's float32 functions.  Both differ from the kernel
by rounding of the same size, not by method.

Layout as on the device: tw[:N] start scores, tw[N + i * N + j] the score of j -> i.
"""
import numpy as np

F = np.float32
NINF = F(-np.inf)
C_MAX = F(3.0e38)


def _rows(tw, N):
    """(row maxima with 0 for a row that is all -inf, E[i][j] = exp(W[i][j] - rowmax_i)) in float32"""
    W = np.asarray(tw, F)[N:].reshape(N, N)
    rm = W.max(1)
    rm = np.where(rm == NINF, F(0), rm).astype(F)
    return rm, np.exp(W - rm[:, None]).astype(F)


def forward_f32(em, tw):
    """-> (Z float64, la [T, N] float32, L [T] float64): asg_full_forward_kernel on em [T, N]"""
    em = np.asarray(em, F)
    T, N = em.shape
    tw = np.asarray(tw, F)
    rm, E = _rows(tw, N)
    la_out, L_out = np.empty((T, N), F), np.empty(T, np.float64)
    L = 0.0
    av = (tw[:N] + em[0]).astype(F)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for t in range(T):
            m = av.max()
            la = (av - (F(0) if m == NINF else m)).astype(F)
            L += float(m)
            q = np.exp(la).astype(F)
            la_out[t], L_out[t] = la, L
            if t + 1 >= T:
                break
            s = (E * q[None, :]).sum(1, dtype=F)
            av = np.where(s > 0, (np.log(np.where(s > 0, s, F(1))).astype(F) + rm).astype(F) + em[t + 1], NINF).astype(F)
        Z = L + float(np.log(q.sum(dtype=F)))
    return Z, la_out, L_out


def backward_f32(em, tw, Z, la, Ls, delta=1.0, want_tr=True):
    """-> (d em [T, N] float32, the utterance's share of d transitions [N + N * N] float32 or None):
    asg_full_backward_kernel with the upstream gradient `delta`"""
    em = np.asarray(em, F)
    T, N = em.shape
    delta = F(delta)
    ge = np.zeros((T, N), F)
    part = np.zeros(N + N * N, F) if want_tr else None
    if not np.isfinite(Z):
        return ge, part  # no finite path: zeros are stored, nothing is multiplied
    rm, E = _rows(tw, N)
    X = np.zeros((N, N), F)  # X[i][r], as the lane (r, half of i) holds it
    bq = np.ones(N, F)
    LB = 0.0
    la_t, L_t = la[T - 1], Ls[T - 1]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for t in range(T - 1, -1, -1):
            lbq = np.where(bq > 0, np.log(np.where(bq > 0, bq, F(1))), NINF).astype(F)
            gam = (np.exp(((la_t + lbq).astype(F) + F(L_t + LB - Z)).astype(F)).astype(F) * delta).astype(F)
            ge[t] = gam
            if t == 0:
                if want_tr:
                    part[:N] = gam
                break
            la_p, L_p = la[t - 1], Ls[t - 1]
            g = ((em[t] + rm).astype(F) + lbq).astype(F)
            mf = g.max()
            f = np.exp((g - (F(0) if mf == NINF else mf)).astype(F)).astype(F)
            c = np.minimum(np.exp((la_p + F(L_p + float(mf) + LB - Z)).astype(F)).astype(F), C_MAX)
            if want_tr:
                X = (X + (f[:, None] * c[None, :]).astype(F)).astype(F)
            bq = (E * f[:, None]).sum(0, dtype=F)
            LB += float(mf)
            la_t, L_t = la_p, L_p
        if want_tr:
            part[N:] = np.where(E > 0, ((E * X).astype(F) * delta).astype(F), F(0)).reshape(-1)
    return ge, part


def asg_full_f32(em, tw, delta=1.0, want_tr=True):
    """one utterance: (Z float64 -- the device stores float32(Z) as the score --, d em, share of d transitions)"""
    Z, la, Ls = forward_f32(em, tw)
    return (Z,) + backward_f32(em, tw, Z, la, Ls, delta, want_tr)


def batch_f32(em, trans, start, frames, delta=None):
    """a padded batch as the three launches see it: (scores [B] float64, d em [B, T, N] float32 with zeros in the pad
    rows, d transitions [N + N * N] float32 = the shares added in utterance order in float64, as
    asg_full_reduce_kernel adds them)"""
    em = np.asarray(em, F)
    B, T, N = em.shape
    tw = np.concatenate([np.asarray(start, F).reshape(-1), np.asarray(trans, F).reshape(-1)])
    delta = np.ones(B, F) if delta is None else np.asarray(delta, F)
    Z, ge, acc = np.empty(B), np.zeros((B, T, N), F), np.zeros(N + N * N)
    for b in range(B):
        f = int(frames[b])
        Z[b], ge[b, :f], part = asg_full_f32(em[b, :f], tw, delta[b])
        acc += part.astype(np.float64)
    return Z, ge, acc.astype(F)
