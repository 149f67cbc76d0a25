"""The yardstick of the batched transducer forced alignment (gtnx_batch_transducer_align), on the
host: the max-plus recurrence of the contract with its tie rule (of two equal candidates the blank arc wins) and the
walk, over a compact plane in float32 (`transcribe`: what the kernel must reproduce bit for bit) and from the logits in
float64 (`reference`).  The gate on a score is the project's, 1e-4 max(1, |want|)."""
import numpy as np


def _best(lpb, lpl):
    """(score, token_frames [U_b], frame_tokens [T_b], ties) of one utterance's planes [T_b, U_b + 1], in their dtype;
    ties: the nodes of the path whose two candidates were equal.  The frames are None without a finite path"""
    Tb, U1 = lpb.shape
    ninf = lpb.dtype.type(-np.inf)
    v = np.full((Tb, U1), ninf, lpb.dtype)
    label, tie = np.zeros((Tb, U1), bool), np.zeros((Tb, U1), bool)
    v[0, 0] = 0
    for d in range(1, Tb + U1 - 1):  # (the anti-diagonal t + u = d from the one before it)
        t = np.arange(max(0, d - U1 + 1), min(Tb - 1, d) + 1)
        u = d - t
        up = np.where(t > 0, v[t - 1, u] + lpb[t - 1, u], ninf)
        left = np.where(u > 0, v[t, u - 1] + lpl[t, u - 1], ninf)
        label[t, u], tie[t, u] = left > up, (left == up) & (up > ninf)
        v[t, u] = np.where(left > up, left, up)
    score = v[Tb - 1, U1 - 1] + lpb[Tb - 1, U1 - 1]
    if not score > -np.inf:
        return score, None, None, 0
    t, u = Tb - 1, U1 - 1
    frames, tokens = np.zeros(U1 - 1, np.int32), np.zeros(Tb, np.int32)
    tokens[t] = u
    ties = 0
    while t or u:
        ties += int(tie[t, u])
        if label[t, u]:
            u -= 1
            frames[u] = t
        else:
            t -= 1
            tokens[t] = u
    return score, frames, tokens, ties


def _outputs(planes, B, T, U, dtype):
    """the contract's four outputs from per-utterance planes (lpb, lpl), None for an utterance that is not valid"""
    scores = np.full(B, -np.inf, dtype)
    token_frames, frame_tokens = np.full((B, U), -1, np.int32), np.full((B, T), -1, np.int32)
    token_scores = np.full((B, U), -np.inf, dtype)
    for b, p in enumerate(planes):
        if p is None:
            continue
        sc, fr, tk, _ = _best(*p)
        if fr is not None:
            scores[b] = sc
            token_frames[b, :len(fr)], frame_tokens[b, :len(tk)] = fr, tk
            token_scores[b, :len(fr)] = p[1][fr, np.arange(len(fr))]
    return scores, token_frames, token_scores, frame_tokens


def transcribe(rows, frames, tlens):
    """the kernel's arithmetic over a compact plane rows [B, T, U + 1, 3] (float32; NaN and +inf close the arc)"""
    B, T, U1, _ = rows.shape
    with np.errstate(invalid="ignore"):
        r = np.where(rows < np.inf, rows, -np.inf).astype(np.float32)
    planes = [(r[b, :Tb, :Ub + 1, 0], r[b, :Tb, :Ub + 1, 1]) if 1 <= Tb <= T and 0 <= Ub < U1 else None
              for b, (Tb, Ub) in enumerate(zip(map(int, frames), map(int, tlens)))]
    return _outputs(planes, B, T, U1 - 1, np.float32)


def planes64(x, targets, frames, tlens, blank, normalize):
    """per utterance (lp_blank, lp_label) [T_b, U_b + 1] in float64 from logits x, as the rows kernels define them"""
    B, T, U1, C = x.shape
    out = []
    for b in range(B):
        Tb, Ub = int(frames[b]), int(tlens[b])
        if not (1 <= Tb <= T and 0 <= Ub < U1):
            out.append(None)
            continue
        xs = x[b, :Tb, :Ub + 1].astype(np.float64)
        with np.errstate(invalid="ignore"):
            lse = np.logaddexp.reduce(xs, axis=2) if normalize else np.zeros(xs.shape[:2])
        dead = ~np.isfinite(lse) | (np.isnan(xs) | (xs == np.inf)).any(axis=2)
        lpb = np.where(dead, -np.inf, xs[:, :, blank] - np.where(dead, 0.0, lse))
        lpl = np.full((Tb, Ub + 1), -np.inf)
        for u, tok in enumerate(int(v) for v in targets[b, :Ub]):
            if 0 <= tok < C and tok != blank:
                lpl[:, u] = np.where(dead[:, u], -np.inf, xs[:, u, tok] - np.where(dead[:, u], 0.0, lse[:, u]))
        out.append((lpb, lpl))
    return out


def reference(x, targets, frames, tlens, blank, normalize):
    """(scores, token_frames, token_scores, frame_tokens) in float64 from the logits"""
    B, T, U1, _ = x.shape
    return _outputs(planes64(x, targets, frames, tlens, blank, normalize), B, T, U1 - 1, np.float64)


def path_score(plane, token_frames):
    """the float64 score of the path that emits token u at frame token_frames[u] on one utterance's plane"""
    lpb, lpl = plane
    fr = np.asarray(token_frames[:lpb.shape[1] - 1], np.int64)
    assert (np.diff(fr) >= 0).all() and (fr >= 0).all() and (fr < lpb.shape[0]).all()
    left = np.searchsorted(fr, np.arange(lpb.shape[0]), side="right")  # the column at which frame t is left
    return lpl[fr, np.arange(len(fr))].sum() + lpb[np.arange(lpb.shape[0]), left].sum()
