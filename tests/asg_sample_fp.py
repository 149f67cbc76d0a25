"""The yardstick of the ASG posterior sampler's tests (gtnx_batch_asg_sample; the contract is DESIGN section 34).

  model     table [C + C * C]: table[c] the start score of label c, table[C + i * C + j] the score of moving from label
            j to label i.  s(y) = table[y0] + x[0,y0] + sum_{t>=1} (table[C + y_t * C + y_{t-1}] + x[t,y_t]); alignment
            y is drawn with probability exp(s(y) / tau - logZ), logZ = log sum_y exp(s(y) / tau)
  mass      only finite entries carry mass: a -inf, +inf or NaN emission or table entry makes every alignment through
            it impossible, and it is never drawn
  no path   no alignment of finite score, or T_b = 0: every sample of the utterance gets -1 rows, length 0, logq -inf,
            and logz is -inf.  No output is ever NaN
  filter    alpha_0[i] = (table[i] + x[0,i]) / tau; alpha_t[i] = x[t,i] / tau + logsumexp_j(table[C + i * C + j] / tau +
            alpha_{t-1}[j]), kept per frame in a rescaled form (relative planes la_t = alpha_t - L_t, the running
            reference L_t in float64); logZ = logsumexp_i alpha_{T-1}[i]
  draw      backward, one uniform per (b, k, t): frame T - 1 has masses exp(alpha_{T-1}[j] - ref), frame t below it,
            given i = y_{t+1}, masses exp(alpha_t[j] + table[C + i * C + j] / tau - ref).  Inverse CDF in label order:
            the smallest j whose cumulative mass over 0 .. j exceeds u * total (the total as the sampler summed it); if
            rounding leaves none, the last label with mass.  A label without mass is never returned
  uniform   Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (t, b, k >> 2, 1) -- the CTC sampler has 0 in
            the last word --, sample k uses output word k & 3, u = (2 * (word >> 9) + 1) * 2^-24; b is the index in the
            whole batch
  logq      the sum of the drawn conditionals' logs log(mass_j / total), added in draw order (frame T - 1 first) from 0
            in float32; in exact arithmetic s(y) / tau - logZ
  collapse  equal neighbours merged; ASG has no blank

Float32 labels need not equal float64 labels where u falls within rounding of a step of a CDF, so a device result is
judged by a CERTIFICATE (certify below), and no sample is left out: every returned label has mass in float64, every
returned alignment a finite score, and for every (b, k, t) the uniform is bracketed by the float64 conditional CDF given
the device's OWN y_{t+1} within tol(C) + 32 d.  tol(C) = (4 C + 64) * 2^-24 is the CTC sampler's derived bound for one
CDF (ctc_sample_fp); d is the drift of float32 planes from float64 ones, measured by this file on that case: the largest
absolute difference between the float64 planes and this file's float32 emulation of the filter (serial sums) over the
entries finite in both, each row shifted to its own maximum, floored at 2^-22; the factor 32 allows for another
summation order and a few ulp of exp on a device.  Tokens and lengths are the merge of the returned labels, logq is
within (T + 8) * 2^-24 * sum |term| + T * 32 d of the float64 s(y) / tau - logZ, and logz within 1e-4 * max(1, |logz|)
of the float64 one (the project's gate for scores).

Measured with the emulation here (numpy) before any device ran: d between 1.1e-6 and 3.3e-6 for (T, C) = (65, 29),
(200, 64), (130, 300), (65, 300) at scale 0.5, (200, 29) at scale 5 and (65, 65) with 30 % table holes, without growth
in T; worst CDF difference 4e-7 .. 1.1e-6.  Worst seen on an MI355X over every test of tests/test_asg_sample_gpu.py: a
bracket miss of 0 of the tolerance (no uniform lay outside its float64 bracket, even before the tolerance is added); the
float32 emulation on the same inputs: 0 as well.
"""
import numpy as np

from asg_score_fp import table_of  # noqa: F401  (the table's layout; re-exported for the tests)
from ctc_sample_fp import philox4x32_10, tol, word_to_uniform

NEG = -np.inf
D_FLOOR = 2.0 ** -22
SCORE_GATE = 1e-4


def uniforms(seed, B, N, T, b0=0):
    """u [B, N, T] float64 of utterances b0 .. b0 + B - 1"""
    seed = int(seed)
    t = np.arange(T, dtype=np.uint64)[None, None, :]
    b = (np.arange(B, dtype=np.uint64) + np.uint64(b0))[:, None, None]
    g = np.arange((N + 3) // 4, dtype=np.uint64)[None, :, None]
    words = philox4x32_10((t, b, g, 1), (seed & 0xFFFFFFFF, seed >> 32))
    u = np.empty((B, 4 * ((N + 3) // 4), T), np.float64)
    for j in range(4):
        u[:, j::4, :] = word_to_uniform(words[j])
    return u[:, :N, :]


def clean(x, dtype=np.float64):
    """entries without mass (-inf, +inf, NaN) as -inf"""
    x = np.asarray(x, dtype)
    return np.where(np.isfinite(x), x, dtype(NEG))


def split(table, C):
    table = np.asarray(table, np.float32)
    assert table.shape == (C + C * C,)
    return table[:C], table[C:].reshape(C, C)  # W[i, j]: j -> i


def _lse(x, axis):
    m = x.max(axis=axis)
    ms = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return ms + np.log(np.exp(x - np.expand_dims(ms, axis)).sum(axis=axis))


def filter64(em, table, temperature=1.0):
    """float64 filter of em [T, C]: (la [T, C] the planes relative to their row's maximum, -inf without mass; L [T] the
    running reference; logz)"""
    T, C = em.shape
    tau = float(temperature)
    st, W = split(table, C)
    x, st, W = clean(em) / tau, clean(st), clean(W) / tau
    la = np.full((T, C), NEG)
    L = np.zeros(T)
    if T == 0:
        return la, L, NEG
    ref = 0.0
    av = clean(clean(table[:C]) + clean(em[0])) / tau
    del st
    for t in range(T):
        if t:
            av = x[t] + _lse(W + la[t - 1][None, :], 1)
        m = av.max()
        if not np.isfinite(m):
            return la, L, NEG  # (the rest of the planes stays without mass)
        la[t] = av - m
        ref += m
        L[t] = ref
    return la, L, float(ref + _lse(la[T - 1], 0))


def filter32(em, table, temperature=1.0):
    """the float32 emulation of a device's filter: exp(W / tau - rowmax) and q = exp(la) in float32, serial sums over j
    in float32, one log per row and frame, the reference in float64.  Same returns as filter64."""
    f = np.float32
    T, C = em.shape
    inv = f(min(f(1.0) / f(temperature), np.finfo(f).max))
    st, W = split(table, C)
    with np.errstate(invalid="ignore", over="ignore"):
        x = clean(clean(em, f) * inv, f)
        Wt = clean(clean(W, f) * inv, f)
        av = clean((clean(st, f) + clean(em[0], f) if T else clean(st, f)) * inv, f)
    rm = Wt.max(axis=1)
    rm = np.where(np.isfinite(rm), rm, f(0)).astype(f)
    E = np.exp(Wt - rm[:, None]).astype(f)
    la = np.full((T, C), NEG, f)
    L = np.zeros(T)
    if T == 0:
        return la, L, NEG
    ref = 0.0
    for t in range(T):
        if t:
            q = np.exp(la[t - 1]).astype(f)
            s = np.cumsum(E * q[None, :], axis=1, dtype=f)[:, -1]  # (serial, in label order)
            with np.errstate(divide="ignore"):
                av = np.where(s > 0, np.log(np.where(s > 0, s, f(1))).astype(f) + rm + x[t], f(NEG)).astype(f)
        m = av.max()
        if not np.isfinite(m):
            return la, L, NEG
        la[t] = av - m
        ref += float(m)
        L[t] = ref
    with np.errstate(divide="ignore"):
        s = np.exp(la[T - 1]).astype(f).sum(dtype=f)
    return la, L, float(ref + float(np.log(s)))


def drift(la64, la32):
    """d of the certificate: the largest difference of the planes over the entries finite in both, floored"""
    both = np.isfinite(la64) & np.isfinite(la32)
    diff = np.abs(np.where(both, la64, 0.0) - np.where(both, la32.astype(np.float64), 0.0))
    return max(float(diff.max(initial=0.0)), D_FLOOR)


def conditional(la_t, wrows):
    """the float64 conditional of a frame for every row of wrows [N, C] (zeros at the last frame): (fin [N, C], F [N, C]
    the normalised cumulative mass in label order, terms [N, C] = log(mass / total), nan without mass)"""
    x = la_t[None, :] + wrows
    fin = np.isfinite(x)
    m = x.max(axis=1)
    assert np.isfinite(m).all(), "a conditional without mass"
    mass = np.exp(x - m[:, None])
    tot = mass.sum(axis=1)
    F = np.cumsum(mass, axis=1) / tot[:, None]
    with np.errstate(invalid="ignore"):
        terms = np.where(fin, x - m[:, None] - np.log(tot)[:, None], np.nan)
    return fin, F, terms


def merge(labels):
    """equal neighbours merged"""
    lab = np.asarray(labels)
    if lab.size == 0:
        return []
    keep = np.concatenate([[True], lab[1:] != lab[:-1]])
    return lab[keep].tolist()


def score_of(em, table, y):
    """s(y) in float64, -inf through an entry without mass"""
    T, C = em.shape
    st, W = split(table, C)
    x, st, W = clean(em), clean(st), clean(W)
    y = np.asarray(y, np.int64)
    return float(st[y[0]] + x[np.arange(T), y].sum() + W[y[1:], y[:-1]].sum())


def sample_ref(em, table, frames=None, num_samples=4, seed=0, temperature=1.0, dtype=np.float64):
    """the sampler by the rules above for em [B, M, C]: (tokens [B, N, M], lengths [B, N], logq [B, N] float32, labels
    [B, N, M], logz [B] float32).  dtype=np.float32 emulates a device: the planes of filter32, masses, a serial
    cumulative sum and the total in float32."""
    em = np.asarray(em, np.float32)
    B, M, C = em.shape
    N = int(num_samples)
    f32 = dtype == np.float32
    tokens = np.full((B, N, M), -1, np.int32)
    labels = np.full((B, N, M), -1, np.int32)
    lengths = np.zeros((B, N), np.int32)
    logq = np.full((B, N), NEG, np.float32)
    logz = np.full(B, NEG, np.float32)
    _, W = split(table, C)
    if f32:
        inv = np.float32(min(np.float32(1.0) / np.float32(temperature), np.finfo(np.float32).max))
        with np.errstate(invalid="ignore", over="ignore"):
            Wt = clean(clean(W, np.float32) * inv, np.float32)
    else:
        Wt = clean(W) / float(temperature)
    for b in range(B):
        T = M if frames is None else int(frames[b])
        la, _, z = (filter32 if f32 else filter64)(em[b, :T], table, temperature)
        if T == 0 or not np.isfinite(z):
            continue
        logz[b] = z
        u = uniforms(seed, 1, N, T, b0=b)[0]
        lab = np.empty((N, T), np.int64)
        acc = np.zeros(N, np.float32)
        for t in range(T - 1, -1, -1):
            x = la[t][None, :] + (Wt[lab[:, t + 1], :] if t < T - 1 else np.zeros((N, C), la.dtype))
            m = x.max(axis=1)
            mass = np.exp(x - m[:, None]).astype(dtype)
            cum = np.cumsum(mass, axis=1, dtype=dtype)  # (serial, in label order)
            tot = cum[:, -1]
            target = (u[:, t].astype(dtype) * tot).astype(dtype)
            has = mass > 0
            last = C - 1 - np.argmax(has[:, ::-1], axis=1)
            for k in range(N):
                idx = int(np.searchsorted(cum[k], target[k], side="right"))  # first j with cum[j] > target
                lab[k, t] = idx if idx < C and has[k, idx] else last[k]
            sel = x[np.arange(N), lab[:, t]]
            term = (sel - m).astype(dtype) - np.log(tot).astype(dtype)
            acc = (acc + term.astype(np.float32)).astype(np.float32)  # (draw order: the association is the contract)
        labels[b, :, :T] = lab
        logq[b] = acc
        for k in range(N):
            tk = merge(lab[k])
            tokens[b, k, :len(tk)] = tk
            lengths[b, k] = len(tk)
    return tokens, lengths, logq, labels, logz


def certify(em, table, frames, num_samples, seed, temperature, tokens, lengths, logq=None, labels=None, logz=None,
            tag=""):
    """judge a result of the sampler for em [B, M, C]: raises AssertionError with the first offender.  `labels` are
    needed (the certificate is about them); `logq` and `logz` may be None.  No sample is left out.  Returns the worst
    miss of the bracket as a multiple of its tolerance tol(C) + 32 d (<= 1; for printing)."""
    em = np.asarray(em, np.float32)
    B, M, C = em.shape
    N = int(num_samples)
    tau = float(temperature)
    assert labels is not None and labels.shape == (B, N, M) and tokens.shape == (B, N, M), (tag, "shapes")
    assert lengths.shape == (B, N) and (logq is None or logq.shape == (B, N)), (tag, "shapes")
    assert logz is None or logz.shape == (B,), (tag, "shapes")
    assert logq is None or not np.isnan(logq).any(), (tag, "NaN in logq")
    assert logz is None or not np.isnan(logz).any(), (tag, "NaN in logz")
    _, W = split(table, C)
    Wt = clean(W) / tau
    worst = 0.0
    for b in range(B):
        T = M if frames is None else int(frames[b])
        la, _, z = filter64(em[b, :T], table, tau)
        if T == 0 or not np.isfinite(z):
            assert (labels[b] == -1).all() and (tokens[b] == -1).all() and (lengths[b] == 0).all(), (tag, b, "no path")
            assert logq is None or np.isneginf(logq[b]).all(), (tag, b, "no path logq", logq[b])
            assert logz is None or np.isneginf(logz[b]), (tag, b, "no path logz", logz[b])
            continue
        d = drift(la, filter32(em[b, :T], table, tau)[0])
        eps = tol(C) + 32.0 * d
        if logz is not None:
            assert abs(float(logz[b]) - z) <= SCORE_GATE * max(1.0, abs(z)), (tag, b, "logz", float(logz[b]), z)
        lab = labels[b, :, :T].astype(np.int64)
        assert (labels[b, :, T:] == -1).all(), (tag, b, "label fill")
        assert ((lab >= 0) & (lab < C)).all(), (tag, b, "label range", int(lab.min()), int(lab.max()))
        u = uniforms(seed, 1, N, T, b0=b)[0]
        ks = np.arange(N)
        tsum = np.zeros(N)
        tabs = np.zeros(N)
        for t in range(T - 1, -1, -1):
            wr = Wt[lab[:, t + 1], :] if t < T - 1 else np.zeros((N, C))
            ok = np.isfinite(la[t][lab[:, t]] + wr[ks, lab[:, t]])
            assert ok.all(), (tag, b, "a label without mass", int(np.argmin(ok)), t, int(lab[np.argmin(ok), t]))
            fin, F, terms = conditional(la[t], wr)
            hi = F[ks, lab[:, t]]
            lo = np.where(lab[:, t] > 0, F[ks, np.maximum(lab[:, t] - 1, 0)], 0.0)
            miss = np.maximum(lo - u[:, t], u[:, t] - hi)
            w = float(miss.max())
            worst = max(worst, w / eps)
            if w > eps:
                k = int(np.argmax(miss))
                raise AssertionError((tag, "bracket", b, k, t, int(lab[k, t]), float(lo[k]), float(u[k, t]),
                                      float(hi[k]), eps, w / eps))
            tt = terms[ks, lab[:, t]]
            tsum += tt
            tabs += np.abs(tt)
        for k in range(N):
            s = score_of(em[b, :T], table, lab[k])
            assert np.isfinite(s), (tag, b, k, "an alignment without a finite score")
            tk = merge(lab[k])
            assert lengths[b, k] == len(tk), (tag, b, k, "length", int(lengths[b, k]), len(tk))
            assert tokens[b, k, :len(tk)].tolist() == tk and (tokens[b, k, len(tk):] == -1).all(), (tag, b, k, "tokens")
            if logq is not None:
                want = s / tau - z
                bound = (T + 8) * 2.0 ** -24 * tabs[k] + T * 32.0 * d
                err = abs(float(logq[b, k]) - want)
                assert err <= bound, (tag, b, k, "logq", float(logq[b, k]), want, err / bound)
    return worst


def alignment_distribution(em, table, temperature=1.0):
    """{alignment (tuple): probability} for em [T, C] in float64 by enumerating the C^T alignments (C^T <= 4096)"""
    T, C = em.shape
    assert C ** T <= 4096
    s = np.array([score_of(em, table, a) for a in np.ndindex(*([C] * T))]) / float(temperature)
    p = np.exp(s - _lse(s, 0))
    return {a: float(pr) for a, pr in zip(np.ndindex(*([C] * T)), p)}


def sequence_distribution(em, table, temperature=1.0):
    """{label sequence (tuple): probability} of the merge of an alignment drawn by the rules"""
    out = {}
    for a, pr in alignment_distribution(em, table, temperature).items():
        tk = tuple(merge(a))
        out[tk] = out.get(tk, 0.0) + pr
    return out


# ---- seeded case generators -------------------------------------------------------------------------------------
def continuous_case(seed, B, T, C, scale=0.5):
    """(em [B, T, C], table): scores without structure"""
    rng = np.random.default_rng(seed)
    em = (rng.standard_normal((B, T, C)) * scale).astype(np.float32)
    trans = (rng.standard_normal((C, C)) * scale).astype(np.float32)
    start = (rng.standard_normal(C) * scale).astype(np.float32)
    return em, table_of(start, trans)


def peaked_case(seed, B, T, C):
    """(em, table, succ): flat emissions; after label j one successor succ[j] holds mass 1 - 1e-6 (C > 1), the rest
    share 1e-6 equally"""
    rng = np.random.default_rng(seed)
    em = np.zeros((B, T, C), np.float32)
    trans = np.full((C, C), np.log(1e-6 / max(C - 1, 1)), np.float32)
    succ = rng.integers(0, C, C)
    trans[succ, np.arange(C)] = np.float32(np.log1p(-1e-6))
    return em, table_of(np.zeros(C, np.float32), trans), succ


def equal_case(B, T, C):
    """every alignment has the same score"""
    return np.zeros((B, T, C), np.float32), np.zeros(C + C * C, np.float32)


def holes_case(seed, B, T, C, p=0.3):
    """integer-valued scores with -inf / +inf / NaN entries in emissions, transitions and start scores (a start entry
    among them); label `keep` stays whole -- its emissions, its start score and its self-transition are finite -- so
    every utterance has a path"""
    rng = np.random.default_rng(seed)

    def punch(a):
        r = rng.random(a.shape)
        a[r < p] = -np.inf
        a[(r >= p) & (r < p + 0.05)] = np.inf
        a[(r >= p + 0.05) & (r < p + 0.1)] = np.nan
        return a

    em = punch(rng.integers(-2, 3, (B, T, C)).astype(np.float32))
    trans = punch(rng.integers(-2, 3, (C, C)).astype(np.float32))
    start = punch(rng.integers(-2, 3, C).astype(np.float32))
    keep = int(rng.integers(0, C))
    em[:, :, keep] = 1.0
    trans[keep, keep] = 0.0
    start[keep] = 0.0
    start[(keep + 1) % C] = -np.inf if C > 1 else start[0]
    return em, table_of(start, trans)


def dead_end_case(seed, B, T, C):
    """(em, table, dead): label `dead` is reachable at every frame and has no finite continuation (its column of the
    transitions is -inf), so it may be drawn at the last frame only"""
    assert C >= 2
    em, table = continuous_case(seed, B, T, C)
    dead = C // 2
    W = table[C:].reshape(C, C)
    W[:, dead] = -np.inf
    em[:, :, dead] += 2.0  # (attractive where it is allowed: a sampler that ignores the dead end picks it often)
    return em, table, dead


# ---- the shapes the device is certified at (C, T, B, N): every filter variant's edges (32 / 33 are inside 29 .. 64, 64 /
# 65, the register / L2 switch at 128 / 129, 256-row steps at 300 and 1024), rows that are no 16-byte multiple, the
# 64-frame blocks of the collapse and of the draw's Philox calls, a last workgroup of the wide filter that is not full
# (B = 70, B = 1, B = 3), the Philox groups of four samples
SHAPES = [(1, 1, 1, 1), (1, 65, 3, 4), (2, 2, 3, 3), (2, 200, 1, 5), (3, 63, 70, 4), (3, 64, 1, 17), (29, 65, 3, 5),
          (29, 130, 70, 1), (29, 200, 3, 17), (64, 64, 3, 4), (64, 130, 1, 3), (65, 63, 3, 5), (65, 2, 70, 1),
          (128, 65, 3, 4), (128, 1, 1, 17), (129, 64, 3, 3), (129, 130, 1, 5), (300, 130, 3, 4), (300, 63, 1, 1),
          (300, 2, 70, 3), (1024, 65, 1, 3), (1024, 2, 3, 5)]


def shape_case(C, T, B, N):
    """(em, table, seed) of a SHAPES entry"""
    seed = 1000 * C + T
    em, table = continuous_case(seed, B, T, C)
    return em, table, seed
