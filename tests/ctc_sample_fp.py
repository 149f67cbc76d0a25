"""The yardstick of the CTC posterior sampler's tests (gtnx_batch_ctc_sample; the contract is DESIGN section 32).

  mass      only finite entries carry mass; -inf, +inf and NaN are never chosen and are left out of Z
  no path   a frame without a finite entry, or T_b = 0: every sample of the utterance gets -1 rows, length 0, logq -inf
  draw      inverse CDF in label order: with u the uniform of (b, k, t), the smallest c whose cumulative mass over the
            labels 0 .. c exceeds u * Z; if rounding leaves none, the last label with mass
  uniform   Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (t, b, k >> 2, 0), sample k uses output word
            k & 3, u = (2 * (word >> 9) + 1) * 2^-24: strictly inside (0, 1), exact in float32
  logq      sum_t (x[b,t,c_t] / tau - log Z[b,t]), added in frame order from 0 in float32

Float32 arithmetic on a device need not give the yardstick's float64 labels where u falls within rounding of a step of
the CDF, so a device result is judged by a CERTIFICATE, not by equality of labels (certify below): every returned label
must carry mass and bracket its uniform within tol(C) of the float64 CDF, the tokens must be the collapse of the
returned labels, and logq the sum of the returned labels' terms within the error of a float32 recursive sum.

tol(C) = (4 C + 64) * 2^-24.  A float32 sum of C non-negative terms in any order is within (C - 1) * 2^-24 of the exact
sum, relative to it; the cumulative sum and Z each take one such error (2 C), the masses exp((x - max) / tau) carry the
rounding of the argument and a few ulp of exp, relative to masses that add to 1 (another 2 C at the most, generously),
and 64 ulp stand for the fixed steps (u * Z, the comparison).  A serial float32 cumulative sum stays at least 100 times
inside it (worst miss seen 8e-7 at C = 5000 against 1.2e-3).

tests/test_ctc_sample_cpu.py pins Philox to its known answers and shows that the certificate has teeth;
tests/test_ctc_sample_gpu.py judges the kernels by it.
"""
import numpy as np

from ctc_decode_fp import collapse

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32-10 of Salmon et al. (SC'11) in uint64 arithmetic.  counter: four arrays (or ints) that broadcast,
    key: two.  Returns the four output words as uint64 arrays holding 32-bit values."""
    c = [np.asarray(v, np.uint64) & MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (np.asarray(v, np.uint64) & MASK for v in key)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]  # (32 x 32 bits: no overflow in 64)
        c = [(p1 >> S32) ^ c[1] ^ k0, p1 & MASK, (p0 >> S32) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def word_to_uniform(word):
    """u = (2 * (word >> 9) + 1) * 2^-24 as float64 (the value is exact in float32 too)"""
    return (2.0 * (np.asarray(word, np.uint64) >> np.uint64(9)).astype(np.float64) + 1.0) * 2.0 ** -24


def uniforms(seed, B, N, T, b0=0):
    """u [B, N, T] float64 of utterances b0 .. b0 + B - 1"""
    seed = int(seed)
    t = np.arange(T, dtype=np.uint64)[None, None, :]
    b = (np.arange(B, dtype=np.uint64) + np.uint64(b0))[:, None, None]
    g = np.arange((N + 3) // 4, dtype=np.uint64)[None, :, None]
    words = philox4x32_10((t, b, g, 0), (seed & 0xFFFFFFFF, seed >> 32))
    u = np.empty((B, 4 * ((N + 3) // 4), T), np.float64)
    for j in range(4):
        u[:, j::4, :] = word_to_uniform(words[j])
    return u[:, :N, :]


def tol(C):
    return (4.0 * C + 64.0) * 2.0 ** -24


def frame_model(em, temperature=1.0):
    """what the float64 rules make of em [..., C]: (finite mask, F the normalised cumulative mass in label order,
    terms x / tau - log Z (nan where the entry has no mass), alive = the row has a finite entry).  Rows without a finite
    entry have F = 0 throughout."""
    x = np.asarray(em, np.float64)
    fin = np.isfinite(x)
    alive = fin.any(axis=-1)
    xs = np.where(fin, x, -np.inf)
    m = np.where(alive, xs.max(axis=-1, initial=-np.inf), 0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        arg = np.where(fin, (xs - m[..., None]) / float(temperature), -np.inf)
    mass = np.exp(arg)
    Z = mass.sum(axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        F = np.where(alive[..., None], np.cumsum(mass, axis=-1) / np.where(alive, Z, 1.0)[..., None], 0.0)
        terms = np.where(fin, arg - np.log(np.where(alive, Z, 1.0))[..., None], np.nan)
    return fin, F, terms, alive


def log_normaliser(em, temperature=1.0):
    """log Z of every row of em [..., C] in float64 (-inf for a row without a finite entry)"""
    x = np.asarray(em, np.float64)
    fin = np.isfinite(x)
    xs = np.where(fin, x, -np.inf) / float(temperature)
    m = xs.max(axis=-1, initial=-np.inf)
    ms = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return ms + np.log(np.exp(xs - ms[..., None]).sum(axis=-1))


def draw_labels(F, fin, u):
    """the rule of the draw on a normalised CDF F [T, C] against u [N, T]: the smallest c with F[t, c] > u, else the
    last label with mass.  (F, not the cumulative mass against u * Z: the same comparison up to rounding.)"""
    T, C = F.shape
    last = C - 1 - np.argmax(fin[:, ::-1], axis=1)
    lab = np.empty(u.shape, np.int64)
    for t in range(T):
        idx = np.searchsorted(F[t], u[:, t], side="right")  # first c with F[c] > u
        lab[:, t] = np.where(idx < C, idx, last[t])
        # a label without mass repeats the value before it and is never the first to exceed u; guard the fallback
        lab[:, t] = np.where(fin[t, np.minimum(lab[:, t], C - 1)], lab[:, t], last[t])
    return lab


def sample_ref(em, frames=None, blank=0, num_samples=4, seed=0, temperature=1.0, dtype=np.float64):
    """the sampler by the rules above for em [B, M, C]: (tokens [B, N, M], lengths [B, N], logq [B, N] float32,
    labels [B, N, M]).  dtype=np.float32 emulates a device: masses, a serial cumulative sum and Z in float32."""
    em = np.asarray(em, np.float32)
    B, M, C = em.shape
    N = int(num_samples)
    tokens = np.full((B, N, M), -1, np.int32)
    labels = np.full((B, N, M), -1, np.int32)
    lengths = np.zeros((B, N), np.int32)
    logq = np.full((B, N), -np.inf, np.float32)
    for b in range(B):
        T = M if frames is None else int(frames[b])
        fin, F, terms, alive = frame_model(em[b, :T], temperature)
        if T == 0 or not alive.all():
            continue
        u = uniforms(seed, 1, N, T, b0=b)[0]
        if dtype == np.float32:
            x = em[b, :T]
            xs = np.where(fin, x, np.float32(-np.inf))
            m = xs.max(axis=1)
            with np.errstate(invalid="ignore"):
                mass = np.where(fin, np.exp(((xs - m[:, None]) / np.float32(temperature)).astype(np.float32)),
                                np.float32(0)).astype(np.float32)
            cum = np.cumsum(mass, axis=1, dtype=np.float32)  # (serial, in label order)
            Zf = cum[:, -1]
            last = C - 1 - np.argmax(fin[:, ::-1], axis=1)
            lab = np.empty((N, T), np.int64)
            for t in range(T):
                target = (u[:, t].astype(np.float32) * Zf[t]).astype(np.float32)
                idx = np.searchsorted(cum[t], target, side="right")
                lab[:, t] = np.where(idx < C, idx, last[t])
        else:
            lab = draw_labels(F, fin, u)
        labels[b, :, :T] = lab
        tt = terms[np.arange(T)[None, :], lab]
        for k in range(N):
            acc = np.float32(0.0)
            for t in range(T):  # (the association is the contract: no np.sum)
                acc = np.float32(acc + np.float32(tt[k, t]))
            logq[b, k] = acc
            tk, _ = collapse(lab[k].tolist(), blank)
            tokens[b, k, :len(tk)] = tk
            lengths[b, k] = len(tk)
    return tokens, lengths, logq, labels


def certify(em, frames, blank, num_samples, seed, temperature, tokens, lengths, logq=None, labels=None, tag=""):
    """judge a result of the sampler for em [B, M, C]: raises AssertionError with the first offender.  `labels` are
    needed (the certificate is about them); `logq` may be None.  No sample is left out.  Returns the worst miss of the
    bracket, as a multiple of tol(C) (<= 1; for printing)."""
    em = np.asarray(em, np.float32)
    B, M, C = em.shape
    N = int(num_samples)
    assert labels is not None and labels.shape == (B, N, M) and tokens.shape == (B, N, M), (tag, "shapes")
    assert lengths.shape == (B, N) and (logq is None or logq.shape == (B, N)), (tag, "shapes")
    assert logq is None or not np.isnan(logq).any(), (tag, "NaN in logq")
    eps = tol(C)
    worst = 0.0
    for b in range(B):
        T = M if frames is None else int(frames[b])
        fin, F, terms, alive = frame_model(em[b, :T], temperature)
        if T == 0 or not alive.all():
            assert (labels[b] == -1).all() and (tokens[b] == -1).all() and (lengths[b] == 0).all(), (tag, b, "no path")
            assert logq is None or np.isneginf(logq[b]).all(), (tag, b, "no path logq", logq[b])
            continue
        lab = labels[b, :, :T].astype(np.int64)
        assert (labels[b, :, T:] == -1).all(), (tag, b, "label fill")
        assert ((lab >= 0) & (lab < C)).all(), (tag, b, "label range", lab.min(), lab.max())
        tix = np.arange(T)[None, :]
        assert fin[tix, lab].all(), (tag, b, "a label without mass", np.argwhere(~fin[tix, lab])[:3].tolist())
        u = uniforms(seed, 1, N, T, b0=b)[0]
        hi = F[tix, lab]
        lo = np.where(lab > 0, F[tix, np.maximum(lab - 1, 0)], 0.0)
        miss = np.maximum(lo - u, u - hi)
        w = float(miss.max())
        worst = max(worst, w / eps)
        if w > eps:
            k, t = np.unravel_index(np.argmax(miss), miss.shape)
            raise AssertionError((tag, "bracket", b, int(k), int(t), int(lab[k, t]), float(lo[k, t]), float(u[k, t]),
                                  float(hi[k, t]), eps))
        tt = terms[tix, lab]
        for k in range(N):
            tk, _ = collapse(lab[k].tolist(), blank)
            assert lengths[b, k] == len(tk), (tag, b, k, "length", int(lengths[b, k]), len(tk))
            assert tokens[b, k, :len(tk)].tolist() == tk and (tokens[b, k, len(tk):] == -1).all(), (tag, b, k, "tokens")
        if logq is not None:
            want = tt.sum(axis=1)
            bound = (T + 8) * 2.0 ** -24 * np.abs(tt).sum(axis=1)
            err = np.abs(logq[b].astype(np.float64) - want)
            assert (err <= bound).all(), (tag, b, "logq", int(np.argmax(err - bound)), logq[b].tolist()[:4],
                                          want.tolist()[:4], float((err / np.maximum(bound, 1e-300)).max()))
    return worst


def sequence_distribution(em, blank, temperature=1.0):
    """{label sequence (tuple): probability} of the collapse of an alignment of em [T, C] drawn by the rules, in
    float64, by enumerating the C^T alignments (small T and C only)"""
    fin, F, terms, alive = frame_model(em, temperature)
    T, C = em.shape
    assert alive.all() and C ** T <= 4096
    p = np.where(fin, np.exp(np.where(fin, terms, 0.0)), 0.0)
    out = {}
    for a in np.ndindex(*([C] * T)):
        pr = float(np.prod([p[t, a[t]] for t in range(T)]))
        tk = tuple(collapse(list(a), blank)[0])
        out[tk] = out.get(tk, 0.0) + pr
    return out


# ---- seeded case generators -------------------------------------------------------------------------------------
def continuous_case(seed, B, T, C):
    """scores without structure, a few nats apart"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, T, C)) * 2.0 - 3.0).astype(np.float32)


def peaked_case(seed, B, T, C):
    """one label of every row holds mass 1 - 1e-6 (C > 1), the rest share 1e-6 equally"""
    rng = np.random.default_rng(seed)
    em = np.full((B, T, C), np.log(1e-6 / max(C - 1, 1)), np.float32)
    peak = rng.integers(0, C, (B, T))
    np.put_along_axis(em, peak[..., None], np.float32(np.log1p(-1e-6)), axis=2)
    return em, peak


def holes_case(seed, B, T, C, p=0.3):
    """integer-valued rows with -inf / +inf / NaN entries; every row keeps at least one finite entry"""
    rng = np.random.default_rng(seed)
    em = rng.integers(-2, 3, (B, T, C)).astype(np.float32)
    r = rng.random((B, T, C))
    em[r < p] = -np.inf
    em[(r >= p) & (r < p + 0.1)] = np.inf
    em[(r >= p + 0.1) & (r < p + 0.2)] = np.nan
    keep = rng.integers(0, C, (B, T))
    np.put_along_axis(em, keep[..., None], np.float32(1.0), axis=2)
    return em
