"""ASG posterior sampling, the parts that need no GPU: the yardstick of tests/asg_sample_fp.py against the enumeration
of all alignments; the certificate that test_asg_sample_gpu.py judges the kernels by has teeth (six wrong samplers are
rejected); the float32 emulation of a device passes it on every input the GPU file certifies; logz of the yardstick is
the full-connect score of tests/ctc_fp64.py; the entry points exist and refuse bad arguments, each naming the entry (the
refusals that need a native linear batch -- a short row stride, a batch that is not linear, a frame count beyond the
batch's rows -- are reached on the device only: test_asg_sample_gpu.py; their torch counterparts are here)."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT, has_gpu
import asg_sample_fp as fp
import ctc_fp64


# the statistical case, shared with test_asg_sample_gpu.py: 256 copies of one T = 4, C = 3 slab, 16 samples each.  The
# table forbids label 1 after label 0 and strongly favours label 2 after label 1.  (The seed was fixed after checking
# that the yardstick passes with it.)
STAT_SEED, STAT_B, STAT_N = 20261, 256, 16


def stat_model():
    slab = np.array([[-0.3, -1.1, -1.6], [-1.2, -0.4, -1.3], [-0.9, -1.4, -0.6], [-1.0, -0.8, -1.2]], np.float32)
    trans = np.array([[0.2, -0.3, 0.1], [-np.inf, 0.0, -0.4], [-0.2, 2.0, 0.3]], np.float32)  # [i, j]: j -> i
    start = np.array([0.1, -0.2, 0.0], np.float32)
    return slab, fp.table_of(start, trans)


def check_frequencies(labels, tokens, lengths, slab, table, temperature=1.0):
    """the frequency of every alignment and of every label sequence over the B * N samples is within
    5 sqrt(p (1 - p) / n) of its enumerated probability"""
    n = tokens.shape[0] * tokens.shape[1]
    T = slab.shape[0]
    adist = fp.alignment_distribution(slab, table, temperature)
    sdist = fp.sequence_distribution(slab, table, temperature)
    assert abs(sum(adist.values()) - 1.0) < 1e-12 and abs(sum(sdist.values()) - 1.0) < 1e-12
    acount, scount = {}, {}
    for b in range(tokens.shape[0]):
        for k in range(tokens.shape[1]):
            a = tuple(labels[b, k, :T].tolist())
            s = tuple(tokens[b, k, :lengths[b, k]].tolist())
            acount[a] = acount.get(a, 0) + 1
            scount[s] = scount.get(s, 0) + 1
    worst = 0.0
    for dist, count in ((adist, acount), (sdist, scount)):
        assert all(dist.get(key, 0.0) > 0.0 for key in count), [key for key in count if not dist.get(key, 0.0) > 0.0]
        for key, p in dist.items():
            f = count.get(key, 0) / n
            bound = 5.0 * np.sqrt(p * (1.0 - p) / n)
            worst = max(worst, abs(f - p) / bound if bound > 0 else 0.0)
            assert abs(f - p) <= bound, (key, f, p, bound)
    print(f"[asg_sample] frequencies: worst deviation {worst:.2f} of the 5-sigma bound")


def test_statistical_case_on_the_yardstick():
    slab, table = stat_model()
    em = np.broadcast_to(slab, (STAT_B,) + slab.shape).copy()
    tokens, lengths, logq, labels, logz = fp.sample_ref(em, table, None, STAT_N, STAT_SEED, 1.0)
    check_frequencies(labels, tokens, lengths, slab, table)
    # no sample went through the forbidden bigram, and logq is the alignment's log-probability
    assert not ((labels[:, :, :-1] == 0) & (labels[:, :, 1:] == 1)).any()
    adist = fp.alignment_distribution(slab, table)
    for b in range(0, STAT_B, 37):
        for k in range(STAT_N):
            assert abs(float(logq[b, k]) - np.log(adist[tuple(labels[b, k].tolist())])) < 1e-5
    fp.certify(em, table, None, STAT_N, STAT_SEED, 1.0, tokens, lengths, logq, labels, logz)


def test_uniforms_use_their_own_stream():
    """counter (t, b, k >> 2, 1), word k & 3: not the CTC sampler's draws, and nothing depends on the batch around"""
    import ctc_sample_fp
    u = fp.uniforms(5, 4, 17, 9)
    assert (ctc_sample_fp.uniforms(5, 4, 17, 9) != u).mean() > 0.99
    assert (fp.uniforms(5, 2, 17, 9, b0=2) == u[2:]).all()
    assert (fp.uniforms(5, 4, 5, 9) == u[:, :5]).all()
    assert (fp.uniforms(5, 4, 17, 3) == u[:, :, :3]).all()
    assert (fp.uniforms(5 + (1 << 32), 4, 17, 9) != u).mean() > 0.99
    words = fp.philox4x32_10((3, 2, 1, 1), (5, 0))
    assert [float(fp.word_to_uniform(w)) for w in words] == u[2, 4:8, 3].tolist()


def test_logz_is_the_full_connect_score():
    for seed, T, C in ((1, 9, 5), (2, 40, 29), (3, 3, 70)):
        em, table = fp.continuous_case(seed, 1, T, C, scale=1.5)
        want = ctc_fp64.asg_fp64(em[0], table)[0]
        for flt in (fp.filter64, fp.filter32):
            got = flt(em[0], table, 1.0)[2]
            assert abs(got - want) <= 1e-4 * max(1.0, abs(want)), (flt.__name__, got, want)
        assert abs(fp.filter64(em[0], table, 1.0)[2] - want) <= 1e-10 * max(1.0, abs(want))


def _structured(seed, B, T, C):
    """a model whose transitions matter: scale 2 on the table, one forbidden bigram (1 after 0)"""
    rng = np.random.default_rng(seed)
    em = (rng.standard_normal((B, T, C)) * 0.7).astype(np.float32)
    trans = (rng.standard_normal((C, C)) * 2.0).astype(np.float32)
    trans[1, 0] = -np.inf
    start = (rng.standard_normal(C) * 0.5).astype(np.float32)
    return em, fp.table_of(start, trans)


def _tokens_of(labels, ctc_blank=None):
    B, N, T = labels.shape
    tk = np.full((B, N, T), -1, np.int32)
    ln = np.zeros((B, N), np.int32)
    for b in range(B):
        for k in range(N):
            seq = fp.merge(labels[b, k])
            if ctc_blank is not None:
                seq = [c for c in seq if c != ctc_blank]
            tk[b, k, :len(seq)] = seq
            ln[b, k] = len(seq)
    return tk, ln


def _inverse_cdf(mass, u):
    cum = np.cumsum(mass)
    idx = int(np.searchsorted(cum, u * cum[-1], side="right"))
    return min(idx, int(np.flatnonzero(mass > 0)[-1]))


def _rejected(em, table, N, seed, tau, labels, logq=None, what=None, **kw):
    tk, ln = _tokens_of(labels, **kw)
    try:
        fp.certify(em, table, None, N, seed, tau, tk, ln, logq, labels)
    except AssertionError as e:
        assert what is None or what in str(e), (what, str(e)[:300])
        return True
    return False


def test_the_certificate_has_teeth():
    B, T, C, N, seed = 2, 12, 5, 8, 77
    em, table = _structured(seed, B, T, C)
    start, W = fp.split(table, C)
    for dtype in (np.float64, np.float32):
        out = fp.sample_ref(em, table, None, N, seed, 1.0, dtype=dtype)
        worst = fp.certify(em, table, None, N, seed, 1.0, *out, tag=dtype.__name__)
        print(f"[asg_sample] certificate C={C} {dtype.__name__}: worst miss {worst:.2e} of the tolerance")
    tokens, lengths, logq, labels, logz = fp.sample_ref(em, table, None, N, seed, 1.0)
    u = fp.uniforms(seed, B, N, T)
    # 1. the last frame's label moved by one where the neighbour's mass exceeds twice the tolerance
    moved = caught = 0
    for b in range(B):
        la = fp.filter64(em[b], table)[0]
        d = fp.drift(la, fp.filter32(em[b], table)[0])
        mass = np.exp(la[T - 1])
        mass /= mass.sum()
        for k in range(N):
            j = int(labels[b, k, T - 1])
            nb = j + 1 if j + 1 < C else j - 1
            if mass[nb] > 2.0 * (fp.tol(C) + 32.0 * d):
                bad = labels.copy()
                bad[b, k, T - 1] = nb
                moved += 1
                caught += _rejected(em, table, N, seed, 1.0, bad)
    assert moved >= B * N // 2 and caught == moved, (moved, caught)
    # 2. per frame from the frame marginals, ignoring the table;  3. forward, each frame given its predecessor only
    per_frame, forward = labels.copy(), labels.copy()
    for b in range(B):
        for k in range(N):
            for t in range(T):
                x = em[b, t].astype(np.float64)
                per_frame[b, k, t] = _inverse_cdf(np.exp(x - x.max()), u[b, k, t])
                w = start if t == 0 else W[:, forward[b, k, t - 1]]
                y = fp.clean(w) + x
                forward[b, k, t] = _inverse_cdf(np.exp(y - y.max()), u[b, k, t])
    assert _rejected(em, table, N, seed, 1.0, per_frame)
    assert _rejected(em, table, N, seed, 1.0, forward, what="bracket")
    # 4. a label through the forbidden bigram
    b, k, t = np.argwhere(labels[:, :, 1:] == 1)[0]  # (frame t + 1 has label 1: label 0 at frame t is forbidden)
    bad = labels.copy()
    bad[b, k, t] = 0
    assert _rejected(em, table, N, seed, 1.0, bad, what="without mass")
    # 5. tokens that are the CTC collapse (label 0 dropped as a blank) instead of the merge
    assert (labels == 0).any()
    assert _rejected(em, table, N, seed, 1.0, labels, what="length", ctc_blank=0) or \
        _rejected(em, table, N, seed, 1.0, labels, what="tokens", ctc_blank=0)
    assert not _rejected(em, table, N, seed, 1.0, labels, logq)
    # 6. logq judged at the wrong temperature: the labels of tau = 0.5 with the log-probabilities they have at tau = 1
    half = fp.sample_ref(em, table, None, N, seed, 0.5)
    fp.certify(em, table, None, N, seed, 0.5, *half)
    z1 = [fp.filter64(em[b], table, 1.0)[2] for b in range(B)]
    lq1 = np.array([[fp.score_of(em[b], table, half[3][b, k]) - z1[b] for k in range(N)] for b in range(B)], np.float32)
    with pytest.raises(AssertionError, match="logq"):
        fp.certify(em, table, None, N, seed, 0.5, half[0], half[1], lq1, half[3], half[4])
    with pytest.raises(AssertionError):  # (and the draws themselves fail when judged at tau = 1)
        fp.certify(em, table, None, N, seed, 1.0, half[0], half[1], None, half[3])
    # a wrong logz, length or fill
    for what in ("logz", "length", "fill"):
        tk, ln, lz = tokens.copy(), lengths.copy(), logz.copy()
        if what == "logz":
            lz[0] += np.float32(2e-4 * max(1.0, abs(float(lz[0]))))
        elif what == "length":
            ln[0, 0] += 1
        else:
            tk[0, 0, -1] = -2
        with pytest.raises(AssertionError):
            fp.certify(em, table, None, N, seed, 1.0, tk, ln, logq, labels, lz)


def test_holes_dead_ends_and_no_path_in_the_yardstick():
    em, table = fp.holes_case(11, 3, 30, 9)
    out = fp.sample_ref(em, table, [30, 0, 7], 6, 3, 1.0)
    fp.certify(em, table, [30, 0, 7], 6, 3, 1.0, *out)
    assert (out[3][1] == -1).all() and (out[1][1] == 0).all() and np.isneginf(out[2][1]).all() and np.isneginf(out[4][1])
    assert (out[3][2, :, 7:] == -1).all() and (out[3][2, :, :7] >= 0).all()
    em, table, dead = fp.dead_end_case(5, 2, 20, 6)
    out = fp.sample_ref(em, table, None, 16, 4, 1.0)
    fp.certify(em, table, None, 16, 4, 1.0, *out)
    assert not (out[3][:, :, :-1] == dead).any() and (out[3][:, :, -1] == dead).any()
    # no alignment of finite score: every start forbidden; a frame of -inf
    em, table = fp.continuous_case(6, 3, 8, 4)
    t2 = table.copy()
    t2[:4] = -np.inf
    out = fp.sample_ref(em, t2, None, 3, 1, 1.0)
    assert (out[3] == -1).all() and np.isneginf(out[4]).all() and np.isneginf(out[2]).all()
    em[1, 5] = -np.inf
    out = fp.sample_ref(em, table, None, 3, 1, 1.0)
    fp.certify(em, table, None, 3, 1, 1.0, *out)
    assert (out[3][1] == -1).all() and (out[3][0] >= 0).all() and (out[3][2] >= 0).all()


@pytest.mark.parametrize("C,T,B,N", fp.SHAPES)
def test_the_float32_emulation_passes_on_the_device_cases(C, T, B, N):
    em, table, seed = fp.shape_case(C, T, B, N)
    B = min(B, 4)  # (utterances are independent: four of a case's inputs stand for its seventy here)
    out = fp.sample_ref(em[:B], table, None, N, seed, 1.0, dtype=np.float32)
    worst = fp.certify(em[:B], table, None, N, seed, 1.0, *out, tag="emulation")
    print(f"[asg_sample] emulation C={C} T={T}: worst miss {worst:.2e} of the tolerance")


def test_entry_points_exist(gtn):
    from gtn_amd import torch_loss
    assert callable(torch_loss.asg_sample)
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    assert hasattr(lib, "gtn_asg_sample_n")
    eng = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_amd.so"))
    assert hasattr(eng, "gtnx_batch_asg_sample") and hasattr(eng, "gtnx_batch_asg_sample_stats")
    assert callable(gtn.Batch.asg_sample)
    calls, utterances = gtn.debug_asg_sample_stats()
    assert calls >= 0 and utterances >= 0


def test_argument_errors_name_the_entry(gtn):
    import torch
    import gtn_amd
    from gtn_amd import torch_loss
    batch = gtn.Batch([gtn.linear_graph(2, 8)])  # (not a Batch.linear)
    with pytest.raises(ValueError, match="asg_sample.*row_stride"):
        batch.asg_sample(64, 64, 64)
    with pytest.raises(ValueError, match="asg_sample.*one frame count per element"):
        batch.asg_sample(64, 64, 64, frames=[1, 1], row_stride=2)
    with pytest.raises(ValueError, match="gtnx_batch_asg_sample.*null output pointer"):
        batch.asg_sample(0, 64, 64, row_stride=2)
    with pytest.raises(ValueError, match="gtnx_batch_asg_sample.*null output pointer"):
        batch.asg_sample(64, 0, 64, row_stride=2)
    with pytest.raises(ValueError, match="gtnx_batch_asg_sample.*null table"):
        batch.asg_sample(64, 64, 0, row_stride=2)
    with pytest.raises(ValueError, match="gtnx_batch_asg_sample.*negative row stride"):
        batch.asg_sample(64, 64, 64, row_stride=-1)
    for n in (0, -1, 1025):
        with pytest.raises(ValueError, match="gtnx_batch_asg_sample.*num_samples outside 1 .. 1024"):
            batch.asg_sample(64, 64, 64, num_samples=n, row_stride=2)
    for tau in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="gtnx_batch_asg_sample.*temperature"):
            batch.asg_sample(64, 64, 64, temperature=tau, row_stride=2)
    for seed in (-1, 1 << 64):
        with pytest.raises(ValueError, match="asg_sample: seed"):
            batch.asg_sample(64, 64, 64, seed=seed, row_stride=2)
    # a batch that is not linear: refused where there is a device to ask, loudly where there is none
    if has_gpu():
        with pytest.raises(ValueError, match="gtnx_batch_asg_sample.*not a native linear batch"):
            batch.asg_sample(64, 64, 64, row_stride=2)
    else:
        with pytest.raises(RuntimeError, match="no HIP device"):
            batch.asg_sample(64, 64, 64, row_stride=2)
    # the C ABI itself
    lib = gtn_amd._lib
    p = ctypes.c_void_p
    assert lib.gtnx_batch_asg_sample(None, None, p(64), 4, 0, 1.0, p(64), 2, p(64), None, None, None) == 1
    assert lib.gtnx_batch_asg_sample(batch._h, None, None, 4, 0, 1.0, p(64), 2, p(64), None, None, None) == 1
    assert lib.gtnx_batch_asg_sample(batch._h, None, p(64), 4, 0, 1.0, None, 2, p(64), None, None, None) == 1
    assert lib.gtnx_batch_asg_sample(batch._h, None, p(64), 4, 0, 1.0, p(64), 2, None, None, None, None) == 1
    assert lib.gtnx_batch_asg_sample(batch._h, None, p(64), 0, 0, 1.0, p(64), 2, p(64), None, None, None) == 1
    assert lib.gtnx_batch_asg_sample(batch._h, None, p(64), 4, 0, 0.0, p(64), 2, p(64), None, None, None) == 1
    # the torch entry
    em, tr = torch.zeros(2, 3, 8), torch.zeros(8, 8)
    with pytest.raises(ValueError, match="asg_sample: the number of labels is outside 1 .. 1024"):
        torch_loss.asg_sample(torch.zeros(1, 2, 1025), torch.zeros(1025, 1025))
    with pytest.raises(ValueError, match="asg_sample: the number of labels is outside 1 .. 1024"):
        torch_loss.asg_sample(torch.zeros(1, 2, 0), torch.zeros(0, 0))
    with pytest.raises(ValueError, match="asg_sample: transitions must be"):
        torch_loss.asg_sample(em, torch.zeros(8, 7))
    with pytest.raises(ValueError, match="asg_sample: start must be"):
        torch_loss.asg_sample(em, tr, start=torch.zeros(7))
    with pytest.raises(ValueError, match="asg_sample: an input length outside 0 .. 3"):
        torch_loss.asg_sample(em, tr, input_lengths=[4, 1])
    with pytest.raises(ValueError, match="asg_sample: 1 input lengths for a batch of 2"):
        torch_loss.asg_sample(em, tr, input_lengths=[1])
    for n in (0, 1025):
        with pytest.raises(ValueError, match="asg_sample: num_samples outside"):
            torch_loss.asg_sample(em, tr, num_samples=n)
    for tau in (0.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="asg_sample: temperature"):
            torch_loss.asg_sample(em, tr, temperature=tau)
    for seed in (-1, 1 << 64):
        with pytest.raises(ValueError, match="asg_sample: seed"):
            torch_loss.asg_sample(em, tr, seed=seed)
    with pytest.raises(ValueError, match="asg_sample: emissions must be a float32 tensor"):
        torch_loss.asg_sample(em.double(), tr)
    with pytest.raises(RuntimeError, match="asg_sample: emissions must be a CUDA tensor"):
        torch_loss.asg_sample(em, tr)


def test_seed_none_comes_from_the_default_cpu_generator(gtn):
    """seed=None takes one integer from torch's default CPU generator, so torch.manual_seed repeats a run"""
    import torch
    from gtn_amd import torch_loss
    em, tr = torch.zeros(2, 3, 8), torch.zeros(8, 8)
    states = []
    for _ in range(2):
        torch.manual_seed(1234)
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            torch_loss.asg_sample(em, tr)
        states.append(torch.get_rng_state())
    assert torch.equal(states[0], states[1])
    torch.manual_seed(1234)
    torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64)
    assert torch.equal(torch.get_rng_state(), states[0])


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU behaviour")
def test_asg_sample_fails_loudly_without_gpu(gtn):
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    lib.gtn_asg_sample_n.argtypes = ([ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2 +
                                     [ctypes.c_int, ctypes.c_uint64, ctypes.c_float] + [ctypes.c_void_p] * 5)
    lib.gtn_asg_sample_n.restype = ctypes.c_int
    lib.gtn_criteria_last_error.restype = ctypes.c_char_p
    rc = lib.gtn_asg_sample_n(None, 1, 2, 8, None, None, 4, 0, 1.0, None, None, None, None, None)
    assert rc == -1 and "no HIP device" in lib.gtn_criteria_last_error().decode()
