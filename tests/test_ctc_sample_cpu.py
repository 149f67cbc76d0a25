"""CTC posterior sampling, the parts that need no GPU: Philox4x32-10 of tests/ctc_sample_fp.py against its known
answers; the uniform is exact in float32 and strictly inside (0, 1); the certificate that test_ctc_sample_gpu.py judges
the kernels by has teeth (a float32 emulation of a device passes it, the same labels shifted by one fail it on more than
90 % of the samples); the statistical case of the GPU file passes on the yardstick with its seed; the entry points
exist, refuse bad arguments before they ask for a device, and fail loudly without one."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT, has_gpu
import ctc_sample_fp as fp


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_philox_known_answers():
    """the vectors of the Random123 distribution (kat_vectors: philox4x32 10)"""
    assert _hex(fp.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    ones = 0xFFFFFFFF
    assert _hex(fp.philox4x32_10((ones,) * 4, (ones, ones))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    pi = (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344)
    assert _hex(fp.philox4x32_10(pi, (0xA4093822, 0x299F31D0))) == "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_philox_broadcasts_like_the_scalar_calls():
    t = np.arange(5, dtype=np.uint64)[:, None]
    b = np.arange(3, dtype=np.uint64)[None, :]
    got = fp.philox4x32_10((t, b, 7, 0), (123, 456))
    for i in range(5):
        for j in range(3):
            one = fp.philox4x32_10((i, j, 7, 0), (123, 456))
            assert [int(w[i, j]) for w in got] == [int(w) for w in one]


def test_uniform_is_exact_in_float32_and_inside_the_unit_interval():
    for w in (0, 1, 511, 512, 0x7FFFFFFF, 0x80000000, 0xFFFFFE00, 0xFFFFFFFF, 0x12345678):
        u = float(fp.word_to_uniform(w))
        assert 0.0 < u < 1.0 and float(np.float32(u)) == u, w
    assert float(fp.word_to_uniform(0)) == 2.0 ** -24 and float(fp.word_to_uniform(0xFFFFFFFF)) == 1.0 - 2.0 ** -24
    u = fp.uniforms(99, 3, 5, 200)
    assert u.shape == (3, 5, 200) and (u > 0).all() and (u < 1).all() and (u.astype(np.float32) == u).all()
    assert abs(u.mean() - 0.5) < 0.02


def test_uniforms_do_not_depend_on_the_batch_around_them():
    """counter (t, b, k >> 2, 0), word k & 3: slicing the batch, fewer samples or fewer frames change nothing"""
    u = fp.uniforms(5, 4, 17, 9)
    assert (fp.uniforms(5, 2, 17, 9, b0=2) == u[2:]).all()
    assert (fp.uniforms(5, 4, 5, 9) == u[:, :5]).all()
    assert (fp.uniforms(5, 4, 17, 3) == u[:, :, :3]).all()
    assert (fp.uniforms(6, 4, 17, 9) != u).mean() > 0.99
    assert (fp.uniforms(5 + (1 << 32), 4, 17, 9) != u).mean() > 0.99  # (the high word is the second key word)
    words = fp.philox4x32_10((3, 2, 1, 0), (5, 0))
    assert [float(fp.word_to_uniform(w)) for w in words] == u[2, 4:8, 3].tolist()


CERT_CASES = [(1, 3, 40, 3, 0), (2, 2, 65, 29, 28), (3, 2, 9, 300, -1), (4, 1, 5, 5000, 0)]


@pytest.mark.parametrize("seed,B,T,C,blank", CERT_CASES)
def test_the_certificate_has_teeth(seed, B, T, C, blank):
    """the yardstick's own float64 result and its float32 emulation of a device pass; the same labels shifted by one
    label fail the bracket on more than 90 % of the samples, and a wrong token, length or logq is caught"""
    em = fp.continuous_case(seed, B, T, C)
    N = 5
    for dtype in (np.float64, np.float32):
        tokens, lengths, logq, labels = fp.sample_ref(em, None, blank, N, seed, 1.0, dtype=dtype)
        worst = fp.certify(em, None, blank, N, seed, 1.0, tokens, lengths, logq, labels, tag=str(dtype))
        print(f"[ctc_sample] certificate C={C} {dtype.__name__}: worst miss {worst:.2e} of tol")
        assert worst <= 0.01  # (a serial float32 sum stays at least 100 times inside)
    # shifted labels, sample by sample
    caught = 0
    for b in range(B):
        for k in range(N):
            bad = labels.copy()
            bad[b, k] = (bad[b, k] + 1) % C
            tk = np.full_like(tokens, -1)
            ln = np.zeros_like(lengths)
            for bb in range(B):
                for kk in range(N):
                    seq, _ = fp.collapse(bad[bb, kk].tolist(), blank)
                    tk[bb, kk, :len(seq)] = seq
                    ln[bb, kk] = len(seq)
            try:
                fp.certify(em, None, blank, N, seed, 1.0, tk, ln, None, bad)
            except AssertionError as e:
                caught += "bracket" in str(e)
    assert caught > 0.9 * B * N, caught
    for what in ("token", "length", "logq", "fill"):
        tk, ln, lq, lb = tokens.copy(), lengths.copy(), logq.copy(), labels.copy()
        if what == "token":
            tk[0, 0, 0] += 1
        elif what == "length":
            ln[0, 0] += 1
        elif what == "logq":
            lq[0, 0] *= np.float32(1.0 + 1e-3)
        else:
            tk[0, 0, -1] = 0 if T > 1 and ln[0, 0] < T else -2
        with pytest.raises(AssertionError):
            fp.certify(em, None, blank, N, seed, 1.0, tk, ln, lq, lb)


def test_the_yardstick_never_returns_a_label_without_mass():
    em = fp.holes_case(11, 3, 30, 9)
    em[1, 4] = -np.inf  # utterance 1 has no path
    em[2, :, :-1] = np.nan  # utterance 2: a single finite entry at the last label
    em[2, :, -1] = 2.0
    tokens, lengths, logq, labels = fp.sample_ref(em, [30, 30, 30], 0, 6, 3, 1.0)
    fp.certify(em, [30, 30, 30], 0, 6, 3, 1.0, tokens, lengths, logq, labels)
    assert (labels[1] == -1).all() and (lengths[1] == 0).all() and np.isneginf(logq[1]).all()
    assert (labels[2] == 8).all() and (lengths[2] == 1).all() and (logq[2] == 0).all()
    assert np.isfinite(em[0][np.arange(30)[None, :], labels[0]]).all()
    # T_b = 0 beside an ordinary neighbour
    tokens, lengths, logq, labels = fp.sample_ref(em, [30, 0, 7], 0, 2, 3, 1.0)
    assert (labels[1] == -1).all() and (labels[2, :, 7:] == -1).all() and (labels[2, :, :7] == 8).all()


def test_temperature_and_frame_counts_in_the_yardstick():
    em = fp.continuous_case(8, 2, 12, 7)
    for tau in (0.5, 2.0):
        out = fp.sample_ref(em, [12, 5], 0, 4, 21, tau)
        fp.certify(em, [12, 5], 0, 4, 21, tau, *out)
        with pytest.raises(AssertionError):  # (judged at another temperature the same labels fail)
            fp.certify(em, [12, 5], 0, 4, 21, 1.0, out[0], out[1], None, out[3])
    full = fp.sample_ref(em[1:, :5], None, 0, 4, 21, 1.0)
    part = fp.sample_ref(em, [12, 5], 0, 4, 21, 1.0)
    # (utterance 1 alone is utterance 0 of its own batch: another counter, other draws; the same batch index repeats)
    again = fp.sample_ref(em, [3, 5], 0, 4, 21, 1.0)
    assert (again[3][1] == part[3][1]).all() and (again[2][1] == part[2][1]).all()
    assert (again[3][0, :, :3] == part[3][0, :, :3]).all()
    assert full[3].shape == (1, 4, 5)


# the statistical case of test_ctc_sample_gpu.py: 256 copies of one slab, N = 16
STAT_SEED, STAT_B, STAT_N = 20240, 256, 16


def stat_slab():
    return np.array([[-0.3, -1.9, -2.2], [-1.2, -0.9, -1.3], [-2.0, -0.4, -1.7]], np.float32)


def check_frequencies(tokens, lengths, slab, blank=0):
    """the frequency of every label sequence over the B * N samples is within 5 sqrt(p (1 - p) / n) of its probability"""
    dist = fp.sequence_distribution(slab, blank)
    assert abs(sum(dist.values()) - 1.0) < 1e-12
    n = tokens.shape[0] * tokens.shape[1]
    counts = {}
    for b in range(tokens.shape[0]):
        for k in range(tokens.shape[1]):
            key = tuple(tokens[b, k, :lengths[b, k]].tolist())
            counts[key] = counts.get(key, 0) + 1
    assert set(counts) <= set(dist), set(counts) - set(dist)
    for key, p in dist.items():
        f = counts.get(key, 0) / n
        bound = 5.0 * np.sqrt(p * (1.0 - p) / n)
        print(f"[ctc_sample] sequence {key}: frequency {f:.4f} probability {p:.4f} bound {bound:.4f}")
        assert abs(f - p) <= bound, (key, f, p, bound)


def test_statistical_case_on_the_yardstick():
    slab = stat_slab()
    em = np.broadcast_to(slab, (STAT_B,) + slab.shape).copy()
    tokens, lengths, logq, labels = fp.sample_ref(em, None, 0, STAT_N, STAT_SEED, 1.0)
    check_frequencies(tokens, lengths, slab)


def test_entry_points_exist(gtn):
    from gtn_amd import torch_loss
    assert callable(torch_loss.ctc_sample)
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    assert hasattr(lib, "gtn_ctc_sample_n")
    eng = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_amd.so"))
    assert hasattr(eng, "gtnx_batch_ctc_sample") and hasattr(eng, "gtnx_batch_ctc_sample_stats")
    assert callable(gtn.Batch.ctc_sample)
    calls, utterances = gtn.debug_ctc_sample_stats()
    assert calls >= 0 and utterances >= 0


def test_argument_errors_come_before_the_device(gtn):
    """what the arguments alone decide is refused as an invalid argument, with or without a device (the checks that
    need a native linear batch are reached on the device only: test_ctc_sample_gpu.py; their torch counterparts are
    here)"""
    import torch
    import gtn_amd
    from gtn_amd import torch_loss
    batch = gtn.Batch([gtn.linear_graph(2, 8)])
    with pytest.raises(ValueError, match="row_stride"):
        batch.ctc_sample(64, 64)
    with pytest.raises(ValueError, match="one frame count per element"):
        batch.ctc_sample(64, 64, frames=[1, 1], row_stride=2)
    with pytest.raises(ValueError, match="null output pointer"):
        batch.ctc_sample(0, 64, row_stride=2)
    with pytest.raises(ValueError, match="null output pointer"):
        batch.ctc_sample(64, 0, row_stride=2)
    with pytest.raises(ValueError, match="negative row stride"):
        batch.ctc_sample(64, 64, row_stride=-1)
    for n in (0, -1, 1025):
        with pytest.raises(ValueError, match="num_samples outside 1 .. 1024"):
            batch.ctc_sample(64, 64, num_samples=n, row_stride=2)
    for tau in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            batch.ctc_sample(64, 64, temperature=tau, row_stride=2)
    for seed in (-1, 1 << 64):
        with pytest.raises(ValueError, match="seed"):
            batch.ctc_sample(64, 64, seed=seed, row_stride=2)
    # the C ABI itself
    lib = gtn_amd._lib
    p = ctypes.c_void_p
    assert lib.gtnx_batch_ctc_sample(None, None, 0, 4, 0, 1.0, p(64), 2, p(64), None, None) == 1
    assert lib.gtnx_batch_ctc_sample(batch._h, None, 0, 4, 0, 1.0, None, 2, p(64), None, None) == 1
    assert lib.gtnx_batch_ctc_sample(batch._h, None, 0, 4, 0, 1.0, p(64), 2, None, None, None) == 1
    assert lib.gtnx_batch_ctc_sample(batch._h, None, 0, 0, 0, 1.0, p(64), 2, p(64), None, None) == 1
    assert lib.gtnx_batch_ctc_sample(batch._h, None, 0, 4, 0, 0.0, p(64), 2, p(64), None, None) == 1
    em = torch.zeros(2, 3, 8)
    with pytest.raises(ValueError, match="blank must be below"):
        torch_loss.ctc_sample(em, blank=8)
    with pytest.raises(ValueError, match="input length outside 0 .. 3"):
        torch_loss.ctc_sample(em, input_lengths=[4, 1])
    with pytest.raises(ValueError, match="input lengths for a batch of 2"):
        torch_loss.ctc_sample(em, input_lengths=[1])
    with pytest.raises(ValueError, match="num_samples outside"):
        torch_loss.ctc_sample(em, num_samples=0)
    with pytest.raises(ValueError, match="num_samples outside"):
        torch_loss.ctc_sample(em, num_samples=1025)
    with pytest.raises(ValueError, match="temperature"):
        torch_loss.ctc_sample(em, temperature=0.0)
    with pytest.raises(ValueError, match="temperature"):
        torch_loss.ctc_sample(em, temperature=float("nan"))
    with pytest.raises(ValueError, match="seed"):
        torch_loss.ctc_sample(em, seed=-1)
    with pytest.raises(ValueError, match="float32 tensor"):
        torch_loss.ctc_sample(em.double())
    with pytest.raises(ValueError, match="float32 tensor"):
        torch_loss.ctc_sample(em[0])
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        torch_loss.ctc_sample(em)


def test_seed_none_comes_from_the_default_cpu_generator(gtn, monkeypatch):
    """seed=None takes one integer from torch's default CPU generator, so torch.manual_seed repeats a run: the two
    calls below reach the CUDA check with the generator advanced by the same single draw"""
    import torch
    from gtn_amd import torch_loss
    em = torch.zeros(2, 3, 8)
    states = []
    for _ in range(2):
        torch.manual_seed(1234)
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            torch_loss.ctc_sample(em)
        states.append(torch.get_rng_state())
    assert torch.equal(states[0], states[1])
    torch.manual_seed(1234)
    want = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
    assert torch.equal(torch.get_rng_state(), states[0]) and 0 <= want < 2 ** 63


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU behaviour")
def test_ctc_sample_fails_loudly_without_gpu(gtn):
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    lib.gtn_ctc_sample_n.argtypes = ([ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_int,
                                     ctypes.c_uint64, ctypes.c_float] + [ctypes.c_void_p] * 4)
    lib.gtn_ctc_sample_n.restype = ctypes.c_int
    lib.gtn_criteria_last_error.restype = ctypes.c_char_p
    rc = lib.gtn_ctc_sample_n(None, 1, 2, 8, 0, None, 4, 0, 1.0, None, None, None, None)
    assert rc == -1 and "no HIP device" in lib.gtn_criteria_last_error().decode()
    with pytest.raises(RuntimeError, match="no HIP device"):
        gtn.Batch([gtn.linear_graph(2, 8)]).ctc_sample(64, 64, row_stride=2)
