"""The batched token-and-duration transducer (TDT) score, the parts that need no GPU: the yardstick
of tests/transducer_tdt_fp.py against brute-force enumeration of every path and central differences, and every refusal
of the engine (through the C ABI, before the first device call), of gtn_amd.transducer_tdt_score and of
gtn_amd.torch_loss.transducer_tdt_score."""
import ctypes
import itertools

import numpy as np
import pytest

import transducer_tdt_fp as fp


def _brute(lt, ld, y, blank, t=0, u=0):
    """log of the sum over every path from (t, u): any arc that stays inside, a blank arc onto frame T at u == U ends"""
    T, D, total = lt.shape[0], ld.shape[2], -np.inf
    for d in range(D):
        if d >= 1:
            if t + d < T:
                total = np.logaddexp(total, lt[t, u, blank] + ld[t, u, d] + _brute(lt, ld, y, blank, t + d, u))
            elif t + d == T and u == len(y):
                total = np.logaddexp(total, lt[t, u, blank] + ld[t, u, d])
        if u < len(y) and t + d < T:
            total = np.logaddexp(total, lt[t, u, y[u]] + ld[t, u, d] + _brute(lt, ld, y, blank, t + d, u + 1))
    return total


@pytest.mark.parametrize("T,U,D", [(1, 0, 2), (1, 2, 3), (2, 1, 5), (4, 2, 3), (5, 1, 2)])
def test_yardstick_against_every_path(T, U, D):
    rng = np.random.default_rng(T * 100 + U * 10 + D)
    C, blank, eps, sigma = 4, 1, 1e-6, 0.05
    x = rng.standard_normal((1, T, U + 1, C + D))
    y = np.asarray([[0, 3][:U]], np.int32)
    lt = x[0, :, :, :C] - np.logaddexp.reduce(x[0, :, :, :C], axis=2, keepdims=True) - sigma
    ld = x[0, :, :, C:] - np.logaddexp.reduce(x[0, :, :, C:], axis=2, keepdims=True)
    args = (y, np.asarray([T]), np.asarray([U]), C, blank, sigma, np.asarray([-0.5]))
    score, grad = fp.reference(x, *args)
    assert abs(score[0] - _brute(lt, ld, y[0], blank)) <= 1e-12
    for idx in itertools.product(range(T), range(U + 1), range(C + D)):  # (the gradient against central differences)
        hi, lo = x.copy(), x.copy()
        hi[(0,) + idx] += eps
        lo[(0,) + idx] -= eps
        fd = -0.5 * (fp.reference(hi, *args)[0][0] - fp.reference(lo, *args)[0][0]) / (2 * eps)
        assert abs(grad[(0,) + idx] - fd) <= 1e-8, idx
    assert np.abs(grad[..., :C].sum(axis=3)).max() <= 1e-12 and np.abs(grad[..., C:].sum(axis=3)).max() <= 1e-12


def test_engine_refusals_come_before_the_device(gtn):
    import gtn_amd
    lib = gtn_amd._lib
    lib.gtnx_last_error.restype = ctypes.c_char_p
    p = ctypes.c_void_p(64)
    before = gtn.debug_transducer_tdt_stats()
    ok = dict(x=p, y=p, fr=p, tl=p, B=1, T=2, U=3, C=4, D=5, blank=0, sigma=0.0)
    for change, text in (({"x": None}, "null input pointer"), ({"tl": None}, "null input pointer"),
                         ({"B": -1}, "negative B"), ({"U": 1024}, "U + 1 outside 1 .. 1024"),
                         ({"T": 0}, "T outside 1 .. 65535"), ({"T": 65536}, "T outside 1 .. 65535"),
                         ({"D": 1}, "D outside 2 .. 8"), ({"D": 9}, "D outside 2 .. 8"),
                         ({"C": 0}, "C < 1 or C + D above 2^20"), ({"C": (1 << 20) - 4}, "C < 1 or C + D above 2^20"),
                         ({"blank": 4}, "blank is not one of the C tokens"), ({"blank": -1}, "blank is not one of the C tokens"),
                         ({"sigma": -0.5}, "sigma must be finite and >= 0"), ({"sigma": float("nan")}, "sigma must be finite and >= 0"),
                         ({"sigma": float("inf")}, "sigma must be finite and >= 0"),
                         ({"B": 1 << 16, "T": 1 << 10, "U": 31}, "B * T * (U + 1) does not fit an int")):
        a = {**ok, **change}
        head = (a["x"], a["y"], a["fr"], a["tl"], a["B"], a["T"], a["U"], a["C"], a["D"], a["blank"], a["sigma"])
        for name, tail in (("gtnx_batch_transducer_tdt_score", (p, None)),
                           ("gtnx_batch_transducer_tdt_score_grad", (p, p, None))):
            assert getattr(lib, name)(*head, *tail) == 1, (name, text)
            assert lib.gtnx_last_error().decode() == f"[{name}] {text}" + (
                " (logits, targets, frames and target_lengths are all read)" if "null input" in text else "")
    head = (p, p, p, p, 1, 2, 3, 4, 5, 0, 0.0)
    assert lib.gtnx_batch_transducer_tdt_score(*head, None, None) == 1
    assert "null scores" in lib.gtnx_last_error().decode()
    for tail in ((None, p, None), (p, None, None)):
        assert lib.gtnx_batch_transducer_tdt_score_grad(*head, *tail) == 1
        assert "null weights or grad" in lib.gtnx_last_error().decode()
    assert lib.gtnx_batch_transducer_tdt_score(p, p, p, p, 0, 2, 3, 4, 5, 0, 0.0, p, None) == 0  # (B == 0: nothing to do)
    assert lib.gtnx_batch_transducer_tdt_score_grad(p, p, p, p, 0, 2, 3, 4, 5, 0, 0.0, p, p, None) == 0
    assert gtn.debug_transducer_tdt_stats() == before  # (nothing launched)


def test_python_entries_refuse_without_a_device(gtn):
    import torch
    import gtn_amd.torch_loss as tl
    x, y = torch.zeros(2, 3, 4, 9), torch.zeros(2, 3, dtype=torch.int32)
    n, s, g = torch.ones(2, dtype=torch.int32), torch.zeros(2), torch.zeros(2, 3, 4, 9)
    for args, kw, text in (((64, 64, 64, 64, 64, 5), {}, "a device address needs B, T, U and C"),
                           ((x, y, n, n, s, 1), {}, "D must be in 2 .. 8"), ((x, y, n, n, s, 9), {}, "D must be in 2 .. 8"),
                           ((x, y, n, n, s, 5), {"sigma": -1.0}, "sigma must be finite"),
                           ((x, y, n, n, s, 5), {"sigma": float("nan")}, "sigma must be finite"),
                           ((x, y, n, n, s, 5), {"blank": 4}, "blank must be one of the 4 tokens"),
                           ((x.double(), y, n, n, s, 5), {}, "logits must be a float32 contiguous tensor"),
                           ((x[0], y, n, n, s, 5), {}, "logits must be a float32 contiguous tensor"),
                           ((x, y, n, n, s, 5), {"C": 5}, "C = 5 is not what logits says"),
                           ((x, y[:, :2], n, n, s, 5), {}, "targets must be"), ((x, y, n.long(), n, s, 5), {}, "frames must be"),
                           ((x, y, n, n, s[:1], 5), {}, "scores_out must be"),
                           ((x, y, n, n, s, 5), {"rows_out": torch.zeros(2, 3, 4, 3)}, "rows_out must be"),
                           ((x, y, n, n, s, 5), {}, "logits must be a CUDA tensor")):
        with pytest.raises(ValueError, match=text):
            gtn.transducer_tdt_score(*args, **kw)
    with pytest.raises(ValueError, match="grad_out must be"):
        gtn.transducer_tdt_score_grad(x, y, n, n, s, g[:1], 5)
    with pytest.raises(ValueError, match="logits must be a CUDA tensor"):
        gtn.transducer_tdt_score_grad(x, y, n, n, s, g, 5)
    with pytest.raises(Exception, match="U \\+ 1 outside 1 .. 1024"):  # (sizes that need no tensor: the engine's refusal)
        gtn.transducer_tdt_score(64, 64, 64, 64, 64, 5, B=1, T=2, U=1024, C=4)
    for args, kw, exc, text in (((x, y, n, n, 1), {}, ValueError, "num_durations must be 2 .. 8"),
                                ((x.double(), y, n, n, 5), {}, ValueError, "logits must be a float32 tensor"),
                                ((x, y.float(), n, n, 5), {}, ValueError, "targets must be"),
                                ((x, y, n, n[:1], 5), {}, ValueError, "target_lengths must be"),
                                ((x, y, n, n, 5), {"blank": 4}, ValueError, "blank must be one of the 4 tokens"),
                                ((x, y, n, n, 5), {"sigma": -0.1}, ValueError, "sigma must be finite"),
                                ((torch.zeros(1, 1, 1025, 3), torch.zeros(1, 1024, dtype=torch.int32), n[:1], n[:1], 2),
                                 {}, ValueError, "U \\+ 1 must be 1 .. 1024"),
                                ((x, y, n, n, 5), {}, RuntimeError, "logits must be a CUDA tensor")):
        with pytest.raises(exc, match=text):
            tl.transducer_tdt_score(*args, **kw)
    with pytest.raises(ValueError, match="reduction must be"):
        tl.transducer_tdt_loss(x, y, n, n, 5, reduction="avg")
