"""The batched transducer (RNN-T) score, the parts that need no GPU: the yardstick of
tests/transducer_fp.py against brute-force enumeration of every alignment and against the closed form for U = 0, the
argument errors of gtn_amd.torch_loss.transducer_score / transducer_loss, and the engine's refusals through the C ABI
for everything it validates before the first device call."""
import ctypes
import itertools

import numpy as np
import pytest

import transducer_fp as fp


def _brute(lp, y, blank):
    """log of the sum over every alignment: T - 1 blanks and U labels in any order, then the last blank"""
    T, U = lp.shape[0], len(y)
    total = -np.inf
    for labels_at in itertools.combinations(range(T - 1 + U), U):
        t = u = 0
        score = 0.0
        for step in range(T - 1 + U):
            if step in labels_at:
                score, u = score + lp[t, u, y[u]], u + 1
            else:
                score, t = score + lp[t, u, blank], t + 1
        total = np.logaddexp(total, score + lp[T - 1, U, blank])
    return total


@pytest.mark.parametrize("T,U", [(1, 0), (1, 2), (2, 1), (3, 2)])
@pytest.mark.parametrize("normalize", [True, False])
def test_yardstick_against_every_alignment(T, U, normalize):
    rng = np.random.default_rng(T * 10 + U)
    C, blank, eps = 4, 1, 1e-6
    x = rng.standard_normal((1, T, U + 1, C))
    y = np.asarray([[0, 3][:U]], np.int32)
    lp = x[0] - (np.logaddexp.reduce(x[0], axis=2, keepdims=True) if normalize else 0.0)
    args = (y, np.asarray([T]), np.asarray([U]), blank, normalize, np.asarray([-0.5]))
    score, grad = fp.reference(x, *args)
    assert abs(score[0] - _brute(lp, y[0], blank)) <= 1e-12
    for idx in itertools.product(range(T), range(U + 1), range(C)):  # (the gradient against central differences)
        hi, lo = x.copy(), x.copy()
        hi[(0,) + idx] += eps
        lo[(0,) + idx] -= eps
        fd = -0.5 * (fp.reference(hi, *args)[0][0] - fp.reference(lo, *args)[0][0]) / (2 * eps)
        assert abs(grad[(0,) + idx] - fd) <= 1e-8, idx
    if normalize:
        assert np.abs(grad.sum(axis=3)).max() <= 1e-12  # (a normalised gradient row sums to 0)


def test_yardstick_closed_form_without_labels():
    x = np.random.default_rng(3).standard_normal((2, 7, 1, 5))
    frames = np.asarray([7, 4])
    score, _ = fp.reference(x, np.zeros((2, 0), np.int32), frames, np.zeros(2, np.int32), 2, True, np.ones(2))
    lp = x[:, :, 0, 2] - np.logaddexp.reduce(x[:, :, 0], axis=2)
    assert np.allclose(score, [lp[0].sum(), lp[1, :4].sum()], rtol=0, atol=1e-12)


def test_torch_entry_argument_errors():
    import torch
    import gtn_amd.torch_loss as tl
    x, y = torch.zeros(2, 3, 4, 5), torch.zeros(2, 3, dtype=torch.int32)
    n = torch.ones(2, dtype=torch.int32)
    for args, kw, exc, text in (((x.double(), y, n, n), {}, ValueError, "logits must be a float32 tensor"),
                                ((x[0], y, n, n), {}, ValueError, "logits must be a float32 tensor"),
                                ((x, y[:, :2], n, n), {}, ValueError, r"targets must be .* \[2, 3\]"),
                                ((x, y.float(), n, n), {}, ValueError, "targets must be"),
                                ((x, y, n[:1], n), {}, ValueError, "input_lengths must be"),
                                ((x, y, n, [1, 1]), {}, ValueError, "target_lengths must be"),
                                ((x, y, n, n), {"blank": 5}, ValueError, "blank must be one of the 5 labels"),
                                ((torch.zeros(1, 1, 1025, 1), torch.zeros(1, 1024, dtype=torch.int32), n[:1], n[:1]),
                                 {}, ValueError, "U \\+ 1 must be 1 .. 1024"),
                                ((torch.zeros(1, 0, 1, 1), torch.zeros(1, 0, dtype=torch.int32), n[:1], n[:1]),
                                 {}, ValueError, "T must be 1 .. 65535"),
                                ((x, y, n, n), {}, RuntimeError, "logits must be a CUDA tensor")):
        with pytest.raises(exc, match=text):
            tl.transducer_score(*args, **kw)
    with pytest.raises(ValueError, match="reduction must be"):
        tl.transducer_loss(x, y, n, n, reduction="avg")


def test_engine_refusals_come_before_the_device(gtn):
    import gtn_amd
    lib = gtn_amd._lib
    lib.gtnx_last_error.restype = ctypes.c_char_p
    p = ctypes.c_void_p(64)
    before = gtn.debug_transducer_stats()
    ok = dict(x=p, y=p, fr=p, tl=p, B=1, T=2, U=3, C=4, blank=0)
    for change, text in (({"x": None}, "null input pointer"), ({"fr": None}, "null input pointer"),
                         ({"B": -1}, "negative B"), ({"U": 1024}, "U + 1 outside 1 .. 1024"),
                         ({"U": -1}, "U + 1 outside 1 .. 1024"), ({"T": 0}, "T outside 1 .. 65535"),
                         ({"T": 65536}, "T outside 1 .. 65535"), ({"C": 0}, "C outside 1 .. 2^20"),
                         ({"C": (1 << 20) + 1}, "C outside 1 .. 2^20"), ({"blank": 4}, "blank is not one of the C labels"),
                         ({"B": 1 << 16, "T": 1 << 10, "U": 31}, "B * T * (U + 1) does not fit an int")):
        a = {**ok, **change}
        head = (a["x"], a["y"], a["fr"], a["tl"], a["B"], a["T"], a["U"], a["C"], a["blank"], 1)
        for name, tail in (("gtnx_batch_transducer_score", (p, None)), ("gtnx_batch_transducer_score_grad", (p, p, None))):
            assert getattr(lib, name)(*head, *tail) == 1, (name, text)
            assert lib.gtnx_last_error().decode() == f"[{name}] {text}" + (
                " (logits, targets, frames and target_lengths are all read)" if "null input" in text else "")
    head = (p, p, p, p, 1, 2, 3, 4, 0, 1)
    assert lib.gtnx_batch_transducer_score(*head, None, None) == 1 and "null scores" in lib.gtnx_last_error().decode()
    assert lib.gtnx_batch_transducer_score_grad(*head, None, p, None) == 1
    assert "null weights or grad" in lib.gtnx_last_error().decode()
    assert lib.gtnx_batch_transducer_score(p, p, p, p, 0, 2, 3, 4, 0, 1, p, None) == 0  # (no utterance: nothing to do)
    assert gtn.debug_transducer_stats() == before  # (nothing launched)
    with pytest.raises(ValueError, match="a device address needs B, T, U and C"):
        gtn.transducer_score(64, 64, 64, 64, 64)
