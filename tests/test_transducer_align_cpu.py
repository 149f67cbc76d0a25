"""The batched transducer forced alignment, the parts that need no GPU: the yardstick of
tests/transducer_align_fp.py against brute-force enumeration of every alignment, the engine's refusals through the C
ABI before the first device call, and the argument errors of gtn_amd.torch_loss.transducer_align / _rows."""
import ctypes
import itertools

import numpy as np
import pytest

import transducer_align_fp as afp


def _brute(lp, y, blank):
    """(score, the frame of every label) of the best of all alignments (the draws are continuous: no ties)"""
    T, U = lp.shape[0], len(y)
    best = (-np.inf, None)
    for labels_at in itertools.combinations(range(T - 1 + U), U):
        t = u = 0
        score, frames = 0.0, []
        for step in range(T - 1 + U):
            if step in labels_at:
                score, u = score + lp[t, u, y[u]], u + 1
                frames.append(t)
            else:
                score, t = score + lp[t, u, blank], t + 1
        best = max(best, (score + lp[T - 1, U, blank], frames), key=lambda p: p[0])
    return best


@pytest.mark.parametrize("T,U", [(1, 0), (1, 2), (2, 1), (3, 2)])
@pytest.mark.parametrize("normalize", [True, False])
def test_yardstick_against_every_alignment(T, U, normalize):
    rng = np.random.default_rng(T * 10 + U)
    C, blank = 4, 1
    x = rng.standard_normal((1, T, U + 1, C))
    y = np.asarray([[0, 3][:U]], np.int32)
    lp = x[0] - (np.logaddexp.reduce(x[0], axis=2, keepdims=True) if normalize else 0.0)
    want, want_frames = _brute(lp, y[0], blank)
    fr, tl = np.asarray([T]), np.asarray([U])
    score, token_frames, token_scores, frame_tokens = afp.reference(x, y, fr, tl, blank, normalize)
    assert abs(score[0] - want) <= 1e-12 and token_frames[0].tolist() == want_frames
    assert np.allclose(token_scores[0], [lp[t, u, y[0, u]] for u, t in enumerate(want_frames)], rtol=0, atol=1e-12)
    assert frame_tokens[0].tolist() == [sum(f <= t for f in want_frames) for t in range(T)]
    plane = afp.planes64(x, y, fr, tl, blank, normalize)[0]
    assert abs(afp.path_score(plane, token_frames[0]) - want) <= 1e-12
    rows = np.stack([plane[0], plane[1], np.zeros_like(plane[0])], axis=2)[None].astype(np.float32)
    got = afp.transcribe(rows, fr, tl)  # (the float32 twin: the same path here, the score within float32)
    assert got[1].tolist() == token_frames.tolist() and abs(got[0][0] - want) <= 1e-5


def test_engine_refusals_come_before_the_device(gtn):
    import gtn_amd
    lib = gtn_amd._lib
    lib.gtnx_last_error.restype = ctypes.c_char_p
    p = ctypes.c_void_p(64)
    before = gtn.debug_transducer_align_stats()
    ok = dict(x=p, y=p, fr=p, tl=p, B=1, T=2, U=3, C=4, blank=0)
    for change, text in (({"x": None}, "null input pointer"), ({"fr": None}, "null input pointer"),
                         ({"B": -1}, "negative B"), ({"U": 1024}, "U + 1 outside 1 .. 1024"),
                         ({"U": -1}, "U + 1 outside 1 .. 1024"), ({"T": 0}, "T outside 1 .. 65535"),
                         ({"T": 65536}, "T outside 1 .. 65535"), ({"C": 0}, "C outside 1 .. 2^20"),
                         ({"C": (1 << 20) + 1}, "C outside 1 .. 2^20"), ({"blank": 4}, "blank is not one of the C labels"),
                         ({"B": 1 << 16, "T": 1 << 10, "U": 31}, "B * T * (U + 1) does not fit an int")):
        a = {**ok, **change}
        tail = (a["y"], a["fr"], a["tl"], a["B"], a["T"], a["U"], a["C"], a["blank"], 1, None, p, p, None, None)
        for name, head in (("gtnx_batch_transducer_align", (a["x"],)), ("gtnx_batch_transducer_align16", (a["x"], 2))):
            assert getattr(lib, name)(*head, *tail) == 1, (name, text)
            assert lib.gtnx_last_error().decode() == f"[{name}] {text}" + (
                " (logits, targets, frames and target_lengths are all read)" if "null input" in text else "")
        if "C" not in change and "blank" not in change and "x" not in change:
            assert lib.gtnx_batch_transducer_align_rows(p, a["fr"], a["tl"], a["B"], a["T"], a["U"], p, p, None, None) == 1
            assert text in lib.gtnx_last_error().decode()
    tail = (p, p, p, 1, 2, 3, 4, 0, 1, None)
    assert lib.gtnx_batch_transducer_align(p, *tail, None, p, None, None) == 1
    assert "null scores or token_frames" in lib.gtnx_last_error().decode()
    assert lib.gtnx_batch_transducer_align(p, *tail, p, None, None, None) == 1
    assert lib.gtnx_batch_transducer_align16(p, 0, *tail, p, p, None, None) == 1
    assert "must be GTNX_DTYPE_F16 or GTNX_DTYPE_BF16" in lib.gtnx_last_error().decode()
    assert lib.gtnx_batch_transducer_align_rows(None, p, p, 1, 2, 3, p, p, None, None) == 1
    assert lib.gtnx_batch_transducer_align(p, p, p, p, 0, 2, 3, 4, 0, 1, None, p, p, None, None) == 0  # (no utterance)
    assert gtn.debug_transducer_align_stats() == before  # (nothing launched)
    with pytest.raises(ValueError, match="a device address needs B, T, U and C"):
        gtn.transducer_align(64, 64, 64, 64, 64, 64)


def test_torch_entry_argument_errors():
    import torch
    import gtn_amd.torch_loss as tl
    x, y = torch.zeros(2, 3, 4, 5), torch.zeros(2, 3, dtype=torch.int32)
    n = torch.ones(2, dtype=torch.int32)
    rows = torch.zeros(2, 3, 4, 3)
    for args, kw, exc, text in (((x.double(), y, n, n), {}, ValueError, "logits must be a float32 tensor"),
                                ((x, y[:, :2], n, n), {}, ValueError, r"targets must be .* \[2, 3\]"),
                                ((x, y, n, [1, 1]), {}, ValueError, "target_lengths must be"),
                                ((x, y, n, n), {"blank": 5}, ValueError, "blank must be one of the 5 labels"),
                                ((x, y, n, n), {"rows": rows[:, :, :3]}, ValueError, r"rows must be .* \[2, 3, 4, 3\]"),
                                ((torch.zeros(1, 1, 1025, 1), torch.zeros(1, 1024, dtype=torch.int32), n[:1], n[:1]),
                                 {}, ValueError, "U \\+ 1 <= 1024"),
                                ((x, y, n, n), {}, RuntimeError, "logits must be a CUDA tensor")):
        with pytest.raises(exc, match=text):
            tl.transducer_align(*args, **kw)
    for args, exc, text in (((rows[..., :2], n, n), ValueError, "rows must be a float32 tensor"),
                            ((rows, n[:1], n), ValueError, "input_lengths must be"),
                            ((rows, n, n), RuntimeError, "rows must be a CUDA tensor")):
        with pytest.raises(exc, match=text):
            tl.transducer_align_rows(*args)
