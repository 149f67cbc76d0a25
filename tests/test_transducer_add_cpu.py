"""The transducer score under an additive joint, the parts that need no GPU: the argument errors of
gtn_amd.torch_loss.transducer_add_score / transducer_add_loss and the engine's refusals through the C ABI for everything
it validates before the first device call."""
import ctypes

import pytest


def test_torch_entry_argument_errors():
    import torch
    import gtn_amd.torch_loss as tl
    am, lm, y = torch.zeros(2, 3, 5), torch.zeros(2, 4, 5), torch.zeros(2, 3, dtype=torch.int32)
    n = torch.ones(2, dtype=torch.int32)
    for args, kw, exc, text in (((am.double(), lm, y, n, n), {}, ValueError, "am must be a float32 tensor"),
                                ((am, lm.half(), y, n, n), {}, ValueError, "lm must be a float32 tensor"),
                                ((am[0], lm, y, n, n), {}, ValueError, "am must be a float32 tensor"),
                                ((am, lm[:, :, None], y, n, n), {}, ValueError, "lm must be a float32 tensor"),
                                ((am, lm[:, :, :4], y, n, n), {}, ValueError, "must agree in B and C"),
                                ((am, lm[:1], y, n, n), {}, ValueError, "must agree in B and C"),
                                ((am, lm, y[:, :2], n, n), {}, ValueError, r"targets must be .* \[2, 3\]"),
                                ((am, lm, y.float(), n, n), {}, ValueError, "targets must be"),
                                ((am, lm, y, n[:1], n), {}, ValueError, "input_lengths must be"),
                                ((am, lm, y, n, [1, 1]), {}, ValueError, "target_lengths must be"),
                                ((am, lm, y, n, n), {"blank": 5}, ValueError, "blank must be one of the 5 labels"),
                                ((am[:1, :, :1], torch.zeros(1, 1025, 1), torch.zeros(1, 1024, dtype=torch.int32),
                                  n[:1], n[:1]), {}, ValueError, "U \\+ 1 must be 1 .. 1024"),
                                ((am[:, :0], lm, y, n, n), {}, ValueError, "T must be 1 .. 65535"),
                                ((am, lm, y, n, n), {}, RuntimeError, "am must be a CUDA tensor")):
        with pytest.raises(exc, match=text):
            tl.transducer_add_score(*args, **kw)
    with pytest.raises(ValueError, match="reduction must be"):
        tl.transducer_add_loss(am, lm, y, n, n, reduction="avg")


def test_engine_refusals_come_before_the_device(gtn):
    import gtn_amd
    lib = gtn_amd._lib
    lib.gtnx_last_error.restype = ctypes.c_char_p
    p = ctypes.c_void_p(64)
    before = gtn.debug_transducer_add_stats()
    ok = dict(am=p, lm=p, y=p, fr=p, tl=p, B=1, T=2, U=3, C=4, blank=0)
    for change, text in (({"am": None}, "null input pointer"), ({"lm": None}, "null input pointer"),
                         ({"tl": None}, "null input pointer"), ({"B": -1}, "negative B"),
                         ({"U": 1024}, "U + 1 outside 1 .. 1024"), ({"T": 0}, "T outside 1 .. 65535"),
                         ({"T": 65536}, "T outside 1 .. 65535"), ({"C": (1 << 20) + 1}, "C outside 1 .. 2^20"),
                         ({"blank": 4}, "blank is not one of the C labels"),
                         ({"B": 1 << 16, "T": 1 << 10, "U": 31}, "B * T * (U + 1) does not fit an int")):
        a = {**ok, **change}
        head = (a["am"], a["lm"], a["y"], a["fr"], a["tl"], a["B"], a["T"], a["U"], a["C"], a["blank"])
        for name, tail in (("gtnx_batch_transducer_add_score", (p, None)),
                           ("gtnx_batch_transducer_add_score_grad", (p, p, p, None))):
            assert getattr(lib, name)(*head, *tail) == 1, (name, text)
            assert lib.gtnx_last_error().decode() == f"[{name}] {text}" + (
                " (am, lm, targets, frames and target_lengths are all read)" if "null input" in text else "")
    head = (p, p, p, p, p, 1, 2, 3, 4, 0)
    assert lib.gtnx_batch_transducer_add_score(*head, None, None) == 1 and "null scores" in lib.gtnx_last_error().decode()
    assert lib.gtnx_batch_transducer_add_score_grad(*head, p, p, None, None) == 1
    assert "null weights or grad" in lib.gtnx_last_error().decode()
    assert lib.gtnx_batch_transducer_add_score(p, p, p, p, p, 0, 2, 3, 4, 0, p, None) == 0  # (no utterance: nothing to do)
    assert lib.gtnx_batch_transducer_add_score_grad(p, p, p, p, p, 0, 2, 3, 4, 0, p, p, p, None) == 0
    assert gtn.debug_transducer_add_stats() == before  # (nothing launched)
    with pytest.raises(ValueError, match="a device address needs B, T, U and C"):
        gtn.transducer_add_score(64, 64, 64, 64, 64, 64)
