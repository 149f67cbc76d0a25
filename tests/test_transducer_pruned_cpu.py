"""The pruned (banded) transducer score, the parts that need no GPU: every refusal of the contract
arrives as an invalid-argument error before a device is asked for, through the C ABI and the Python entry, and
torch_loss.transducer_prune_ranges equals a numpy transcription of its rule exactly."""
import ctypes
import re

import numpy as np
import pytest

BAD = [({"x": None}, "null input pointer"), ({"rg": None}, "null input pointer"), ({"fr": None}, "null input pointer"),
       ({"B": -1}, "negative B"), ({"U": 1024}, "U + 1 outside 1 .. 1024"), ({"S": 0}, "S outside 1 .. min(64, U + 1)"),
       ({"S": 65, "U": 100}, "S outside 1 .. min(64, U + 1)"), ({"S": 5}, "S outside 1 .. min(64, U + 1)"),
       ({"T": 0}, "T outside 1 .. 65535"), ({"T": 65536}, "T outside 1 .. 65535"), ({"C": 0}, "C outside 1 .. 2^20"),
       ({"blank": 4}, "blank is not one of the C labels"),
       ({"B": 1 << 16, "T": 1 << 10, "S": 32, "U": 31}, "B * T * S does not fit an int")]


@pytest.mark.parametrize("change,text", BAD, ids=[t + str(sorted(c)) for c, t in BAD])
def test_refusals_come_before_the_device(gtn, change, text):
    import gtn_amd
    lib = gtn_amd._lib
    lib.gtnx_last_error.restype = ctypes.c_char_p
    p = ctypes.c_void_p(64)
    before = gtn.debug_transducer_pruned_stats()
    a = {**dict(x=p, rg=p, y=p, fr=p, tl=p, B=1, T=2, S=2, U=3, C=4, blank=0), **change}
    head = (a["x"], a["rg"], a["y"], a["fr"], a["tl"], a["B"], a["T"], a["S"], a["U"], a["C"], a["blank"], 1)
    for name, tail in (("gtnx_batch_transducer_pruned_score", (p, None)),
                       ("gtnx_batch_transducer_pruned_score_grad", (p, p, None))):
        assert getattr(lib, name)(*head, *tail) == 1, name
        assert lib.gtnx_last_error().decode().startswith(f"[{name}] {text}")
    addr = {k: (None if v is None else 64) for k, v in a.items() if k in ("x", "rg", "y", "fr", "tl")}
    dims = {k: a[k] for k in "BTSUC"}
    with pytest.raises(ValueError, match="blank must be" if "blank" in change else re.escape(text)):
        gtn.transducer_pruned_score(addr["x"], addr["rg"], addr["y"], addr["fr"], addr["tl"], 64, None, a["blank"], **dims)
    assert gtn.debug_transducer_pruned_stats() == before  # (nothing launched)


def test_null_outputs_empty_batches_and_the_occupancy_entry(gtn):
    import gtn_amd
    lib = gtn_amd._lib
    lib.gtnx_last_error.restype = ctypes.c_char_p
    p = ctypes.c_void_p(64)
    head = (p, p, p, p, p, 1, 2, 2, 3, 4, 0, 1)
    assert lib.gtnx_batch_transducer_pruned_score(*head, None, None) == 1
    assert "null scores" in lib.gtnx_last_error().decode()
    assert lib.gtnx_batch_transducer_pruned_score_grad(*head, None, p, None) == 1
    assert "null weights or grad" in lib.gtnx_last_error().decode()
    assert lib.gtnx_batch_transducer_pruned_score(p, p, p, p, p, 0, 2, 2, 3, 4, 0, 1, p, None) == 0  # (B == 0)
    for args, text in (((None, p, p, 1, 2, 3, p), "null input pointer"), ((p, p, p, 1, 2, 3, None), "null occupancy"),
                       ((p, p, p, -1, 2, 3, p), "negative B"), ((p, p, p, 1, 2, 1024, p), "U + 1 outside"),
                       ((p, p, p, 1, 0, 3, p), "T outside")):
        assert lib.gtnx_batch_transducer_occupancy(*args) == 1 and text in lib.gtnx_last_error().decode()
    assert lib.gtnx_batch_transducer_occupancy(p, p, p, 0, 2, 3, p) == 0
    with pytest.raises(ValueError, match="a device address needs B, T, S, U and C"):
        gtn.transducer_pruned_score(64, 64, 64, 64, 64, 64)


def test_torch_entry_argument_errors():
    import torch
    import gtn_amd.torch_loss as tl
    x, y, r = torch.zeros(2, 3, 2, 5), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int64)
    n = torch.ones(2, dtype=torch.int32)
    for args, kw, exc, text in (((x.double(), r, y, n, n), {}, ValueError, "logits must be a float32 tensor"),
                                ((x, r[:, :2], y, n, n), {}, ValueError, r"ranges must be .* \[2, 3\]"),
                                ((x, r.float(), y, n, n), {}, ValueError, "ranges must be"),
                                ((x, r, y, n[:1], n), {}, ValueError, "input_lengths must be"),
                                ((x, r, y[:, :0], n, n), {}, ValueError, "S must be 1 .. min"),
                                ((x, r, y, n, n), {"blank": 5}, ValueError, "blank must be one of the 5 labels"),
                                ((x, r, y, n, n), {}, RuntimeError, "logits must be a CUDA tensor")):
        with pytest.raises(exc, match=text):
            tl.transducer_pruned_score(*args, **kw)
    with pytest.raises(ValueError, match="reduction must be"):
        tl.transducer_pruned_loss(x, r, y, n, n, reduction="avg")
    with pytest.raises(RuntimeError, match="rows must be a CUDA tensor"):
        tl.transducer_occupancy(torch.zeros(2, 3, 4, 3), n, n)


def _ranges_by_the_rule(occ, Tb, Ub, S):
    """DESIGN section 44's rule for one utterance, step by step"""
    T, E = occ.shape[0], max(0, Ub + 1 - S)
    a = []
    for t in range(Tb):
        sums = [occ[t, s:s + S].sum() for s in range(E + 1)]
        hi = min(E, t * (S - 1))
        lo = min(hi, max(0, E - (Tb - 1 - t) * (S - 1)))
        a.append(min(max(int(np.argmax(sums)), lo), hi))  # (argmax: the smallest start among the largest)
    m = [min(a[t:]) for t in range(Tb)]
    r = [0]
    for t in range(1, Tb):
        r.append(min(m[t], r[-1] + S - 1))
    return r + [r[-1]] * (T - Tb)


# E == 0; E > (T_b - 1)(S - 1); plain; and, in every random plane, frames whose best window would break monotonicity
# or jump by more than S - 1 (asserted below on the unconstrained starts)
@pytest.mark.parametrize("T,U,S,lengths", [(6, 3, 4, [(6, 3), (3, 2)]), (4, 12, 3, [(4, 12), (2, 9)]),
                                           (12, 10, 4, [(12, 10), (7, 5), (1, 0), (12, 3)])])
def test_prune_ranges_equals_the_rule(T, U, S, lengths):
    import torch
    import gtn_amd.torch_loss as tl
    rng = np.random.default_rng(T + U)
    occ = rng.integers(0, 4, (len(lengths), T, U + 1)).astype(np.float32)  # (small integers: window sums are exact)
    if T == 12:  # (the best window jumps by 7 and then falls back to 0)
        occ[0, 4, :4], occ[0, 5, 7:], occ[0, 6, :4] = 9, 9, 9
    fr, tl_ = np.asarray([l[0] for l in lengths]), np.asarray([l[1] for l in lengths])
    got = tl.transducer_prune_ranges(torch.from_numpy(occ), torch.from_numpy(fr), torch.from_numpy(tl_), S).numpy()
    want = np.asarray([_ranges_by_the_rule(occ[b], int(fr[b]), int(tl_[b]), S) for b in range(len(lengths))])
    assert got.dtype == np.int32 and (got == want).all(), (got, want)
    for b, (Tb, Ub) in enumerate(lengths):
        step, E = np.diff(got[b, :Tb]), max(0, Ub + 1 - S)
        assert got[b, 0] == 0 and (step >= 0).all() and (step <= S - 1).all()
        assert got[b, Tb - 1] == E or E > (Tb - 1) * (S - 1)
    if T == 12:
        raw = np.diff([int(np.argmax([occ[0, t, s:s + S].sum() for s in range(U + 2 - S)])) for t in range(T)])
        assert (raw < 0).any() and (raw > S - 1).any()
