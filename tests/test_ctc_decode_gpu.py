"""Batched CTC best-path decode with device-resident output (linear_decode.hip through gtnx_batch_linear_decode;
gtn_amd.Batch.linear_decode, gtn_amd.torch_loss.ctc_decode, gtn_ctc_decode_n).

The judge is the numpy yardstick of tests/ctc_decode_fp.py, which tests/test_ctc_decode_cpu.py pins to the oracle's
shortestPath on linearGraph(T, C).  Labels, tokens, starts and lengths are compared with ==, and so are the scores: only
the row maxima are added, in frame order from 0 in float32 on both sides, so there is nothing to tolerate.  Every output
is allocated with a guard row and column of sentinels that must survive.
"""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from ctc_decode_fp import continuous_case, decode_batch, holes_case, planted_case, tie_case

pytestmark = pytest.mark.gpu
SENTINEL = -7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("labels", "scores", "tokens", "starts", "lengths")


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True, order="C")).to("cuda:0")  # (the cached cases are read-only)


def _decode(gtn, em, frames=None, rows=None, blank=-1, scores=True, collapsed=True, starts=True, lengths=True, pad=1,
            address=False, batch=None):
    """Batch.linear_decode on Batch.linear (or on `batch`); outputs allocated with a guard row and `pad` guard columns
    of sentinels that must survive (pad > 1: row_stride > T; address: raw device addresses with row_stride).
    Returns ([labels, scores, tokens, starts, lengths] as numpy, None where not asked for, (fast, fallback) counts of
    this call); _decode.raw keeps the arrays with their guards, also when the call raised"""
    import torch
    B, T, C = em.shape
    em_dev = _dev(em)
    ems = batch if batch is not None else gtn.Batch.linear(B, T, C, em_dev, False, True, rows)

    def ints(on):
        return torch.full((B + 1, T + pad), SENTINEL, dtype=torch.int32, device="cuda:0") if on else None
    lab, col, sta = ints(True), ints(collapsed), ints(starts)
    ln = torch.full((B + 1,), SENTINEL, dtype=torch.int32, device="cuda:0") if lengths else None
    sc = torch.full((B + 1,), float("nan"), dtype=torch.float32, device="cuda:0") if scores else None
    torch.cuda.synchronize()

    def view(t):
        if t is None:
            return None
        return t.data_ptr() if address else t[:B, :T]
    f0, b0 = gtn.debug_linear_decode_stats()
    try:
        ems.linear_decode(view(lab), sc, frames, blank, view(col), view(sta), ln,
                          row_stride=T + pad if address else None)
    finally:
        gtn.synchronize()
        f1, b1 = gtn.debug_linear_decode_stats()
        raw = [None if t is None else t.cpu().numpy() for t in (lab, sc, col, sta, ln)]
        _decode.raw = raw
        for name, r in zip(NAMES, raw):
            if r is None:
                continue
            if r.ndim == 2:
                assert (r[B] == SENTINEL).all() and (r[:, T:] == SENTINEL).all(), name
            elif name == "scores":
                assert np.isnan(r[B]), name
            else:
                assert r[B] == SENTINEL, name
    out = [None if r is None else (r[:B, :T] if r.ndim == 2 else r[:B]) for r in raw]
    return out, (f1 - f0, b1 - b0)


def _check(tag, got, want):
    """every output that was asked for == the yardstick's (scores bit for bit; NaN never appears in either)"""
    for name, g, w in zip(NAMES, got, want):
        if g is None:
            continue
        if name == "scores":
            print(f"[ctc_decode] {tag} scores {g[:4]!r} yardstick {w[:4]!r}")
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (tag, name, bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


@functools.lru_cache(maxsize=None)
def _planted(seed, B, T, C, blank, frames=None):
    em = planted_case(seed, B, T, C, blank)
    em.setflags(write=False)
    return em, decode_batch(em, frames, blank)


# C: each lanes-per-row variant (<= 32, <= 64, <= 128, above), rows that are not 16-byte aligned, with head and tail
# (3, 9, 29, 65, 300 after a head, 1025), one element past the 1024 that four trips of a 64-lane group load (1025), rows
# of many trips (5000).  T: the 64-frame collapse blocks and the rows per workgroup of every variant.  B: 1, 3, 70.
SHAPES = [(1, 1, 1, 0), (1, 65, 3, -1), (2, 2, 3, 1), (3, 63, 70, 0), (9, 64, 3, 8), (29, 65, 70, 0), (29, 200, 3, -1),
          (64, 128, 1, 63), (65, 129, 3, 0), (256, 200, 3, 255), (256, 64, 70, 0), (300, 65, 3, -1), (1025, 129, 3, 0),
          (1025, 2, 1, 1024), (5000, 63, 3, 4999), (5000, 128, 1, 0)]


@pytest.mark.parametrize("C,T,B,blank", SHAPES)
def test_decode_matches_the_yardstick(gtn, C, T, B, blank):
    """planted paths with label runs, blank runs and repeats separated by a blank: all five outputs == the yardstick,
    sentinels intact, the launches took the batch"""
    em, want = _planted(100 + C + T, B, T, C, blank)
    got, stats = _decode(gtn, em, blank=blank)
    assert stats == (B, 0)
    _check(f"C={C} T={T} B={B} blank={blank}", got, want)
    if C > 1 and T >= 63:
        assert (want[4] > 0).all() and (want[4] < T).all()  # (the plant did its work: neither 0 nor T)
    noise = continuous_case(C + T, B, T, C)
    got, _ = _decode(gtn, noise, blank=blank)
    _check(f"noise C={C} T={T} B={B}", got, decode_batch(noise, None, blank))


@pytest.mark.parametrize("kind", ["zero", "01", "int", "late"])
@pytest.mark.parametrize("C", [3, 29, 64, 65, 300, 1025])
def test_exact_ties_go_to_the_smallest_label(gtn, C, kind):
    """integer-valued emissions: the smallest label among equal maxima, between the lanes of a row and between the
    trips of the row loop ('late': the maximum at one label in every 64 and at the last)"""
    B, T = 3, 9
    em = tie_case(700 + C, B, T, C, kind)
    for blank in (0, -1):
        got, stats = _decode(gtn, em, blank=blank)
        assert stats == (B, 0)
        _check(f"ties C={C} {kind} blank={blank}", got, decode_batch(em, None, blank))


def test_runs_across_the_64_frame_blocks(gtn):
    """a repeat straddling a block edge is one token, a blank run straddling one is dropped whole, a label on both
    sides of a blank run that straddles an edge counts twice"""
    T, C, blank = 200, 9, 0
    seq = np.zeros((2, T), np.int64)
    seq[0] = np.arange(T) % 7 + 1           # a new token every frame ...
    seq[0, 60:70] = 5                       # ... a repeat across frame 64
    seq[0, 120:135] = blank                 # ... a blank run across frame 128
    seq[0, 119] = seq[0, 135] = 3           # the same label on both sides of it
    seq[0, 191:194] = 2                     # a repeat across frame 192
    seq[1] = blank                          # all blank but the block edges
    seq[1, 63] = seq[1, 64] = 4
    seq[1, 127] = 4
    seq[1, 128] = 6
    em = np.full((2, T, C), -9.0, np.float32)
    for b in range(2):
        em[b, np.arange(T), seq[b]] = 1.0
    want = decode_batch(em, None, blank)
    assert want[2][1, :3].tolist() == [4, 4, 6] and want[3][1, :3].tolist() == [63, 127, 128] and want[4][1] == 3
    got, _ = _decode(gtn, em, blank=blank)
    _check("block edges", got, want)
    got, _ = _decode(gtn, em, blank=-1)
    _check("block edges, no blank", got, decode_batch(em, None, -1))


RAGGED = (70, 1, 0, 69, 64, 65, 2, 70)  # T, T - 1, 1 and 0 among them


@pytest.mark.parametrize("mode", ["frames", "rows", "both"])
def test_mixed_frame_counts(gtn, mode):
    """per-utterance lengths through `frames`, through Batch.linear(rows=) and through both: == the yardstick at each
    length; NaN in every pad row changes no bit of any output"""
    T, C, blank = 70, 29, 0
    fr = tuple(f for f in RAGGED if f > 0) if mode == "rows" else RAGGED
    B = len(fr)
    em, want = _planted(77, B, T, C, blank, fr)
    rows = None if mode == "frames" else [max(f, 1) for f in fr] if mode == "both" else list(fr)
    frames = None if mode == "rows" else list(fr)
    got, stats = _decode(gtn, em, frames, rows, blank)
    assert stats == (B, 0)
    _check(f"ragged {mode}", got, want)
    raw = _decode.raw
    poisoned = em.copy()
    for b in range(B):
        poisoned[b, fr[b]:] = np.nan
    _decode(gtn, poisoned, frames, rows, blank)
    for name, r0, r1 in zip(NAMES, raw, _decode.raw):
        assert r0.tobytes() == r1.tobytes(), name


def test_full_length_frames_equal_no_frames(gtn):
    B, T, C = 3, 65, 29
    em, want = _planted(78, B, T, C, 0)
    _decode(gtn, em, None, None, 0)
    raw = _decode.raw
    _decode(gtn, em, [T] * B, None, 0)
    for name, r0, r1 in zip(NAMES, raw, _decode.raw):
        assert r0.tobytes() == r1.tobytes(), name


def test_no_path_and_entries_that_are_never_chosen(gtn):
    """an utterance with one all--inf row beside ordinary ones: rows of -1, score -inf, length 0, the neighbours
    untouched; isolated -inf and NaN entries inside valid rows are never chosen"""
    B, T, C, blank = 5, 66, 29, 0
    em = planted_case(79, B, T, C, blank).copy()
    em[1, 40] = -np.inf                      # no path
    em[2, :, 0::3] = -np.inf                 # holes in every row, label 0 (the blank) among them
    em[2, 5, :] = -np.inf
    em[2, 5, 28] = -30.0                     # one entry above -inf, the last of the row
    em[3, :, 1::2] = np.nan                  # NaN in every row
    em[3, 7, 0] = np.nan
    em[4, 65] = np.nan                       # a row of NaN alone: nothing is chosen, no path
    want = decode_batch(em, None, blank)
    assert want[1][1] == -np.inf and want[1][4] == -np.inf and (want[0][1] == -1).all() and (want[0][4] == -1).all()
    assert np.isfinite(want[1][[0, 2, 3]]).all() and want[0][2, 5] == 28
    got, stats = _decode(gtn, em, blank=blank)
    assert stats == (B, 0)
    _check("no path", got, want)
    for name, g in zip(NAMES, got):
        if g.ndim == 2:
            assert (g[1] == -1).all() and (g[4] == -1).all(), name
    assert got[4][1] == 0 and got[4][4] == 0
    holes = holes_case(80, 6, 33, 9, p=0.4)
    got, _ = _decode(gtn, holes, blank=blank)
    _check("holes", got, decode_batch(holes, None, blank))


@pytest.mark.parametrize("address", [False, True])
def test_row_stride_above_T(gtn, address):
    """rows 5 entries wider than T, as tensor views and as raw device addresses with row_stride"""
    B, T, C = 3, 65, 29
    em, want = _planted(81, B, T, C, 0)
    got, stats = _decode(gtn, em, blank=0, pad=5, address=address)
    assert stats == (B, 0)
    _check(f"stride address={address}", got, want)


@pytest.mark.parametrize("scores,collapsed,starts,lengths", [(False, False, False, False), (True, False, False, False),
                                                             (False, True, False, False), (False, True, True, False),
                                                             (True, True, False, True)])
def test_outputs_are_optional(gtn, scores, collapsed, starts, lengths):
    B, T, C = 3, 65, 29
    em, want = _planted(82, B, T, C, 0, (65, 30, 0))
    got, stats = _decode(gtn, em, [65, 30, 0], None, 0, scores, collapsed, starts, lengths)
    assert stats == (B, 0)
    assert [g is not None for g in got] == [True, scores, collapsed, starts, lengths]
    _check("optional", got, want)


def test_bad_arguments_raise_before_anything_is_written(gtn):
    """a count outside 0 .. M or above the rows the batch carries, a stride below M, a blank that is no label:
    ValueError, outputs untouched"""
    B, T, C = 3, 9, 8
    em, _ = _planted(83, B, T, C, 0)
    for kw, msg in ((dict(frames=[9, 10, 1]), "outside 0 .. M"), (dict(frames=[-1, 2, 3]), "outside 0 .. M"),
                    (dict(frames=[9, 5, 1], rows=[9, 4, 9]), "beyond the rows"), (dict(blank=8), "blank"),
                    (dict(address=True, pad=-1), "row_stride is shorter")):
        with pytest.raises(ValueError, match=msg):
            _decode(gtn, em, **kw)
        if kw.get("pad") != -1:  # (those arrays have no guard column to look at)
            for r in _decode.raw:
                assert r is None or (r == SENTINEL).all() or np.isnan(r).all()


@pytest.mark.parametrize("C,T,B", [(29, 65, 3), (300, 129, 2)])
def test_agrees_with_what_ships_today(gtn, C, T, B):
    """labels == those read from viterbi_path(Batch.linear) and scores == viterbi_score's, bit for bit"""
    em, want = _planted(84 + C, B, T, C, 0)
    got, _ = _decode(gtn, em, blank=0)
    ems = gtn.Batch.linear(B, T, C, _dev(em), False, False)
    paths = gtn.viterbi_path(ems)
    for b in range(B):
        assert got[0][b].tolist() == paths[b].labels_to_list(), b
    old = np.asarray(gtn.viterbi_score(ems).items(), np.float32)
    assert got[1].tobytes() == old.tobytes(), (got[1], old)


def test_fallback(gtn):
    """a batch of graphs: the path-graph route -- the same five outputs, counted as fallback; frames are refused"""
    B, T, C, blank = 3, 17, 9, 0
    em = planted_case(85, B, T, C, blank).copy()
    em[1, 4] = -np.inf  # (no path there, on this route too)
    want = decode_batch(em, None, blank)
    graphs = gtn.linear_graph_n(B, T, C, _dev(em), False)
    got, stats = _decode(gtn, em, blank=blank, batch=gtn.Batch(graphs))
    assert stats == (0, B)
    _check("fallback", got, want)
    with pytest.raises(ValueError, match="frame counts need a native linear batch"):
        _decode(gtn, em, frames=[T] * B, blank=blank, batch=gtn.Batch(graphs))
    assert (_decode.raw[0] == SENTINEL).all()


TORCH_CASES = [(21, 4, 40, 12, 0, False), (22, 3, 75, 29, 28, True), (23, 66, 5, 9, 0, True)]  # seed B T C blank ragged


def _torch_frames(seed, B, T):
    fr = np.random.default_rng(seed).integers(0, T + 1, B)
    fr[0] = T
    return tuple(int(f) for f in fr)


def _torch_entry(gtn, em, blank, frames, collapse, side_stream):
    import torch
    from gtn_amd import torch_loss
    x = _dev(em).requires_grad_(True)
    before = x.detach().clone()
    torch.cuda.synchronize()
    kw = dict(blank=blank, input_lengths=None if frames is None else list(frames), collapse=collapse)
    try:
        if side_stream:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                out = torch_loss.ctc_decode(x, **kw)
            torch.cuda.current_stream().wait_stream(s)
        else:
            out = torch_loss.ctc_decode(x, **kw)
        torch.cuda.synchronize()
    finally:
        gtn.set_stream(None)
    B, T, _ = em.shape
    assert len(out) == (5 if collapse else 2)
    kinds = ((torch.int32, (B, T)), (torch.float32, (B,)), (torch.int32, (B, T)), (torch.int32, (B, T)),
             (torch.int32, (B,)))
    for o, (dt, shape) in zip(out, kinds):
        assert o.dtype == dt and o.shape == shape and o.device == x.device and not o.requires_grad
    assert torch.equal(x.detach(), before)
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("side_stream", [True, False])
@pytest.mark.parametrize("seed,B,T,C,blank,ragged", TORCH_CASES)
def test_torch_entry(gtn, seed, B, T, C, blank, ragged, side_stream):
    """torch_loss.ctc_decode (native route) on a non-default stream and on the default one, with and without
    input_lengths and collapse: dtypes, device, shapes; results == the yardstick; log_probs untouched, nothing requires
    grad; counted as the launches"""
    frames = _torch_frames(seed, B, T) if ragged else None
    em, want = _planted(seed, B, T, C, blank, frames)
    f0, b0 = gtn.debug_linear_decode_stats()
    out = _torch_entry(gtn, em, blank, frames, ragged, side_stream)
    f1, b1 = gtn.debug_linear_decode_stats()
    assert (f1 - f0, b1 - b0) == (B, 0)
    _check(f"torch seed={seed}", out, want)


_CHILD = "--python-criteria-child"


def test_torch_entry_python_route(tmp_path):
    """GTN_AMD_PYTHON_CRITERIA=1 in a fresh process: Batch.linear(borrow).linear_decode"""
    out = str(tmp_path / "child.npz")
    env = dict(os.environ, GTN_AMD_PYTHON_CRITERIA="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), _CHILD, out], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    z = np.load(out)
    i = 0
    for seed, B, T, C, blank, ragged in TORCH_CASES:
        frames = _torch_frames(seed, B, T) if ragged else None
        want = _planted(seed, B, T, C, blank, frames)[1]
        for side_stream in (True, False):
            _check(f"python route {i}", [z[f"o{i}_{k}"] for k in range(5 if ragged else 2)], want)
            i += 1
    assert int(z["fast"]) == sum(2 * c[1] for c in TORCH_CASES) and int(z["fallback"]) == 0


def _python_route_child(out):
    sys.path.insert(0, ROOT)
    import gtn_amd as gtn
    from gtn_amd import torch_loss
    assert not torch_loss._native()
    res, i = {}, 0
    for seed, B, T, C, blank, ragged in TORCH_CASES:
        frames = _torch_frames(seed, B, T) if ragged else None
        em = planted_case(seed, B, T, C, blank)
        for side_stream in (True, False):
            for k, o in enumerate(_torch_entry(gtn, em, blank, frames, ragged, side_stream)):
                res[f"o{i}_{k}"] = o
            i += 1
    res["fast"], res["fallback"] = gtn.debug_linear_decode_stats()
    np.savez(out, **res)


def test_criteria_abi(gtn):
    """gtn_ctc_decode_n gives the five tensors the Batch API gives"""
    import torch
    seed, B, T, C, blank, _ = TORCH_CASES[1]
    frames = _torch_frames(seed, B, T)
    em, want = _planted(seed, B, T, C, blank, frames)
    em_dev = _dev(em)
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    lib.gtn_ctc_decode_n.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 6
    lib.gtn_ctc_decode_n.restype = ctypes.c_int
    lib.gtn_criteria_last_error.restype = ctypes.c_char_p
    fr = np.ascontiguousarray(frames, dtype=np.int32)
    lab, tok, sta = (torch.full((B, T), SENTINEL, dtype=torch.int32, device="cuda:0") for _ in range(3))
    sc = torch.full((B,), float("nan"), dtype=torch.float32, device="cuda:0")
    le = torch.full((B,), SENTINEL, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    rc = lib.gtn_ctc_decode_n(em_dev.data_ptr(), B, T, C, blank, fr.ctypes.data, lab.data_ptr(), sc.data_ptr(),
                              tok.data_ptr(), sta.data_ptr(), le.data_ptr())
    assert rc == 0, lib.gtn_criteria_last_error().decode()
    gtn.synchronize()
    _check("abi", [t.cpu().numpy() for t in (lab, sc, tok, sta, le)], want)


def test_round_trip_through_forced_alignment(gtn):
    """ctc_forced_align(log_probs, decoded tokens) reproduces the decoded frame labels on a case without ties: the
    best path over all label sequences is the best path of its own collapsed sequence"""
    from gtn_amd import torch_loss
    B, T, C, blank = 4, 65, 32, 0  # (an alphabet the alignment launch takes: a multiple of 4)
    em, want = _planted(86, B, T, C, blank)
    x = _dev(em)
    try:
        labels, scores, tokens, starts, lengths = torch_loss.ctc_decode(x, blank=blank)
        targets = [tokens[b, :int(lengths[b])].cpu().tolist() for b in range(B)]
        assert all(len(t) > 0 for t in targets)
        al, _, asc = torch_loss.ctc_forced_align(x, targets, blank=blank)
        import torch
        torch.cuda.synchronize()
    finally:
        gtn.set_stream(None)
    assert (labels.cpu().numpy() == want[0]).all()
    assert (al.cpu().numpy() == want[0]).all()
    assert np.allclose(asc.cpu().numpy(), want[1], rtol=1e-5, atol=0)


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == _CHILD:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _python_route_child(sys.argv[2])
