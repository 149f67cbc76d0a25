"""Batched ASG Viterbi decode with device-resident output (asg_decode.hip through gtnx_batch_viterbi_decode;
gtn_amd.Batch.viterbi_decode, gtn_amd.torch_loss.asg_decode, gtn_asg_decode_n).

The judge of labels and collapsed sequences is the float64 full-connect Viterbi of tests/asg_decode_fp.py, which
tests/test_asg_decode_cpu.py pins to the oracle's shortest path on the lattice the reference would build, exact ties
included (smallest source label, smallest final label).  Every continuous seed is vetted on the host first: the same
recursion in the device's float32 association has to pick the float64 path, else the seed is to be replaced.  Scores
are held to 1e-5 relative to max(1, |score|): T <= 129 float32 additions along the path, each within 2^-24 relative of
a running sum below ~1e3, stay far inside that bound.
"""
import contextlib
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from asg_decode_fp import asg_decode_fp64, float32_agrees, seeded_case, tie_case

pytestmark = pytest.mark.gpu
SENTINEL = -7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _transitions(gtn, trans, start, sort=True):
    """gtn::criteria::asgTransitions with weights: arc i = start -> label i, arc N + i N + j = j -> i"""
    N = len(start)
    g = gtn.Graph(False)
    g.add_nodes(np.array([1] + [0] * N, np.uint8), np.array([0] + [1] * N, np.uint8))
    n = np.arange(N)
    src = np.concatenate([np.zeros(N, np.int32), np.tile(n + 1, N).astype(np.int32)])
    dst = np.concatenate([n + 1, np.repeat(n + 1, N)]).astype(np.int32)
    lab = np.concatenate([n, np.repeat(n, N)]).astype(np.int32)
    w = np.concatenate([np.asarray(start, np.float32), np.asarray(trans, np.float32).reshape(-1)])
    g.add_arcs(src, dst, lab, lab, w)
    if sort:
        g.arc_sort()
    return g


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _decode(gtn, em_dev, tg, frames=None, rows=None, collapse=True, want_scores=True):
    """Batch.viterbi_decode on Batch.linear; outputs allocated with a guard row and column of sentinels that must
    survive.  Returns (labels [B, T], scores [B], collapsed [B, T] or None, lengths [B] or None, (fast, fallback)
    counts of this call)"""
    import torch
    B, T, N = em_dev.shape
    ems = gtn.Batch.linear(B, T, N, em_dev, False, True, rows)
    lab = torch.full((B + 1, T + 1), SENTINEL, dtype=torch.int32, device="cuda:0")
    col = torch.full((B + 1, T + 1), SENTINEL, dtype=torch.int32, device="cuda:0") if collapse else None
    ln = torch.full((B + 1,), SENTINEL, dtype=torch.int32, device="cuda:0") if collapse else None
    sc = torch.full((B + 1,), float("nan"), dtype=torch.float32, device="cuda:0") if want_scores else None
    f0, b0 = gtn.debug_decode_stats()
    try:
        ems.viterbi_decode(tg, lab[:B, :T], sc, frames, col[:B, :T] if collapse else None, ln)
    finally:
        gtn.synchronize()
        f1, b1 = gtn.debug_decode_stats()
        labn = lab.cpu().numpy()
        assert (labn[B] == SENTINEL).all() and (labn[:, T] == SENTINEL).all()
        if want_scores:
            scn = sc.cpu().numpy()
            assert np.isnan(scn[B])
        if collapse:
            coln, lnn = col.cpu().numpy(), ln.cpu().numpy()
            assert (coln[B] == SENTINEL).all() and (coln[:, T] == SENTINEL).all() and lnn[B] == SENTINEL
        _decode.last_raw = (labn, coln if collapse else None)  # (guards included; kept when the call raised, too)
    return (labn[:B, :T], scn[:B] if want_scores else None, coln[:B, :T] if collapse else None,
            lnn[:B] if collapse else None, (f1 - f0, b1 - b0))


def _score_ok(got, want):
    if not np.isfinite(want):
        return got == want
    return abs(float(got) - want) <= 1e-5 * max(1.0, abs(want))


def _check_row(tag, T, labels, score, collapsed, length, want, exact_score=False):
    wl, ws, wc = want
    print(f"[asg_decode] {tag} score {score!r} fp64 {ws!r}")
    assert labels.tolist() == wl.tolist(), tag
    if score is not None:
        assert (score == ws) if exact_score else _score_ok(score, ws), (tag, score, ws)
    if collapsed is not None:
        assert int(length) == len(wc), tag
        assert collapsed.tolist() == wc + [-1] * (T - len(wc)), tag


@functools.lru_cache(maxsize=None)
def _vetted(seed, B, T, N, frames=None):
    """a continuous case whose every utterance float32 and float64 decode alike (checked here, before the device sees
    it), with its float64 results: (em, trans, start, [(labels, score, collapsed)])"""
    em, trans, start = seeded_case(seed, T, N, B)
    want = []
    for b in range(B):
        f = T if frames is None else frames[b]
        assert float32_agrees(em[b], trans, start, f), f"replace seed {seed}: utterance {b} separates float32 from float64"
        want.append(asg_decode_fp64(em[b], trans, start, f))
    return em, trans, start, want


@contextlib.contextmanager
def _lazy():
    with _env(GTNX_LAZY_COMPOSE="1"):
        yield


def _ships_today(gtn, em, tg):
    """the route before this call existed: viterbi_path / viterbi_score over compose(ems, [transitions]), the labels read
    from the path graphs"""
    B, T, N = em.shape
    with _lazy():
        ems = gtn.linear_graph_n(B, T, N, _dev(em), False)
        paths = gtn.viterbi_path(gtn.compose(ems, [tg]))
        scores = gtn.items(gtn.viterbi_score(gtn.compose(ems, [tg])))
    return [p.labels_to_list() for p in paths], np.asarray(scores, np.float32)


# N: the dense minimum (7, 8), the trace's 64-lane slices (63, 64, 65), 300, C4's 513 nodes, the top of the regime;
# T: the trace's two-step look-ahead (1, 2, 3), the 64-entry store period (63, 64, 65, 128, 129);
# B: the sweep's 64-utterance slabs (1, 64, 65)
SHAPES = [(7, 1, 1), (7, 2, 64), (7, 3, 65), (8, 63, 1), (8, 64, 65), (63, 65, 3), (64, 128, 2), (65, 129, 64),
          (300, 65, 3), (300, 2, 1), (512, 129, 2), (512, 3, 65), (1023, 64, 2), (1023, 129, 1), (1023, 1, 1)]


@pytest.mark.parametrize("N,T,B", SHAPES)
def test_decode_matches_fp64_and_what_ships_today(gtn, N, T, B):
    """full length: labels and collapsed sequences == the yardstick, scores within the bound, sentinels intact, the
    one-launch route took the batch; labels == those read from viterbi_path(compose(ems, [transitions])) and scores ==
    viterbi_score's, bit for bit"""
    em, trans, start, want = _vetted(1000 + N + T, B, T, N)
    tg = _transitions(gtn, trans, start)
    labels, scores, col, ln, stats = _decode(gtn, _dev(em), tg)
    assert stats == (B, 0)
    for b in range(B):
        _check_row(f"N={N} T={T} b={b}", T, labels[b], scores[b], col[b], ln[b], want[b])
    old_labels, old_scores = _ships_today(gtn, em, tg)
    for b in range(B):
        assert labels[b].tolist() == old_labels[b], b
    assert scores.tobytes() == old_scores.tobytes()


@pytest.mark.parametrize("sort", [True, False])
@pytest.mark.parametrize("C,kind", [(17, "zero"), (17, "01"), (17, "int"), (40, "zero"), (40, "01"), (40, "int")])
def test_integer_ties(gtn, C, kind, sort):
    """exact ties everywhere, at alphabets whose in-lists std::sort scrambles: labels and scores == the yardstick
    (smallest source label, smallest final label), transitions arc-sorted and as built"""
    B, T = 5, 14
    em, trans, start = tie_case(300 + C, T, C, kind, B)
    tg = _transitions(gtn, trans, start, sort)
    labels, scores, col, ln, stats = _decode(gtn, _dev(em), tg)
    assert stats == (B, 0)
    for b in range(B):
        _check_row(f"C={C} {kind} b={b}", T, labels[b], scores[b], col[b], ln[b],
                   asg_decode_fp64(em[b], trans, start), exact_score=True)


RAGGED = (70, 1, 0, 33, 64, 65, 2, 70)  # T, 1 and 0 among them


@pytest.mark.parametrize("mode", ["frames", "rows", "both"])
def test_mixed_frame_counts(gtn, mode):
    """per-utterance lengths through `frames`, through Batch.linear(rows=) and through both: results == the yardstick at
    each length and == per-utterance decodes of em[b, :T_b] by what ships today; NaN in every pad row changes no bit of
    any output"""
    T, N = 70, 12
    fr = tuple(f for f in RAGGED if f > 0) if mode == "rows" else RAGGED
    B = len(fr)
    em, trans, start, want = _vetted(77, B, T, N, fr)
    tg = _transitions(gtn, trans, start)
    rows = None if mode == "frames" else [max(f, 1) for f in fr] if mode == "both" else list(fr)
    frames = None if mode == "rows" else list(fr)
    labels, scores, col, ln, stats = _decode(gtn, _dev(em), tg, frames, rows)
    assert stats == (B, 0)
    raw = _decode.last_raw
    for b in range(B):
        _check_row(f"{mode} b={b} T_b={fr[b]}", T, labels[b], scores[b], col[b], ln[b], want[b])
        if fr[b] >= 1:
            old_labels, old_scores = _ships_today(gtn, em[b:b + 1, :fr[b]], tg)
            assert labels[b, :fr[b]].tolist() == old_labels[0]
            assert scores[b:b + 1].tobytes() == old_scores.tobytes()
    poisoned = em.copy()
    for b in range(B):
        poisoned[b, fr[b]:] = np.nan
    l2, s2, c2, n2, stats = _decode(gtn, _dev(poisoned), tg, frames, rows)
    assert stats == (B, 0)
    assert raw[0].tobytes() == _decode.last_raw[0].tobytes() and raw[1].tobytes() == _decode.last_raw[1].tobytes()
    assert scores.tobytes() == s2.tobytes() and ln.tobytes() == n2.tobytes()


def test_outputs_are_optional(gtn):
    em, trans, start, want = _vetted(78, 3, 9, 8)
    tg = _transitions(gtn, trans, start)
    labels, scores, col, ln, stats = _decode(gtn, _dev(em), tg, collapse=False, want_scores=False)
    assert stats == (3, 0) and scores is None and col is None
    for b in range(3):
        _check_row(f"labels only b={b}", 9, labels[b], None, None, None, want[b])


def test_bad_frame_counts_raise_before_anything_is_written(gtn):
    """a count outside 0 .. M, or above the rows the batch carries: ValueError, outputs untouched"""
    em, trans, start, _ = _vetted(78, 3, 9, 8)
    tg = _transitions(gtn, trans, start)
    for frames, rows, msg in (([9, 10, 1], None, "outside 0 .. M"), ([-1, 2, 3], None, "outside 0 .. M"),
                              ([9, 5, 1], [9, 4, 9], "beyond the rows")):
        with pytest.raises(ValueError, match=msg):
            _decode(gtn, _dev(em), tg, frames, rows)
        assert (_decode.last_raw[0] == SENTINEL).all() and (_decode.last_raw[1] == SENTINEL).all()


@pytest.mark.parametrize("N,T,B,env", [(4, 9, 3, {}), (1025, 2, 2, {}), (12, 9, 3, {"GTNX_NO_DENSE": "1"})])
def test_fallback(gtn, N, T, B, env):
    """fewer than 7 or more than 1023 labels, or the dense regime switched off: the path-graph route -- same labels,
    collapsed sequences and scores, counted as fallback; frame counts are refused there"""
    em, trans, start, want = _vetted(500 + N, B, T, N)
    tg = _transitions(gtn, trans, start)
    with _env(**env):
        labels, scores, col, ln, stats = _decode(gtn, _dev(em), tg)
        assert stats == (0, B)
        for b in range(B):
            _check_row(f"fallback N={N} b={b}", T, labels[b], scores[b], col[b], ln[b], want[b])
        with pytest.raises(ValueError, match="frame counts need"):
            _decode(gtn, _dev(em), tg, [T] * B)
        assert (_decode.last_raw[0] == SENTINEL).all()


TORCH_CASES = [(21, 4, 40, 12, False), (22, 3, 75, 32, True), (23, 66, 5, 9, True)]  # seed, B, T, N, ragged


def _torch_frames(seed, B, T):
    fr = np.random.default_rng(seed).integers(0, T + 1, B)
    fr[0] = T
    return tuple(int(f) for f in fr)


def _torch_entry(gtn, em, trans, start, frames, collapse, side_stream):
    import torch
    from gtn_amd import torch_loss
    x = _dev(em).requires_grad_(True)
    tr, st = _dev(trans).requires_grad_(True), _dev(start)
    before = x.detach().clone()
    torch.cuda.synchronize()
    kw = dict(start=st, input_lengths=None if frames is None else list(frames), collapse=collapse)
    try:
        if side_stream:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                out = torch_loss.asg_decode(x, tr, **kw)
            torch.cuda.current_stream().wait_stream(s)
        else:
            out = torch_loss.asg_decode(x, tr, **kw)
        torch.cuda.synchronize()
    finally:
        gtn.set_stream(None)
    B, T, _ = em.shape
    assert len(out) == (4 if collapse else 2)
    for o, dt, shape in zip(out, (torch.int32, torch.float32, torch.int32, torch.int32), ((B, T), (B,), (B, T), (B,))):
        assert o.dtype == dt and o.shape == shape and o.device == x.device and not o.requires_grad
    assert torch.equal(x.detach(), before)
    return [o.cpu().numpy() for o in out]


def _check_torch(out, T, want):
    for b in range(len(want)):
        col, ln = (out[2][b], out[3][b]) if len(out) == 4 else (None, None)
        _check_row(f"torch b={b}", T, out[0][b], out[1][b], col, ln, want[b])


@pytest.mark.parametrize("side_stream", [True, False])
@pytest.mark.parametrize("seed,B,T,N,ragged", TORCH_CASES)
def test_torch_entry(gtn, seed, B, T, N, ragged, side_stream):
    """torch_loss.asg_decode (native route) on a non-default stream and on the default one, with and without
    input_lengths and collapse: dtypes, device, shapes; results equal the yardstick; emissions untouched, nothing
    requires grad; counted as the launch"""
    frames = _torch_frames(seed, B, T) if ragged else None
    em, trans, start, want = _vetted(seed, B, T, N, frames)
    f0, b0 = gtn.debug_decode_stats()
    out = _torch_entry(gtn, em, trans, start, frames, ragged, side_stream)
    f1, b1 = gtn.debug_decode_stats()
    assert (f1 - f0, b1 - b0) == (B, 0)
    _check_torch(out, T, want)


_CHILD = "--python-criteria-child"


def test_torch_entry_python_route(tmp_path):
    """GTN_AMD_PYTHON_CRITERIA=1 in a fresh process: Batch.linear(borrow).viterbi_decode"""
    out = str(tmp_path / "child.npz")
    env = dict(os.environ, GTN_AMD_PYTHON_CRITERIA="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), _CHILD, out], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    z = np.load(out)
    i = 0
    for seed, B, T, N, ragged in TORCH_CASES:
        frames = _torch_frames(seed, B, T) if ragged else None
        want = _vetted(seed, B, T, N, frames)[3]
        for side_stream in (True, False):
            _check_torch([z[f"o{i}_{k}"] for k in range(4 if ragged else 2)], T, want)
            i += 1
    assert int(z["fast"]) == sum(2 * c[1] for c in TORCH_CASES) and int(z["fallback"]) == 0


def _python_route_child(out):
    sys.path.insert(0, ROOT)
    import gtn_amd as gtn
    from gtn_amd import torch_loss
    assert not torch_loss._native()
    res, i = {}, 0
    for seed, B, T, N, ragged in TORCH_CASES:
        frames = _torch_frames(seed, B, T) if ragged else None
        em, trans, start = seeded_case(seed, T, N, B)
        for side_stream in (True, False):
            for k, o in enumerate(_torch_entry(gtn, em, trans, start, frames, ragged, side_stream)):
                res[f"o{i}_{k}"] = o
            i += 1
    res["fast"], res["fallback"] = gtn.debug_decode_stats()
    np.savez(out, **res)


def test_criteria_abi(gtn):
    """gtn_asg_decode_n gives the four tensors the Batch API gives"""
    import torch
    seed, B, T, N, _ = TORCH_CASES[1]
    frames = _torch_frames(seed, B, T)
    em, trans, start, want = _vetted(seed, B, T, N, frames)
    em_dev = _dev(em)
    labels, scores, col, ln, _ = _decode(gtn, em_dev, _transitions(gtn, trans, start), list(frames))
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    lib.gtn_asg_decode_n.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 6
    lib.gtn_asg_decode_n.restype = ctypes.c_int
    lib.gtn_criteria_last_error.restype = ctypes.c_char_p
    w = _dev(np.concatenate([start, trans.reshape(-1)]).astype(np.float32))
    fr = np.ascontiguousarray(frames, dtype=np.int32)
    lab = torch.full((B, T), SENTINEL, dtype=torch.int32, device="cuda:0")
    cl = torch.full((B, T), SENTINEL, dtype=torch.int32, device="cuda:0")
    sc = torch.full((B,), float("nan"), dtype=torch.float32, device="cuda:0")
    le = torch.full((B,), SENTINEL, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    rc = lib.gtn_asg_decode_n(em_dev.data_ptr(), B, T, N, w.data_ptr(), fr.ctypes.data, lab.data_ptr(), sc.data_ptr(),
                              cl.data_ptr(), le.data_ptr())
    assert rc == 0, lib.gtn_criteria_last_error().decode()
    gtn.synchronize()
    assert (lab.cpu().numpy() == labels).all() and (cl.cpu().numpy() == col).all() and (le.cpu().numpy() == ln).all()
    assert sc.cpu().numpy().tobytes() == scores.tobytes()
    for b in range(B):
        _check_row(f"abi b={b}", T, labels[b], scores[b], col[b], ln[b], want[b])


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == _CHILD:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _python_route_child(sys.argv[2])
