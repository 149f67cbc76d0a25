"""Batched ASG forced alignment with device-resident output (asg_align.hip through gtnx_batch_viterbi_align;
gtn_amd.Batch.viterbi_align on Batch.asg_force_align x Batch.linear, gtn_amd.torch_loss.asg_forced_align,
gtn_asg_align_n).

The judge of labels and tokens is the float64 trellis Viterbi of tests/asg_align_fp.py, which
tests/test_asg_align_cpu.py pins to the oracle's shortest path on the lattice the reference would build, exact ties
included (the step wins).  Scores are held to 1e-5 relative to max(1, |score|): the kernel sums T float32 terms of
magnitude <= ~10 in path order, each addition within 2^-24 relative of the running sum, which stays far inside that
bound at T <= 600.
"""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from asg_align_fp import FP_CASES, TIE_CASES, asg_align_fp64, seeded_case, tie_case

pytestmark = pytest.mark.gpu
SENTINEL = -7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _transitions(gtn, trans, start):
    """gtn::criteria::asgTransitions with weights: arc i = start -> label i, arc N + i N + j = j -> i; arc-sorted"""
    N = len(start)
    g = gtn.Graph(False)
    g.add_nodes(np.array([1] + [0] * N, np.uint8), np.array([0] + [1] * N, np.uint8))
    n = np.arange(N)
    src = np.concatenate([np.zeros(N, np.int32), np.tile(n + 1, N).astype(np.int32)])
    dst = np.concatenate([n + 1, np.repeat(n + 1, N)]).astype(np.int32)
    lab = np.concatenate([n, np.repeat(n, N)]).astype(np.int32)
    w = np.concatenate([np.asarray(start, np.float32), np.asarray(trans, np.float32).reshape(-1)])
    g.add_arcs(src, dst, lab, lab, w)
    g.arc_sort()
    return g


_TRANS = {}  # id(trans) -> (trans, start, graph): the 4.2 M arcs of a 2048-label transitions graph are built once


def _cached_transitions(gtn, trans, start):
    hit = _TRANS.get(id(trans))
    if hit is None or hit[0] is not trans or hit[1] is not start:
        hit = _TRANS[id(trans)] = (trans, start, _transitions(gtn, trans, start))
    return hit[2]


def _product(gtn, em_dev, trans, start, targets, chain_first, rows=None):
    B, T, N = em_dev.shape
    fals = gtn.Batch.asg_force_align([list(t) for t in targets], _cached_transitions(gtn, trans, start), N)
    ems = gtn.Batch.linear(B, T, N, em_dev, False, True, rows)
    return gtn.compose(ems, fals) if chain_first else gtn.compose(fals, ems)


def _align(gtn, em_dev, trans, start, targets, chain_first=False, frames=None, want_tokens=True, rows=None):
    """Batch.viterbi_align on asg_force_align x linear; outputs allocated with a guard row and column that must
    survive.  Returns (labels [B, T], tokens [B, T] or None, scores [B], (fast, fallback) counts of this call)"""
    import torch
    B, T, N = em_dev.shape
    comp = _product(gtn, em_dev, trans, start, targets, chain_first, rows)
    lab = torch.full((B + 1, T + 1), SENTINEL, dtype=torch.int32, device="cuda:0")
    tok = torch.full((B + 1, T + 1), SENTINEL, dtype=torch.int32, device="cuda:0") if want_tokens else None
    sc = torch.full((B + 1,), float("nan"), dtype=torch.float32, device="cuda:0")
    f0, b0 = gtn.debug_align_stats()
    comp.viterbi_align(lab[:B, :T], tok[:B, :T] if want_tokens else None, sc, frames)
    gtn.synchronize()
    f1, b1 = gtn.debug_align_stats()
    labn, scn = lab.cpu().numpy(), sc.cpu().numpy()
    assert (labn[B] == SENTINEL).all() and (labn[:, T] == SENTINEL).all() and np.isnan(scn[B])
    tokn = None
    if want_tokens:
        tokn = tok.cpu().numpy()
        assert (tokn[B] == SENTINEL).all() and (tokn[:, T] == SENTINEL).all()
        tokn = tokn[:B, :T]
    return labn[:B, :T], tokn, scn[:B], (f1 - f0, b1 - b0)


def _score_ok(got, want):
    if not np.isfinite(want):
        return got == want
    return abs(float(got) - want) <= 1e-5 * max(1.0, abs(want))


def _check_tokens(labels, tokens, target):
    """tokens run from 0 to U - 1 in steps of 0 / 1 and labels == target[tokens]"""
    target = np.asarray(target, np.int64)
    assert tokens[0] == 0 and tokens[-1] == len(target) - 1
    steps = np.diff(tokens)
    assert ((steps == 0) | (steps == 1)).all()
    assert (labels == target[tokens]).all()


def _check_row(tag, labels, tokens, score, want, f, target):
    wl, wt, ws = want
    print(f"[asg_align] {tag} score {score!r} fp64 {ws!r}")
    assert labels.tolist() == wl.tolist(), tag
    assert tokens.tolist() == wt.tolist(), tag
    assert _score_ok(score, ws), (tag, score, ws)
    if np.isfinite(ws) and f > 0:
        _check_tokens(labels[:f], tokens[:f], target)


# (nodes of the widest target, labels, Ts): every nodes-per-lane instantiation and its edges (64 | 65, 128 | 129,
# 256 | 257, 512); T = U (steps only), U + 1, and around the back-pointer word period (32 / NPL steps), the store
# period (64) and the chase's batch (8 or 16 word rows); C = 8 fills a staged block with 256 rows, C = 300 with 6 (block
# not full), C = 2048 with one
SHAPES = [
    (2, 8, [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257]),
    (64, 300, [63, 64, 65, 127, 128, 129, 257]),
    (65, 8, [64, 65, 66, 127, 128, 129, 255, 256, 257]),
    (128, 2048, [127, 128, 257]),
    (129, 8, [128, 129, 130, 255, 256, 257]),
    (257, 300, [256, 257, 258, 300]),
    (257, 2048, [256]),
    (512, 8, [511, 512, 513, 575, 576, 577]),
]


@functools.lru_cache(maxsize=None)
def _shape_case(nodes, N, T):
    """seeded inputs of one (shape, T) and their yardstick, computed once and shared by both argument orders: the
    widest target, the widest target of ONE repeated label, a random shorter one, a single label"""
    rng = np.random.default_rng(1000 * nodes + 7 * N + T)
    U = nodes - 1
    em = rng.normal(0, 2, (4, T, N)).astype(np.float32)
    trans = rng.normal(0, 1, (N, N)).astype(np.float32)
    start = rng.normal(0, 1, N).astype(np.float32)
    targets = [rng.integers(0, N, U).tolist(), [int(rng.integers(0, N))] * U,
               rng.integers(0, N, int(rng.integers(1, U + 1))).tolist(), [int(rng.integers(0, N))]]
    want = [asg_align_fp64(em[b], trans, start, targets[b]) for b in range(4)]
    for w in want:
        for a in w[:2]:
            a.setflags(write=False)
    return em, trans, start, targets, want


@pytest.mark.parametrize("chain_first", [False, True])
@pytest.mark.parametrize("nodes,N,Ts", SHAPES)
def test_shapes_vs_fp64(gtn, nodes, N, Ts, chain_first):
    for T in Ts:
        em, trans, start, targets, want = _shape_case(nodes, N, T)
        B = len(targets)
        assert all(len(t) <= T for t in targets)
        labels, tokens, scores, counts = _align(gtn, _dev(em), trans, start, targets, chain_first)
        assert counts == (B, 0)
        for b in range(B):
            _check_row(f"nodes={nodes} C={N} T={T} b={b}", labels[b], tokens[b], scores[b], want[b], T, targets[b])


@pytest.mark.parametrize("nodes,N,T", [(64, 8, 100), (129, 300, 200), (300, 256, 310), (512, 12, 520)])
def test_agrees_with_the_path_graph_route(gtn, nodes, N, T):
    """continuous inputs: labels equal viterbi_path(product)[b].labels_to_list(), scores equal viterbi_score(product)
    bit for bit (both routes add alpha + (w + e) along the same path)"""
    em, trans, start, targets, _ = _shape_case(nodes, N, T)
    B = len(targets)
    em_dev = _dev(em)
    labels, _, scores, counts = _align(gtn, em_dev, trans, start, targets)
    assert counts == (B, 0)
    prod = _product(gtn, em_dev, trans, start, targets, False)
    paths = gtn.viterbi_path(prod)
    vs = np.asarray(gtn.viterbi_score(_product(gtn, em_dev, trans, start, targets, False)).items(), np.float32)
    for b in range(B):
        assert labels[b].tolist() == paths[b].labels_to_list(), b
        print(f"[asg_align] route nodes={nodes} b={b} score {scores[b]!r} viterbi_score {vs[b]!r}")
        assert scores[b] == vs[b]


@pytest.mark.parametrize("chain_first", [False, True])
@pytest.mark.parametrize("seed,B,Tmax,Umax,nlab,rep,kind", TIE_CASES)
def test_exact_ties_on_the_device(gtn, seed, B, Tmax, Umax, nlab, rep, kind, chain_first):
    """the integer cases of tests/test_asg_align_cpu.py (pinned to the oracle there), padded to an alphabet of 8
    columns and one batch per case with per-utterance frame counts: labels and tokens == the yardstick, scores =="""
    utts, trans, start = tie_case(seed, B, Tmax, Umax, nlab, rep, kind, N=8)
    T = max(e.shape[0] for e, _ in utts)
    em = np.zeros((B, T, 8), np.float32)
    frames = np.zeros(B, np.int32)
    for b, (e, _) in enumerate(utts):
        em[b, :e.shape[0]] = e
        frames[b] = e.shape[0]
    targets = [t for _, t in utts]
    labels, tokens, scores, counts = _align(gtn, _dev(em), trans, start, targets, chain_first, frames)
    assert counts == (B, 0)
    for b in range(B):
        wl, wt, ws = asg_align_fp64(em[b], trans, start, targets[b], frames[b])
        assert labels[b].tolist() == wl.tolist(), (seed, b, targets[b])
        assert tokens[b].tolist() == wt.tolist(), (seed, b, targets[b])
        assert scores[b] == np.float32(ws)
        _check_tokens(labels[b, :frames[b]], tokens[b, :frames[b]], targets[b])


def test_frames_and_padding(gtn):
    """mixed frame counts in one batch, among them frames = U (steps only), U - 1 (no path: -inf, rows of -1) and 0;
    entries past frames[b] are -1; NaN in every emission row past frames[b] changes no bit; Batch.linear(rows=)
    without frames gives the same; frames[b] > rows[b] is refused"""
    B, T, N = 7, 90, 16
    rng = np.random.default_rng(77)
    em = rng.normal(0, 2, (B, T, N)).astype(np.float32)
    trans = rng.normal(0, 1, (N, N)).astype(np.float32)
    start = rng.normal(0, 1, N).astype(np.float32)
    targets = [rng.integers(0, N, u).tolist() for u in (30, 12, 25, 1, 64, 9, 70)]
    frames = np.array([T, 12, 24, 0, 65, 40, 70], np.int32)  # b=1, 6: steps only; b=2: one frame short; b=3: none
    want = [asg_align_fp64(em[b], trans, start, targets[b], frames[b]) for b in range(B)]
    assert [np.isfinite(w[2]) for w in want] == [True, True, False, False, True, True, True]
    labels, tokens, scores, counts = _align(gtn, _dev(em), trans, start, targets, False, frames)
    assert counts == (B, 0)
    for b in range(B):
        f = int(frames[b])
        assert (labels[b, f:] == -1).all() and (tokens[b, f:] == -1).all()
        _check_row(f"frames b={b}", labels[b], tokens[b], scores[b], want[b], f, targets[b])
    assert scores[2] == -np.inf and (labels[2] == -1).all() and (tokens[2] == -1).all()
    assert scores[3] == -np.inf and (labels[3] == -1).all()
    # NaN in every row that does not count
    em_nan = em.copy()
    for b in range(B):
        em_nan[b, frames[b]:] = np.nan
    l2, t2, s2, _ = _align(gtn, _dev(em_nan), trans, start, targets, True, frames)
    assert (l2 == labels).all() and (t2 == tokens).all() and s2.tobytes() == scores.tobytes()
    # the chain's own row counts (1 .. T) are the default frame counts
    rows = np.maximum(frames, 1)
    em_rows = em.copy()
    for b in range(B):
        em_rows[b, rows[b]:] = np.nan
    l3, t3, s3, counts = _align(gtn, _dev(em_rows), trans, start, targets, False, None, rows=rows)
    assert counts == (B, 0)
    for b in range(B):
        if frames[b] >= 1:
            assert (l3[b] == labels[b]).all() and (t3[b] == tokens[b]).all() and s3[b].tobytes() == scores[b].tobytes()
    # (b = 3: one row and a target of one label -- a path of one frame)
    _check_row("rows b=3", l3[3], t3[3], s3[3], asg_align_fp64(em[3], trans, start, targets[3], 1), 1, targets[3])
    with pytest.raises(ValueError, match="frame"):
        over = rows.copy()
        over[1] += 1
        _align(gtn, _dev(em), trans, start, targets, False, over, rows=rows)
    with pytest.raises(ValueError, match="frame"):
        _align(gtn, _dev(em), trans, start, targets, False, np.full(B, T + 1, np.int32))


@pytest.mark.parametrize("nodes,N,T,B", [(513, 8, 520, 1), (6, 9, 20, 3)])
def test_shapes_outside_the_launch_take_the_path_graphs(gtn, nodes, N, T, B):
    """a 513-node target, an alphabet that is no multiple of 4: labels and scores through the path graphs (equal to
    viterbi_path), counted as such; token indices and frame counts are errors there, not garbage"""
    rng = np.random.default_rng(nodes + N)
    em = rng.normal(0, 2, (B, T, N)).astype(np.float32)
    trans = rng.normal(0, 1, (N, N)).astype(np.float32)
    start = rng.normal(0, 1, N).astype(np.float32)
    targets = [rng.integers(0, N, nodes - 1).tolist() for _ in range(B)]
    em_dev = _dev(em)
    labels, _, scores, counts = _align(gtn, em_dev, trans, start, targets, want_tokens=False)
    assert counts == (0, B)
    paths = gtn.viterbi_path(_product(gtn, em_dev, trans, start, targets, False))
    for b in range(B):
        assert labels[b].tolist() == paths[b].labels_to_list()
        wl, _, ws = asg_align_fp64(em[b], trans, start, targets[b])
        assert labels[b].tolist() == wl.tolist() and _score_ok(scores[b], ws)
    with pytest.raises(ValueError, match="token"):
        _align(gtn, em_dev, trans, start, targets, want_tokens=True)
    with pytest.raises(ValueError, match="frame"):
        _align(gtn, em_dev, trans, start, targets, frames=[T] * B, want_tokens=False)


def test_wide_alphabet_product_serves_the_alignment_only(gtn):
    """past the band sweeps' 1024 labels a product of force-alignment acceptors exists for the alignment launch alone:
    forward_score and its gradients over it still go the per-graph way and give what the per-graph functions give"""
    B, T, N = 2, 12, 1028
    rng = np.random.default_rng(1028)
    em = rng.normal(0, 2, (B, T, N)).astype(np.float32)
    trans = rng.normal(0, 1, (N, N)).astype(np.float32)
    start = rng.normal(0, 1, N).astype(np.float32)
    targets = [[5, 1027, 1027, 3], [1000, 2]]
    em_dev = _dev(em)
    labels, tokens, scores, counts = _align(gtn, em_dev, trans, start, targets)
    assert counts == (B, 0)
    for b in range(B):
        _check_row(f"wide b={b}", labels[b], tokens[b], scores[b], asg_align_fp64(em[b], trans, start, targets[b]), T,
                   targets[b])
    res = {}
    for batch in (True, False):
        tg = _transitions(gtn, trans, start)
        tg.calc_grad = True
        if batch:
            ems = gtn.Batch.linear(B, T, N, em_dev, True, True)
            fs = gtn.forward_score(gtn.compose(ems, gtn.Batch.asg_force_align(targets, tg, N)))
            gtn.backward(fs)
            vals = np.asarray(fs.items())
        else:
            ems = gtn.linear_graph_n(B, T, N, em_dev)
            fals = []
            for t in targets:
                f = gtn.Graph(False)
                f.add_node(True, False)
                for l in range(1, len(t) + 1):
                    f.add_node(False, l == len(t))
                    f.add_arc(l - 1, l, int(t[l - 1]))
                    f.add_arc(l, l, int(t[l - 1]))
                fals.append(f)
            fs = gtn.forward_score(gtn.compose(ems, gtn.compose(fals, [tg])))
            gtn.backward(fs)
            vals = np.asarray(gtn.items(fs))
        ge = np.stack([ems[b].grad().weights_to_numpy().reshape(T, N) for b in range(B)])
        res[batch] = (vals, ge, tg.grad().weights_to_numpy().copy())
    np.testing.assert_allclose(res[True][0], res[False][0], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(res[True][1], res[False][1], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(res[True][2], res[False][2], rtol=2e-4, atol=5e-5)


def _torch_entry(gtn, em, trans, start, targets, frames, side_stream):
    import torch
    from gtn_amd import torch_loss
    x = _dev(em).requires_grad_(True)
    tr, st = _dev(trans).requires_grad_(True), _dev(start)
    before = x.detach().clone()
    torch.cuda.synchronize()
    args = (x, tr, targets, st, None if frames is None else frames.tolist())
    try:
        if side_stream:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                out = torch_loss.asg_forced_align(*args)
            torch.cuda.current_stream().wait_stream(s)
        else:
            out = torch_loss.asg_forced_align(*args)
        torch.cuda.synchronize()
    finally:
        gtn.set_stream(None)
    labels, tokens, scores = out
    B, T, _ = em.shape
    assert labels.dtype == torch.int32 and tokens.dtype == torch.int32 and scores.dtype == torch.float32
    assert labels.shape == (B, T) and tokens.shape == (B, T) and scores.shape == (B,)
    assert labels.device == x.device and tokens.device == x.device and scores.device == x.device
    assert not labels.requires_grad and not scores.requires_grad
    assert torch.equal(x.detach(), before)
    return labels.cpu().numpy(), tokens.cpu().numpy(), scores.cpu().numpy()


def _check_torch(out, em, trans, start, targets, frames):
    ln, tn, sn = out
    for b in range(len(targets)):
        f = em.shape[1] if frames is None else int(frames[b])
        _check_row(f"torch b={b}", ln[b], tn[b], sn[b], asg_align_fp64(em[b], trans, start, targets[b], f), f, targets[b])


@pytest.mark.parametrize("side_stream", [True, False])
@pytest.mark.parametrize("seed,B,T,N,Umax,ragged", FP_CASES)
def test_torch_entry(gtn, seed, B, T, N, Umax, ragged, side_stream):
    """torch_loss.asg_forced_align (native route) on a non-default stream and on the default one, with and without
    input_lengths: dtypes, device, shapes; results equal the yardstick; emissions untouched, nothing requires grad;
    counted as the launch"""
    em, trans, start, targets, frames = seeded_case(seed, B, T, N, Umax, ragged)
    f0, b0 = gtn.debug_align_stats()
    out = _torch_entry(gtn, em, trans, start, targets, frames if ragged else None, side_stream)
    f1, b1 = gtn.debug_align_stats()
    assert (f1 - f0, b1 - b0) == (B, 0)
    _check_torch(out, em, trans, start, targets, frames if ragged else None)


_CHILD = "--python-criteria-child"


def test_torch_entry_python_route(tmp_path):
    """GTN_AMD_PYTHON_CRITERIA=1 in a fresh process: Batch.linear(borrow) o Batch.asg_force_align -> viterbi_align"""
    out = str(tmp_path / "child.npz")
    env = dict(os.environ, GTN_AMD_PYTHON_CRITERIA="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), _CHILD, out], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    z = np.load(out)
    i = 0
    for seed, B, T, N, Umax, ragged in FP_CASES:
        em, trans, start, targets, frames = seeded_case(seed, B, T, N, Umax, ragged)
        for side_stream in (True, False):
            _check_torch((z[f"l{i}"], z[f"t{i}"], z[f"s{i}"]), em, trans, start, targets, frames if ragged else None)
            i += 1
    assert int(z["fast"]) == sum(2 * c[1] for c in FP_CASES) and int(z["fallback"]) == 0


def _python_route_child(out):
    sys.path.insert(0, ROOT)
    import gtn_amd as gtn
    from gtn_amd import torch_loss
    assert not torch_loss._native()
    res, i = {}, 0
    for seed, B, T, N, Umax, ragged in FP_CASES:
        em, trans, start, targets, frames = seeded_case(seed, B, T, N, Umax, ragged)
        for side_stream in (True, False):
            res[f"l{i}"], res[f"t{i}"], res[f"s{i}"] = _torch_entry(gtn, em, trans, start, targets,
                                                                    frames if ragged else None, side_stream)
            i += 1
    res["fast"], res["fallback"] = gtn.debug_align_stats()
    np.savez(out, **res)


def test_criteria_abi(gtn):
    """gtn_asg_align_n gives the three tensors the Batch API gives"""
    import torch
    seed, B, T, N, Umax, ragged = FP_CASES[1]
    em, trans, start, targets, frames = seeded_case(seed, B, T, N, Umax, ragged)
    em_dev = _dev(em)
    labels, tokens, scores, _ = _align(gtn, em_dev, trans, start, targets, True, frames)
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    lib.gtn_asg_align_n.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 5
    lib.gtn_asg_align_n.restype = ctypes.c_int
    lib.gtn_criteria_last_error.restype = ctypes.c_char_p
    w = _dev(np.concatenate([start, trans.reshape(-1)]).astype(np.float32))
    flat = np.ascontiguousarray(np.concatenate([np.asarray(t, np.int32) for t in targets]))
    lens = np.ascontiguousarray([len(t) for t in targets], dtype=np.int32)
    lab = torch.full((B, T), SENTINEL, dtype=torch.int32, device="cuda:0")
    tok = torch.full((B, T), SENTINEL, dtype=torch.int32, device="cuda:0")
    sc = torch.full((B,), float("nan"), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rc = lib.gtn_asg_align_n(em_dev.data_ptr(), flat.ctypes.data, lens.ctypes.data, B, T, N, w.data_ptr(),
                             frames.ctypes.data, lab.data_ptr(), tok.data_ptr(), sc.data_ptr())
    assert rc == 0, lib.gtn_criteria_last_error().decode()
    gtn.synchronize()
    assert (lab.cpu().numpy() == labels).all() and (tok.cpu().numpy() == tokens).all()
    assert sc.cpu().numpy().tobytes() == scores.tobytes()


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == _CHILD:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _python_route_child(sys.argv[2])
