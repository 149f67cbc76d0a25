"""Batched CTC forced alignment with device-resident output (gtnx_batch_viterbi_align, align.hip;
gtn_amd.Batch.viterbi_align, gtn_amd.torch_loss.ctc_forced_align).

The judge of labels and scores is the oracle's shortest path on the lattice the reference would build
(oracle_path below: compose the CTC target with the chain, shortest_path()), as tests/test_lazy_gpu.py uses it.
Every utterance a test does not construct to be infeasible has at least U + (adjacent equal labels) frames, which is
exactly when a CTC path exists; the tests assert that on their inputs before they call the engine.
"""
import numpy as np
import pytest

import graphgen as gg
from ctc_align_fp import FP_CASES, ctc_align_fp64, min_frames, seeded_case
from test_align_cpu import oracle_path

pytestmark = pytest.mark.gpu
SENTINEL = -7


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _align(gtn, em_dev, targets, blank=0, chain_first=False, frames=None, want_tokens=True):
    """Batch.viterbi_align on ctc_targets x linear; outputs allocated with a guard row and column that must survive.
    Returns (labels [B, T], tokens [B, T] or None, scores [B], (fast, fallback) utterance counts of this call)"""
    import torch
    B, T, C = em_dev.shape
    ctcs = gtn.Batch.ctc_targets([list(t) for t in targets], blank, False)
    ems = gtn.Batch.linear(B, T, C, em_dev, False, True)
    comp = gtn.compose(ems, ctcs) if chain_first else gtn.intersect(ctcs, ems)
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


def _check_tokens(labels, tokens, target, blank):
    """labels[t] == target[tokens[t]] where tokens[t] >= 0, blank elsewhere; tokens non-decreasing over their
    non-negative entries in steps of at most 1; every index occurs"""
    target = np.asarray(target, np.int64)
    on = tokens >= 0
    assert (labels[on] == target[tokens[on]]).all()
    assert (labels[~on] == blank).all()
    steps = np.diff(tokens[on])
    assert ((steps == 0) | (steps == 1)).all()
    assert sorted(set(tokens[on].tolist())) == list(range(len(target)))


def _assert_feasible(targets, frames):
    for t, f in zip(targets, frames):
        assert f >= min_frames(t), (t, f)


def _score_ok(got, want):
    return got == np.float32(want) or abs(got - want) <= 1e-6 * abs(want)


@pytest.mark.parametrize("B,T,C,U,chain_first,fast", [
    (4, 60, 9, 7, False, False),  # nine labels, not a multiple of 4: the path-graph route
    (4, 60, 12, 7, False, True),  # (... and the same shape on an alphabet the launch takes)
    (3, 200, 64, 40, True, True),
    (2, 300, 20, 140, False, True),   # 281-node targets: eight nodes per lane
    (2, 33, 300, 5, False, True),     # a wide alphabet (300 = 4 x 75: the launch takes it)
    (1, 1, 4, 1, False, True),
])
def test_align_vs_oracle(gtn, B, T, C, U, chain_first, fast):
    """float weights at the shapes of test_lazy_gpu.py::test_band_viterbi_vs_oracle: labels equal the oracle's path
    labels, scores bit-equal or within 1e-6 relative, tokens consistent with labels and targets; the counters show
    the one launch for every shape whose alphabet is a multiple of 4 -- all but the first, whose nine labels take the
    path-graph route (that shape is run a second time with twelve labels)"""
    rng = np.random.default_rng(T * 7 + C)
    em = rng.normal(0, 2, (B, T, C)).astype(np.float32)
    tg = [rng.integers(1, C, int(rng.integers(max(1, U // 2), U + 1))).tolist() for _ in range(B)]
    _assert_feasible(tg, [T] * B)
    is_fast = C % 4 == 0
    assert fast == is_fast
    labels, tokens, scores, (nf, nb) = _align(gtn, _dev(em), tg, 0, chain_first, None, want_tokens=is_fast)
    assert (nf, nb) == ((B, 0) if is_fast else (0, B))
    for b in range(B):
        want_score, want = oracle_path(em[b], tg[b], 0, chain_first)
        assert want is not None
        print(f"[align] shape {(B, T, C, U)} b={b} score {scores[b]!r} oracle {want_score!r}")
        assert labels[b].tolist() == want
        assert _score_ok(scores[b], want_score)
        if is_fast:
            _check_tokens(labels[b], tokens[b], tg[b], 0)
    if not is_fast:  # token indices are not defined on the path-graph route: an error, not garbage
        with pytest.raises(ValueError, match="token"):
            _align(gtn, _dev(em), tg, 0, chain_first, None, want_tokens=True)


def test_align_exact_ties_follow_the_reference(gtn):
    """integer emissions make exact ties, which the launch decides by the reference's queue order (closed-form node
    ranks) without a flag or a second launch: the batch of test_band_viterbi_exact_ties_follow_the_reference (the
    all-zero utterance included) -- as it is (five labels: the path-graph route) and with its alphabet padded to
    eight columns no target uses (the launch) -- plus seeded random targets with repeated labels"""
    B, T, C = 5, 12, 5
    rng = np.random.default_rng(3)
    em = rng.integers(-1, 2, (B, T, C)).astype(np.float32)
    em[0] = 0.0
    tg = [[1, 2], [3, 3, 1], [4], [1, 2, 3, 4], [2, 2]]
    _assert_feasible(tg, [T] * B)
    labels, _, scores, (nf, nb) = _align(gtn, _dev(em), tg, want_tokens=False)
    assert (nf, nb) == (0, B)
    for b in range(B):
        want_score, want = oracle_path(em[b], tg[b])
        assert labels[b].tolist() == want and scores[b] == np.float32(want_score)
    em8 = np.concatenate([em, rng.integers(-1, 2, (B, T, 3)).astype(np.float32)], axis=2)
    labels, tokens, scores, (nf, nb) = _align(gtn, _dev(em8), tg)
    assert (nf, nb) == (B, 0)
    for b in range(B):
        want_score, want = oracle_path(em8[b], tg[b])
        assert labels[b].tolist() == want and scores[b] == np.float32(want_score)
        _check_tokens(labels[b], tokens[b], tg[b], 0)
    for seed, B, T, C, Umax, nlab in [(11, 24, 14, 8, 6, 3), (12, 16, 30, 4, 12, 3), (13, 6, 40, 16, 70, 5),
                                      (14, 4, 300, 8, 140, 7)]:
        rng = np.random.default_rng(seed)
        em = rng.integers(-1, 2, (B, T, C)).astype(np.float32)
        tg = []
        while len(tg) < B:
            t = rng.integers(1, 1 + nlab, int(rng.integers(0, Umax + 1))).tolist()
            if min_frames(t) <= T:
                tg.append(t)
        _assert_feasible(tg, [T] * B)
        labels, tokens, scores, (nf, nb) = _align(gtn, _dev(em), tg)
        assert (nf, nb) == (B, 0)
        for b in range(B):
            want_score, want = oracle_path(em[b], tg[b])
            assert want is not None
            assert labels[b].tolist() == want, (seed, b, tg[b])
            assert scores[b] == np.float32(want_score)
            _check_tokens(labels[b], tokens[b], tg[b], 0)


def test_align_blank_not_the_smallest_label(gtn):
    """blank = C - 1 (the closed form of the tie ranks does not apply: path-graph route), integer emissions"""
    B, T, C = 8, 16, 8
    rng = np.random.default_rng(21)
    em = rng.integers(-1, 2, (B, T, C)).astype(np.float32)
    tg = []
    while len(tg) < B:
        t = rng.integers(0, C - 1, int(rng.integers(1, 7))).tolist()
        if min_frames(t) <= T:
            tg.append(t)
    _assert_feasible(tg, [T] * B)
    labels, _, scores, (nf, nb) = _align(gtn, _dev(em), tg, blank=C - 1, want_tokens=False)
    assert (nf, nb) == (0, B)
    for b in range(B):
        want_score, want = oracle_path(em[b], tg[b], blank=C - 1)
        assert want is not None
        assert labels[b].tolist() == want and scores[b] == np.float32(want_score)


def test_align_frames(gtn):
    """mixed lengths in one batch: row b is the oracle's path on em[b, :frames[b]], -1 beyond; one utterance made
    infeasible (one frame fewer than labels): score -inf, rows of -1, its neighbours unaffected"""
    B, T, C, Umax = 9, 90, 16, 30
    em, tg, frames = seeded_case(31, B, T, C, Umax, ragged_frames=True)
    bad = 4
    frames[bad] = len(tg[bad]) - 1 if len(tg[bad]) > 1 else 0
    if len(tg[bad]) < 2:
        tg[bad] = [3, 5, 3]
        frames[bad] = 2
    frames[0] = T
    frames[B - 1] = min_frames(tg[B - 1])  # the shortest that fits
    _assert_feasible([t for b, t in enumerate(tg) if b != bad], [f for b, f in enumerate(frames) if b != bad])
    assert frames[bad] < min_frames(tg[bad])
    labels, tokens, scores, (nf, nb) = _align(gtn, _dev(em), tg, frames=frames)
    assert (nf, nb) == (B, 0)
    for b in range(B):
        f = int(frames[b])
        assert (labels[b, f:] == -1).all() and (tokens[b, f:] == -1).all()
        if b == bad:
            assert scores[b] == -np.inf and (labels[b] == -1).all() and (tokens[b] == -1).all()
            continue
        want_score, want = oracle_path(em[b, :f], tg[b])
        assert want is not None
        assert labels[b, :f].tolist() == want
        assert _score_ok(scores[b], want_score)
        _check_tokens(labels[b, :f], tokens[b, :f], tg[b], 0)


def test_align_full_size_c3(gtn):
    """BASELINE config C3 (B = 512, T = 1000, C = 256, U <= 100, seeded floats): the labels of all 512 utterances equal
    those of the existing gtn.viterbi_path(Batch) route on the same tensors, 8 seeded utterances also the oracle's"""
    import torch
    B, T, C, U = 512, 1000, 256, 100
    rng = np.random.default_rng(2024)
    em = (rng.random((B, T, C), dtype=np.float32) * 10 - 5).astype(np.float32)
    tg = [rng.integers(1, C, int(rng.integers(U // 2, U + 1))).tolist() for _ in range(B)]
    _assert_feasible(tg, [T] * B)
    em_dev = _dev(em)
    labels, tokens, scores, (nf, nb) = _align(gtn, em_dev, tg)
    assert (nf, nb) == (B, 0)
    ctcs = gtn.Batch.ctc_targets(tg, 0, False)
    ems = gtn.Batch.linear(B, T, C, em_dev, False, True)
    paths = gtn.viterbi_path(gtn.intersect(ctcs, ems))
    for b in range(B):
        p = paths[b]
        assert labels[b].tolist() == p.labels_to_list(), b
    for b in np.random.default_rng(7).choice(B, 8, replace=False):
        want_score, want = oracle_path(em[b], tg[b])
        assert labels[b].tolist() == want
        assert _score_ok(scores[b], want_score)
        _check_tokens(labels[b], tokens[b], tg[b], 0)
    del em_dev
    torch.cuda.empty_cache()


@pytest.mark.parametrize("side_stream", [True, False])
@pytest.mark.parametrize("seed,B,T,C,Umax,ragged", FP_CASES)
def test_torch_entry(gtn, seed, B, T, C, Umax, ragged, side_stream):
    """torch_loss.ctc_forced_align on a non-default stream and on the default one: dtypes, device, shapes; labels
    equal the float64 trellis Viterbi of tests/ctc_align_fp.py (pinned to the oracle on these very inputs by
    tests/test_align_cpu.py); log_probs is left untouched and nothing requires grad"""
    import torch
    from gtn_amd import torch_loss
    em, tg, frames = seeded_case(seed, B, T, C, Umax, ragged)
    _assert_feasible(tg, frames)
    x = _dev(em).requires_grad_(True)
    before = x.detach().clone()
    torch.cuda.synchronize()
    f0, b0 = gtn.debug_align_stats()
    try:
        if side_stream:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                out = torch_loss.ctc_forced_align(x, tg, 0, frames.tolist() if ragged else None)
            torch.cuda.current_stream().wait_stream(s)
        else:
            out = torch_loss.ctc_forced_align(x, tg, 0, frames.tolist() if ragged else None)
        torch.cuda.synchronize()
    finally:
        gtn.set_stream(None)
    f1, b1 = gtn.debug_align_stats()
    assert (f1 - f0, b1 - b0) == (B, 0)
    labels, tokens, scores = out
    assert labels.dtype == torch.int32 and tokens.dtype == torch.int32 and scores.dtype == torch.float32
    assert labels.shape == (B, T) and tokens.shape == (B, T) and scores.shape == (B,)
    assert labels.device == x.device and tokens.device == x.device and scores.device == x.device
    assert not labels.requires_grad and not scores.requires_grad
    assert torch.equal(x.detach(), before)
    ln, tn, sn = labels.cpu().numpy(), tokens.cpu().numpy(), scores.cpu().numpy()
    for b in range(B):
        wl, wt, ws = ctc_align_fp64(em[b], tg[b], 0, int(frames[b]))
        assert ln[b].tolist() == wl.tolist()
        assert tn[b].tolist() == wt.tolist()
        assert abs(sn[b] - ws) <= 1e-5 * max(1.0, abs(ws))


def test_align_fallback_is_total(gtn):
    """a GRAPHS batch (host-built targets, compositions BUILT under compose_mode(0)) gives the labels of viterbi_path +
    labels_to_list; token indices are an error there, and so are frame counts"""
    import torch
    B, T, C = 5, 25, 7
    rng = np.random.default_rng(41)
    em = rng.normal(0, 2, (B, T, C)).astype(np.float32)
    tg = [rng.integers(1, C, int(rng.integers(1, 8))).tolist() for _ in range(B)]
    _assert_feasible(tg, [T] * B)
    prev = gtn.compose_mode(0)
    try:
        ems = gtn.linear_graph_n(B, T, C, _dev(em))
        ctcs = [gg.to_api(gtn, gg.ctc_target_graph(t)) for t in tg]
        comp = gtn.intersect(ctcs, ems)
        batch = gtn.Batch(comp)
        lab = torch.full((B, T + 3), SENTINEL, dtype=torch.int32, device="cuda:0")
        sc = torch.empty(B, dtype=torch.float32, device="cuda:0")
        f0, b0 = gtn.debug_align_stats()
        batch.viterbi_align(lab, None, sc)
        gtn.synchronize()
        f1, b1 = gtn.debug_align_stats()
        assert (f1 - f0, b1 - b0) == (0, B)
        paths = gtn.viterbi_path(comp)
        labn, scn = lab.cpu().numpy(), sc.cpu().numpy()
        for b in range(B):
            want = paths[b].labels_to_list()
            assert len(want) == T and labn[b, :T].tolist() == want
            assert (labn[b, T:] == SENTINEL).all()
            want_score, want_o = oracle_path(em[b], tg[b])
            assert want == want_o and _score_ok(scn[b], want_score)
        tok = torch.empty((B, T + 3), dtype=torch.int32, device="cuda:0")
        with pytest.raises(ValueError, match="token"):
            batch.viterbi_align(lab, tok)
        with pytest.raises(ValueError, match="frame"):
            batch.viterbi_align(lab, None, None, [T] * B)
    finally:
        gtn.compose_mode(prev)
