"""Batched ASG prefix beam search with a compiled LM graph fused in (asg_beam.hip, the graph instantiation of the search
kernel, through gtnx_batch_asg_beam_decode_graph; gtn_amd.Batch.asg_beam_decode(lm=LmGraph),
gtn_amd.torch_loss.asg_beam_decode(lm_graph=...), gtn_asg_beam_decode_graph_n).  DESIGN section 31.

Two anchors that need no tolerance: with zero weight and bonus and a graph that permits every label the outputs are the
bytes of the call without a graph, and a bigram acceptor whose arcs all weigh 0 gives the bytes of the plain call on the
table with -inf where the acceptor has no arc.  Back-off trigrams and a lexicon, which no table can express, are judged
by the float64 yardstick of tests/asg_beam_graph_fp.py (pinned to a brute-force enumeration by
test_asg_beam_graph_cpu.py): tokens and lengths with ==, sound because every such case vets on the host
(test_asg_beam_graph_cpu.py::test_every_gpu_case_vets), both score kinds within SCORE_FACTOR (8) err of float64, err
being the case's host-side distance of the float32 forms from float64 -- never anything the device gave.  The largest
|device - float64| / err seen on an MI355X is in DESIGN section 31.

Every output sits between guards of sentinels that must survive, as in test_asg_beam_gpu.py, whose harness this is with
the graph's arguments and a fourth output.
"""
import ctypes
import os

import numpy as np
import pytest

import asg_beam_fp as af
import asg_beam_graph_fp as gfp
from test_asg_beam_gpu import SENTINEL, _dev
from test_asg_beam_gpu import _decode as _decode_plain

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tokens", "lengths", "scores", "am_scores")
WORST = {"ratio": 0.0}


def _lm(gtn, G, shuffle=None):
    return gtn.LmGraph(G.to_api(gtn, shuffle_seed=shuffle))


def _decode(gtn, em, table, W, K, nbest, lm, alpha=gfp.ALPHA, beta=gfp.BETA, frames=None, pad=1, address=False,
            am=True, batch=None, host_am=False):
    """Batch.asg_beam_decode(lm=) on Batch.linear with guarded outputs.  Returns the four outputs as numpy and the
    (calls, utterances) this call counted; _decode.raw keeps the arrays with their guards, also when the call raised.
    am=False hands no am_scores over (its array keeps its sentinels); host_am hands over host memory"""
    import torch
    B, T, C = em.shape
    em_dev = _dev(em)  # (borrowed by the batch: it must outlive the call)
    ems = batch if batch is not None else gtn.Batch.linear(B, T, C, em_dev, False, True)
    tok = torch.full((B + 2, nbest, T + pad), SENTINEL, dtype=torch.int32, device="cuda:0")
    ln = torch.full((B * nbest + 2,), SENTINEL, dtype=torch.int32, device="cuda:0")
    sc = torch.full((B * nbest + 2,), float("nan"), dtype=torch.float32, device="cuda:0")
    ams = torch.full((B * nbest + 2,), float("nan"), dtype=torch.float32, device="cuda:0")
    host = np.full(B * nbest, np.nan, np.float32)
    tab = _dev(table)
    torch.cuda.synchronize()
    tv, lv = tok[1:B + 1, :, :T], ln[1:B * nbest + 1].view(B, nbest)
    sv, av = sc[1:B * nbest + 1].view(B, nbest), ams[1:B * nbest + 1].view(B, nbest)
    c0 = gtn.debug_asg_beam_stats()
    try:
        if address or host_am:
            out_am = host.ctypes.data if host_am else (av.data_ptr() if am else None)
            ems.asg_beam_decode(tv.data_ptr(), lv.data_ptr(), sv.data_ptr(), frames, tab.data_ptr(), W, K, nbest,
                                row_stride=T + pad, lm=lm, lm_weight=alpha, insertion_bonus=beta, am_scores_out=out_am)
        else:
            ems.asg_beam_decode(tv, lv, sv, frames, tab, W, K, nbest, lm=lm, lm_weight=alpha, insertion_bonus=beta,
                                am_scores_out=av if am else None)
    finally:
        gtn.synchronize()
        c1 = gtn.debug_asg_beam_stats()
        raw = [t.cpu().numpy() for t in (tok, ln, sc, ams)]
        _decode.raw = raw
        _decode.host = host
        assert (raw[0][0] == SENTINEL).all() and (raw[0][B + 1] == SENTINEL).all(), "tokens: guard rows"
        assert (raw[0][:, :, T:] == SENTINEL).all(), "tokens: guard columns"
        assert raw[1][0] == SENTINEL and raw[1][-1] == SENTINEL, "lengths: guards"
        assert np.isnan(raw[2][0]) and np.isnan(raw[2][-1]), "scores: guards"
        assert np.isnan(raw[3][0]) and np.isnan(raw[3][-1]), "am_scores: guards"
    out = [raw[0][1:B + 1, :, :T]] + [r[1:-1].reshape(B, nbest) for r in raw[1:]]
    return out, (c1[0] - c0[0], c1[1] - c0[1])


def _untouched():
    tok, ln, sc, ams = _decode.raw
    return ((tok == SENTINEL).all() and (ln == SENTINEL).all() and np.isnan(sc).all() and np.isnan(ams).all()
            and np.isnan(_decode.host).all())


def _same_bytes(tag, raw0, raw1, n=4):
    for name, r0, r1 in list(zip(NAMES, raw0, raw1))[:n]:
        assert r0.tobytes() == r1.tobytes(), (tag, name)


def test_zero_weight_and_bonus_is_the_call_without_a_graph(gtn):
    """alpha = beta = 0 with a graph that permits everything: tokens, lengths and scores, guards included, are the
    bytes of the call without a graph, and am_scores those of scores"""
    for case in (af.SHAPE_CASES[9], af.SHAPE_CASES[10], af.RAGGED_CASE, af.RECREATED_CASES[0]):
        kind, seed, B, T, C, W, K, nbest, fr, holes = case
        em, table, _, _ = af.results_of(case)
        frames = None if fr is None else list(fr)
        _decode_plain(gtn, em, table, W, K, nbest, frames=frames)
        plain = _decode_plain.raw
        _, stats = _decode(gtn, em, table, W, K, nbest, _lm(gtn, gfp.trigram_graph(seed, C)), 0.0, 0.0, frames=frames)
        assert stats == (1, B)
        _same_bytes(case, plain, _decode.raw, 3)
        assert _decode.raw[3].tobytes() == _decode.raw[2].tobytes(), case


@pytest.mark.parametrize("holes", [0.0, 0.3])
@pytest.mark.parametrize("shape", gfp.IDENTITY_SHAPES, ids=lambda s: "B{}-T{}-C{}-W{}-K{}".format(*s))
def test_a_zero_weight_bigram_acceptor_is_the_struck_out_table(gtn, shape, holes):
    """a bigram acceptor whose arcs all weigh 0: L stays exactly 0 and s + 0 has s's bits (no score is a zero:
    test_asg_beam_graph_cpu.py), so tokens, lengths and scores are the bytes of the plain call on the table with -inf
    in the start and off-diagonal entries where the acceptor has no arc"""
    B, T, C, W, K = shape
    nbest = min(W, 4)
    em, table, G, struck = gfp.identity_case(shape, holes)
    plain, _ = _decode_plain(gtn, em, struck, W, K, nbest)
    want = _decode_plain.raw
    got, stats = _decode(gtn, em, table, W, K, nbest, _lm(gtn, G, shuffle=C), alpha=0.7, beta=0.0)
    assert stats == (1, B) and np.isfinite(got[2][:, 0]).all() and (got[1][:, 0] > 0).any()
    _same_bytes((shape, holes), want, _decode.raw, 3)
    assert _decode.raw[3].tobytes() == _decode.raw[2].tobytes()


def _want(case):
    """(em, table, G, the float64 outputs, err) of an entry of asg_beam_graph_fp's case lists"""
    seed, B, T, C, W, K, nbest, frames, gkind = case
    em, table, G, res, _ = gfp.results_of(case)
    return em, table, G, gfp.rows_of_graph(res["f64"], T, nbest), gfp.case_err_lm(res, nbest)


def _check(tag, got, want, err):
    """tokens and lengths == the float64 yardstick; both score kinds within 8 err of it (-inf where it is -inf)"""
    for name, g, w in zip(NAMES[:2], got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (tag, name, bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
    for name, g, w in zip(NAMES[2:], got[2:], want[2:]):
        assert g.dtype == np.float32 and g.shape == w.shape and not np.isnan(g).any(), (tag, name)
        dead = np.isneginf(w)
        assert (np.isneginf(g) == dead).all(), (tag, name, g, w)
        dist = float(np.abs(g[~dead].astype(np.float64) - w[~dead]).max()) if (~dead).any() else 0.0
        ratio = dist / err if err else 0.0
        WORST["ratio"] = max(WORST["ratio"], ratio)
        print(f"[asg_beam_graph] {tag} {name}: |device - float64| {dist:.3g}, err {err:.3g}, ratio {ratio:.3g}, "
              f"largest ratio so far {WORST['ratio']:.3g}")
        assert dist <= gfp.SCORE_FACTOR * err, (tag, name, dist, err)


def _run_case(gtn, case, **kw):
    seed, B, T, C, W, K, nbest, frames, gkind = case
    em, table, G, want, err = _want(case)
    got, stats = _decode(gtn, em, table, W, K, nbest, _lm(gtn, G, shuffle=seed),
                         frames=None if frames is None else list(frames), **kw)
    assert stats == (1, B)
    _check(str(case[:7]) + gkind, got, want, err)
    return got


def _rows(got, B, nbest):
    return [[tuple(got[0][b, r, :got[1][b, r]]) for r in range(nbest) if np.isfinite(got[2][b, r])] for b in range(B)]


@pytest.mark.parametrize("case", gfp.TRIGRAM_CASES + gfp.RECREATED_CASES + [gfp.LEXICON_CASE],
                         ids=lambda c: "B{1}-T{2}-C{3}-W{4}-K{5}-n{6}-seed{0}-{8}".format(*c))
def test_trigram_and_lexicon_match_the_yardstick(gtn, case):
    """the state depends on two labels: no table can say this.  Among the cases lane 31 of the set and a unigram state
    with 70 arcs that are not contiguous, a list above 32 prefixes (the second pass of the walks) with epsilon chains
    of 8, a prefix that leaves the list and comes back with its state and its L, and a lexicon whose constraint bites.
    No returned row appears twice, and every one is a sequence the numpy walk accepts"""
    got = _run_case(gtn, case)
    G = gfp.results_of(case)[2]
    for b, rows in enumerate(_rows(got, case[1], case[6])):
        assert len(set(rows)) == len(rows) > 0, b
        for y in rows:
            assert all(a != c for a, c in zip(y, y[1:])) and gfp.accepts(G, y), (b, y)
    if case == gfp.LEXICON_CASE:
        seed, B, T, C, W, K, nbest, _, _ = case
        em, table = gfp.results_of(case)[:2]
        free, _ = _decode_plain(gtn, em, table, W, K, nbest)
        assert not all(gfp.accepts(G, y) for rows in _rows(free, B, nbest) for y in rows)


def test_unpruned_am_scores_are_asg_score_and_the_rest_is_the_walk(gtn):
    """C = 4, T = 5, W = 64, K = C: no ancestor of a returned hypothesis is pruned (test_asg_beam_graph_cpu.py checks
    it against the enumeration), so am_scores is Batch.asg_score of the returned tokens, run on the device from the
    returned tensors, within the 8 err of test_asg_beam_gpu.py's unpruned test; scores - am_scores is the host walk's L
    within the rounding of the float32 sums involved; every returned sequence is accepted"""
    import torch
    case = gfp.UNPRUNED_CASE
    seed, B, T, C, W, K, nbest, _, _ = case
    assert T == 5 and C == 4 and W == 64 and K == C
    got = _run_case(gtn, case)
    em, table, G, _, err = _want(case)
    x, tab = _dev(em), _dev(table)
    ems = gtn.Batch.linear(B, T, C, x, False, True)
    ref = torch.full((B, nbest), float("nan"), dtype=torch.float32, device="cuda:0")
    ems.asg_score(tab, _dev(got[0]), _dev(got[1]), ref, max_length=T)
    gtn.synchronize()
    ref = ref.cpu().numpy()
    eps = float(np.finfo(np.float32).eps)
    for b in range(B):
        for r in range(nbest):
            assert np.isfinite(got[3][b, r])
            y = tuple(got[0][b, r, :got[1][b, r]])
            assert gfp.accepts(G, y), (b, r, y)
            am, total = float(got[3][b, r]), float(got[2][b, r])
            d_ref = abs(am - float(ref[b, r]))
            L32 = gfp.walk_score(G, y, gfp.ALPHA, gfp.BETA, np.float32)
            L64 = float(gfp.walk_score(G, y, gfp.ALPHA, gfp.BETA))
            # the device's L is the float32 walked sum; scores = fl(am + L), so scores - am is L up to that one rounding
            d_L = abs((total - am) - float(L32))
            print(f"[asg_beam_graph] unpruned b={b} r={r}: |am - asg_score| {d_ref:.3g} (err {err:.3g}), "
                  f"|(scores - am) - L| {d_L:.3g}, |L32 - L64| {abs(float(L32) - L64):.3g}")
            assert d_ref <= gfp.SCORE_FACTOR * err, (b, r, d_ref, err)
            assert np.float32(np.float32(am) + L32).tobytes() == got[2][b, r].tobytes(), (b, r)
            assert d_L <= eps * max(abs(total), abs(am), abs(float(L32))), (b, r, d_L)


def test_mixed_frame_counts(gtn):
    """per-utterance lengths with 0, 1, T - 1 and T among them: the yardstick at each length; NaN in every pad row
    changes no bit of any output"""
    case = gfp.RAGGED_CASE
    seed, B, T, C, W, K, nbest, fr, gkind = case
    assert 0 in fr and 1 in fr and T - 1 in fr and T in fr
    got = _run_case(gtn, case)
    raw = _decode.raw
    em, table, G, _, _ = _want(case)
    poisoned = em.copy()
    for b in range(B):
        poisoned[b, fr[b]:] = np.nan
    _decode(gtn, poisoned, table, W, K, nbest, _lm(gtn, G), frames=list(fr))
    _same_bytes("pad rows", raw, _decode.raw)
    for b in range(B):
        if fr[b] == 0:
            assert (got[0][b] == -1).all() and (got[1][b] == 0).all()
            assert np.isneginf(got[2][b]).all() and np.isneginf(got[3][b]).all()


def test_two_runs_give_the_same_bits(gtn):
    for case in (gfp.TRIGRAM_CASES[1], gfp.TRIGRAM_CASES[2]):
        seed, B, T, C, W, K, nbest, frames, gkind = case
        em, table, G, _, _ = _want(case)
        lm = _lm(gtn, G)
        _decode(gtn, em, table, W, K, nbest, lm)
        first = _decode.raw
        _decode(gtn, em, table, W, K, nbest, lm)
        _same_bytes(case, first, _decode.raw)


@pytest.mark.parametrize("address", [False, True])
def test_row_stride_above_M(gtn, address):
    """rows 5 entries wider than M, as tensor views and as raw device addresses: the gap keeps its sentinels (the
    harness asserts it) and the rest has the bits of dense rows"""
    case = gfp.TORCH_CASE
    seed, B, T, C, W, K, nbest, frames, gkind = case
    wide = _run_case(gtn, case, pad=5, address=address)
    em, table, G, _, _ = _want(case)
    dense, stats = _decode(gtn, em, table, W, K, nbest, _lm(gtn, G), pad=0)
    assert stats == (1, B)
    for name, g, d in zip(NAMES, wide, dense):
        assert g.tobytes() == d.tobytes(), name


def test_null_am_scores(gtn):
    """without am_scores the other three outputs have the same bytes, and nothing is written where it would have been"""
    case = gfp.TORCH_CASE
    seed, B, T, C, W, K, nbest, frames, gkind = case
    em, table, G, _, _ = _want(case)
    lm = _lm(gtn, G)
    _decode(gtn, em, table, W, K, nbest, lm)
    full = _decode.raw
    for address in (False, True):
        _, stats = _decode(gtn, em, table, W, K, nbest, lm, am=False, address=address)
        assert stats == (1, B)
        _same_bytes("null am_scores", full, _decode.raw, 3)
        assert np.isnan(_decode.raw[3]).all()


def test_refusals_leave_every_output_untouched(gtn):
    """a destroyed handle, a weight or bonus that is not finite, a batch that is not linear, am_scores on the host and
    the shape limits: ValueError under the graph call's name, no output has changed and nothing was counted"""
    B, T, C = 3, 9, 8
    em = af.continuous_case(83, B, T, C)
    table = af.table_case(83, C)
    G = gfp.trigram_graph(83, C)
    lm = _lm(gtn, G)
    name = r"\[gtnx_batch_asg_beam_decode_graph\] "
    c0 = gtn.debug_asg_beam_stats()
    for alpha, beta in ((float("nan"), 0.0), (float("inf"), 0.0), (1.0, float("-inf"))):
        with pytest.raises(ValueError, match="must be finite"):
            _decode(gtn, em, table, 4, 4, 2, lm, alpha=alpha, beta=beta)
        assert _untouched()
    stale = _lm(gtn, G)
    gone = stale._h
    stale.destroy()
    with pytest.raises(ValueError, match=name + "null LM graph handle"):
        _decode(gtn, em, table, 4, 4, 2, stale)
    assert _untouched()
    foreign = ctypes.create_string_buffer(256)
    for handle in (gone, ctypes.addressof(foreign)):
        stale._h = handle
        try:
            with pytest.raises(ValueError, match=name + "not a live LM graph handle"):
                _decode(gtn, em, table, 4, 4, 2, stale)
        finally:
            stale._h = None
        assert _untouched()
    graphs = gtn.Batch([gtn.linear_graph(T, C) for _ in range(B)])
    with pytest.raises(ValueError, match=name + "not a native linear batch"):
        _decode(gtn, em, table, 4, 4, 2, lm, batch=graphs, address=True)
    assert _untouched()
    with pytest.raises(ValueError, match=name + "am_scores is not memory of the engine's current device"):
        _decode(gtn, em, table, 4, 4, 2, lm, host_am=True)  # (pageable host memory)
    assert _untouched()
    for kw, msg in ((dict(W=65), "beam_size outside 1 .. 64"), (dict(K=33), "cutoff_top_n outside 1 .. 32"),
                    (dict(nbest=5), "nbest outside 1 .. beam_size"), (dict(W=0, nbest=1), "beam_size outside 1 .. 64")):
        a = dict(W=4, K=4, nbest=2)
        a.update(kw)
        with pytest.raises(ValueError, match=name + msg):
            _decode(gtn, em, table, a["W"], a["K"], a["nbest"], lm)
        assert _untouched()
    with pytest.raises(ValueError, match=name + "row_stride is shorter than the rows of the batch"):
        _decode(gtn, em, table, 4, 4, 2, lm, pad=-1, address=True)
    assert _untouched()
    with pytest.raises(ValueError, match=name + "a frame count outside 0 .. M"):
        _decode(gtn, em, table, 4, 4, 2, lm, frames=[T + 1, 1, 1])
    assert _untouched()
    wide = np.zeros((1, 1, (1 << 19) + 1), np.float32)
    with pytest.raises(ValueError, match=name + r"more than 2\^19 labels"):
        _decode(gtn, wide, np.zeros(2, np.float32), 4, 4, 2, lm, address=True)
    assert _untouched()
    assert gtn.debug_asg_beam_stats() == c0
    got, stats = _decode(gtn, em, table, 4, 4, 2, lm)  # (the graph itself is fine)
    assert stats == (1, B) and np.isfinite(got[2][:, 0]).all()


def test_rows_times_beam_beyond_an_int_is_refused(gtn):
    """M * beam_size must fit an int (a one-label batch of 2^25 rows at beam_size 64)"""
    import torch
    ln = torch.full((4,), SENTINEL, dtype=torch.int32, device="cuda:0")
    sc = torch.full((4,), float("nan"), dtype=torch.float32, device="cuda:0")
    tok = torch.full((4, 1), SENTINEL, dtype=torch.int32, device="cuda:0")
    tab = torch.zeros(2, device="cuda:0")
    lm = _lm(gtn, gfp.trigram_graph(1, 2))
    c0 = gtn.debug_asg_beam_stats()
    M = 1 << 25
    x = torch.zeros(1, M, 1, device="cuda:0")
    ems = gtn.Batch.linear(1, M, 1, x, False, True)
    msg = r"\[gtnx_batch_asg_beam_decode_graph\] rows times beam_size does not fit an int"
    with pytest.raises(ValueError, match=msg):
        ems.asg_beam_decode(tok.data_ptr(), ln[1:], sc[1:], None, tab, 64, 1, 1, row_stride=M, lm=lm,
                            am_scores_out=sc[2:])
    gtn.synchronize()
    assert (ln == SENTINEL).all() and sc.isnan().all() and (tok == SENTINEL).all()
    assert gtn.debug_asg_beam_stats() == c0


def test_torch_entry_and_criteria_abi_equal_the_batch_route(gtn):
    """torch_loss.asg_beam_decode(lm_graph=) gives the bytes of Batch.asg_beam_decode(lm=LmGraph), three tensors unless
    return_am_scores; gtn_asg_beam_decode_graph_n gives them too, am_scores null allowed"""
    import torch
    from gtn_amd import torch_loss
    case = gfp.TORCH_CASE
    seed, B, T, C, W, K, nbest, frames, gkind = case
    em, table, G, want, err = _want(case)
    lm = _lm(gtn, G)
    x = _dev(em)
    tr, start = _dev(table[C:].reshape(C, C)), _dev(table[:C])
    kw = dict(beam_size=W, cutoff_top_n=K, nbest=nbest, lm_graph=lm, lm_weight=gfp.ALPHA, insertion_bonus=gfp.BETA)
    try:
        c0 = gtn.debug_asg_beam_stats()
        out4 = torch_loss.asg_beam_decode(x, tr, start, return_am_scores=True, **kw)
        c1 = gtn.debug_asg_beam_stats()
        out3 = torch_loss.asg_beam_decode(x, tr, start, **kw)
        torch.cuda.synchronize()
    finally:
        gtn.set_stream(None)
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, B) and len(out4) == 4 and len(out3) == 3
    kinds = ((torch.int32, (B, nbest, T)), (torch.int32, (B, nbest)), (torch.float32, (B, nbest)),
             (torch.float32, (B, nbest)))
    for o, (dt, shape) in zip(out4, kinds):
        assert o.dtype == dt and o.shape == shape and o.device == x.device and not o.requires_grad
    out4 = [o.cpu().numpy() for o in out4]
    _check("torch", out4, want, err)
    got, _ = _decode(gtn, em, table, W, K, nbest, lm, pad=0)
    for name, g, o in zip(NAMES, got, out4):
        assert g.tobytes() == o.tobytes(), name
    for g, o in zip(out4, out3):
        assert g.tobytes() == o.cpu().numpy().tobytes()
    # the criteria library's C entry
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    fn = lib.gtn_asg_beam_decode_graph_n
    fn.argtypes = ([ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3
                   + [ctypes.c_void_p] + [ctypes.c_float] * 2 + [ctypes.c_void_p] * 4)
    fn.restype = ctypes.c_int
    lib.gtn_criteria_last_error.restype = ctypes.c_char_p
    w_dev = _dev(table)
    tok = torch.full((B, nbest, T), SENTINEL, dtype=torch.int32, device="cuda:0")
    le = torch.full((B, nbest), SENTINEL, dtype=torch.int32, device="cuda:0")
    sc = torch.full((B, nbest), float("nan"), dtype=torch.float32, device="cuda:0")
    ams = torch.full((B, nbest), float("nan"), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rc = fn(x.data_ptr(), B, T, C, w_dev.data_ptr(), None, W, K, nbest, lm._h, gfp.ALPHA, gfp.BETA, tok.data_ptr(),
            le.data_ptr(), sc.data_ptr(), ams.data_ptr())
    assert rc == 0, lib.gtn_criteria_last_error().decode()
    gtn.synchronize()
    for name, t, o in zip(NAMES, (tok, le, sc, ams), out4):
        assert t.cpu().numpy().tobytes() == o.tobytes(), name
    ams.fill_(float("nan"))
    torch.cuda.synchronize()
    rc = fn(x.data_ptr(), B, T, C, w_dev.data_ptr(), None, W, K, nbest, lm._h, gfp.ALPHA, gfp.BETA, tok.data_ptr(),
            le.data_ptr(), sc.data_ptr(), None)
    assert rc == 0, lib.gtn_criteria_last_error().decode()
    gtn.synchronize()
    assert sc.cpu().numpy().tobytes() == out4[2].tobytes() and torch.isnan(ams).all()
    rc = fn(x.data_ptr(), B, T, C, w_dev.data_ptr(), None, W, K, nbest, None, gfp.ALPHA, gfp.BETA, tok.data_ptr(),
            le.data_ptr(), sc.data_ptr(), None)
    assert rc == -1
    assert "[gtnx_batch_asg_beam_decode_graph] null LM graph handle" in lib.gtn_criteria_last_error().decode()
