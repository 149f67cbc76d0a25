"""Batched CTC prefix beam search with a compiled LM graph fused in (ctc_beam.hip, the graph instantiation of the search
kernel, through gtnx_batch_ctc_beam_decode_graph; gtn_amd.LmGraph, gtn_amd.Batch.ctc_beam_decode(lm=LmGraph),
gtn_amd.torch_loss.ctc_beam_decode(lm_graph=...), gtn_ctc_beam_decode_graph_n).  DESIGN section 30.

Two anchors.  A graph that spells a bigram table -- in full, or as a back-off bigram expanded on the host -- must give
the bytes of the table route, which needs no tolerance.  A back-off trigram, which no table can express, is judged by
the float64 yardstick of tests/ctc_beam_graph_fp.py (pinned to a brute-force enumeration by
test_ctc_beam_graph_cpu.py): tokens and lengths with ==, sound because every such case vets on the host
(test_ctc_beam_graph_cpu.py::test_every_gpu_case_vets), both score kinds within 8 err of float64, err being the case's
host-side distance of the float32 forms from float64 -- never anything the device gave.  The largest
|device - float64| / err seen on an MI355X is in DESIGN section 30.

The guard-sentinel harness is test_ctc_beam_lm_gpu.py's.
"""
import ctypes
import os

import numpy as np
import pytest

import ctc_beam_fp as fp
import ctc_beam_graph_fp as gfp
import ctc_beam_lm_fp as lfp
from test_ctc_beam_lm_gpu import NAMES, SENTINEL, _decode, _dev, _untouched

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY_SHAPES = [(1, 5, 5, 2, 3), (3, 63, 33, 16, 16), (2, 65, 129, 64, 32)]  # (B, T, C, W, K)


def _lm(gtn, G, shuffle=None):
    return gtn.LmGraph(G.to_api(gtn, shuffle_seed=shuffle))


def _same_bytes(tag, raw0, raw1, names=NAMES):
    for name, r0, r1 in zip(NAMES, raw0, raw1):
        if name in names:
            assert r0.tobytes() == r1.tobytes(), (tag, name)


@pytest.mark.parametrize("holes", [0.0, 0.3])
@pytest.mark.parametrize("shape", IDENTITY_SHAPES, ids=lambda s: "B{}-T{}-C{}-W{}-K{}".format(*s))
def test_a_full_bigram_graph_is_the_table_route(gtn, shape, holes):
    """a random table as a graph -- a start state and a state per label, every arc whose entry is above -inf: all four
    outputs, guards included, are the bytes of ctc_beam_decode(lm=table)"""
    B, T, C, W, K = shape
    nbest = min(W, 4)
    em = fp.continuous_case(C + 1, B, T, C)
    w = lfp.table_case(C + 1, C, holes)
    _, stats = _decode(gtn, em, 0, W, K, nbest, w)
    table = _decode.raw
    got, stats = _decode(gtn, em, 0, W, K, nbest, lm=_lm(gtn, gfp.bigram_graph(w, C), shuffle=C))
    assert stats == (1, B) and np.isfinite(got[2][:, 0]).all() and (got[1][:, 0] > 0).any()
    _same_bytes((shape, holes), table, _decode.raw)


@pytest.mark.parametrize("shape", IDENTITY_SHAPES, ids=lambda s: "B{}-T{}-C{}-W{}-K{}".format(*s))
def test_a_backoff_bigram_graph_is_its_expanded_table(gtn, shape):
    """every label state has some arcs and an epsilon arc to a unigram state with all of them; expanded on the host into
    w[C + i*C + j] = walk(state_j, i) (float32, in walk order) the table route gives the same bytes"""
    B, T, C, W, K = shape
    nbest = min(W, 4)
    em = fp.continuous_case(C + 2, B, T, C)
    G = gfp.backoff_bigram_graph(C, C)
    w = gfp.expand_bigram(G, C)
    assert np.isfinite(w).all() and any(-1 in G.out[2 + c] and len(G.out[2 + c]) < C for c in range(C))
    _decode(gtn, em, C - 1, W, K, nbest, w)
    table = _decode.raw
    got, stats = _decode(gtn, em, C - 1, W, K, nbest, lm=_lm(gtn, G, shuffle=C))
    assert stats == (1, B) and np.isfinite(got[2][:, 0]).all()
    _same_bytes(shape, table, _decode.raw)


def test_zero_weight_and_bonus_is_the_call_without_a_language_model(gtn):
    """alpha = beta = 0 with a graph that permits everything: every output byte-equal to the call without a language
    model, am_scores to scores"""
    for case in (fp.SHAPE_CASES[9], fp.SHAPE_CASES[10], fp.RAGGED_CASE, fp.RECREATED_CASES[0]):
        kind, seed, B, T, C, blank, W, K, nbest, fr = case
        em = fp.results_of(case)[0]
        frames = None if fr is None else list(fr)
        _decode(gtn, em, blank, W, K, nbest, frames=frames)
        plain = _decode.raw
        _decode(gtn, em, blank, W, K, nbest, alpha=0.0, beta=0.0, frames=frames, lm=_lm(gtn, gfp.trigram_graph(seed, C)))
        _same_bytes(case, plain, _decode.raw, NAMES[:3])
        assert _decode.raw[3][1:-1].tobytes() == _decode.raw[2][1:-1].tobytes(), case


def _want(case):
    """(em, G, the float64 outputs, err) of an entry of ctc_beam_graph_fp's case lists"""
    seed, B, T, C, blank, W, K, nbest, frames, gkind = case
    em, G, res, _ = gfp.results_of(case)
    tokens = np.full((B, nbest, T), -1, np.int32)
    lengths = np.zeros((B, nbest), np.int32)
    scores = np.full((B, nbest), -np.inf, np.float64)
    am_scores = np.full((B, nbest), -np.inf, np.float64)
    for b in range(B):
        for r, (toks, s, a) in enumerate(res["f64"][b][:nbest]):
            tokens[b, r, :len(toks)] = toks
            lengths[b, r] = len(toks)
            scores[b, r] = s
            am_scores[b, r] = a
    return em, G, (tokens, lengths, scores, am_scores), gfp.case_err_lm(res, nbest)


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
        print(f"[ctc_beam_graph] {tag} {name}: |device - float64| {dist:.3g}, err {err:.3g}, "
              f"ratio {dist / err if err else 0:.3g}")
        assert dist <= gfp.SCORE_FACTOR * err, (tag, name, dist, err)


def _run_case(gtn, case, **kw):
    seed, B, T, C, blank, W, K, nbest, frames, gkind = case
    em, G, want, err = _want(case)
    got, stats = _decode(gtn, em, blank, W, K, nbest, lm=_lm(gtn, G, shuffle=seed),
                         frames=None if frames is None else list(frames), **kw)
    assert stats == (1, B)
    _check(str(case[:8]) + case[9], got, want, err)
    return got


@pytest.mark.parametrize("case", gfp.TRIGRAM_CASES + gfp.RECREATED_CASES,
                         ids=lambda c: "B{1}-T{2}-C{3}-blank{4}-W{5}-K{6}-n{7}-seed{0}-{9}".format(*c))
def test_backoff_trigram_matches_the_yardstick(gtn, case):
    """the state depends on two labels: no table can say this.  Among the cases a unigram state with 70 arcs that are
    not contiguous, epsilon chains of 8, and a prefix that leaves the list and comes back with its state and its L"""
    got = _run_case(gtn, case)
    for b in range(case[1]):
        rows = [tuple(got[0][b, r, :got[1][b, r]]) for r in range(case[7]) if np.isfinite(got[2][b, r])]
        assert len(set(rows)) == len(rows), b


def test_constraints(gtn):
    """a lexicon-like acceptor without epsilon arcs: every returned sequence is one the numpy walk accepts (the search
    without it returns some that are not).  A start state without arcs forbids every label: no slot has a token, and
    only the empty prefix has a score -- the all-blank path's, as with a table whose start entries are all -inf"""
    B, T, C, blank, W, K, nbest = 3, 40, 12, 0, 16, 8, 4
    em = fp.continuous_case(5, B, T, C)
    G = gfp.lexicon_graph(5, C)
    got, _ = _decode(gtn, em, blank, W, K, nbest, lm=_lm(gtn, G))
    free, _ = _decode(gtn, em, blank, W, K, nbest)
    seqs = lambda out: [tuple(out[0][b, r, :out[1][b, r]]) for b in range(B) for r in range(nbest)
                        if np.isfinite(out[2][b, r])]
    assert np.isfinite(got[2][:, 0]).all() and any(len(y) > 1 for y in seqs(got))
    assert not all(gfp.accepts(G, y) for y in seqs(free)) and all(gfp.accepts(G, y) for y in seqs(got))
    closed = gfp.Arcs(2, 0, [(1, 1, c, 0.0) for c in range(C)])
    only, _ = _decode(gtn, em, blank, W, K, nbest, lm=_lm(gtn, closed))
    assert (only[0] == -1).all() and (only[1] == 0).all()
    assert np.isfinite(only[2][:, 0]).all() and np.isneginf(only[2][:, 1:]).all()
    assert only[2].tobytes() == only[3].tobytes()
    blanks = np.zeros(B, np.float32)
    for t in range(T):
        blanks = (blanks + em[:, t, blank]).astype(np.float32)
    assert only[2][:, 0].tobytes() == blanks.tobytes()
    # ... and where blank is not offered either nothing at all is left: -1 / 0 / -inf in every slot
    dead = em.copy()
    dead[:, 0, blank] = -np.inf
    none, _ = _decode(gtn, dead, blank, W, K, nbest, lm=_lm(gtn, closed))
    assert (none[0] == -1).all() and (none[1] == 0).all() and np.isneginf(none[2]).all() and np.isneginf(none[3]).all()


def test_mixed_frame_counts(gtn):
    """per-utterance lengths with 0 and T among them: the yardstick at each length; NaN in every pad row changes no bit
    of any output"""
    case = gfp.RAGGED_CASE
    seed, B, T, C, blank, W, K, nbest, fr, gkind = case
    got = _run_case(gtn, case)
    raw = _decode.raw
    em, G, _, _ = _want(case)
    poisoned = em.copy()
    for b in range(B):
        poisoned[b, fr[b]:] = np.nan
    _decode(gtn, poisoned, blank, W, K, nbest, lm=_lm(gtn, G), frames=list(fr))
    _same_bytes("pad rows", raw, _decode.raw)
    for b in range(B):
        if fr[b] == 0:
            assert (got[0][b] == -1).all() and (got[1][b] == 0).all()
            assert np.isneginf(got[2][b]).all() and np.isneginf(got[3][b]).all()


def test_unpruned_am_scores_are_ctc_score_on_the_device(gtn):
    """C = 4, T = 5, W = 64, K = C: no ancestor of a returned hypothesis is pruned (test_ctc_beam_graph_cpu.py checks it
    against the enumeration), so am_scores is torch_loss.ctc_score of the returned tokens, within the 1e-4 max(1,
    |score|) of test_ctc_beam_lm_gpu.py"""
    import torch
    from gtn_amd import torch_loss
    case = gfp.UNPRUNED_CASE
    seed, B, T, C, blank, W, K, nbest, _, _ = case
    assert T == 5 and C == 4 and W == 64 and K == C
    got = _run_case(gtn, case)
    x = _dev(_want(case)[0])
    try:
        ref = torch_loss.ctc_score(x, _dev(got[0]), _dev(got[1]), blank=blank)
        torch.cuda.synchronize()
        ref = ref.detach().cpu().numpy()
    finally:
        gtn.set_stream(None)
    assert ref.shape == (B, nbest)
    seen = 0
    for b in range(B):
        for r in range(nbest):
            if np.isfinite(got[3][b, r]):
                s = float(got[3][b, r])
                print(f"[ctc_beam_graph] unpruned b={b} r={r} am {s!r} ctc_score {float(ref[b, r])!r}")
                assert abs(s - float(ref[b, r])) <= 1e-4 * max(1.0, abs(s)), (b, r, s, float(ref[b, r]))
                seen += 1
    assert seen >= B


def test_refusals_leave_every_output_untouched(gtn):
    """a table and a graph together, a destroyed and a foreign handle, more than 2^19 labels, a weight that is not
    finite: ValueError, no output has changed and nothing was counted"""
    import torch
    from gtn_amd import torch_loss
    B, T, C = 3, 9, 8
    em = fp.continuous_case(83, B, T, C)
    G = gfp.backoff_bigram_graph(83, C)
    lm = _lm(gtn, G)
    c0 = gtn.debug_ctc_beam_stats()
    for alpha, beta in ((float("nan"), 0.0), (float("inf"), 0.0), (1.0, float("-inf"))):
        with pytest.raises(ValueError, match="must be finite"):
            _decode(gtn, em, 0, 4, 4, 2, alpha=alpha, beta=beta, lm=lm)
        assert _untouched()
    with pytest.raises(ValueError, match="nbest above beam_size"):
        _decode(gtn, em, 0, 4, 4, 5, lm=lm)
    assert _untouched()
    wide = np.zeros((1, 1, (1 << 19) + 1), np.float32)
    with pytest.raises(ValueError, match=r"more than 2\^19 labels"):
        _decode(gtn, wide, 0, 4, 4, 2, lm=lm)
    assert _untouched()
    x = _dev(em)
    try:
        with pytest.raises(ValueError, match="not both"):
            torch_loss.ctc_beam_decode(x, transitions=torch.zeros(C, C, device="cuda:0"), lm_graph=lm)
    finally:
        gtn.set_stream(None)
    foreign = ctypes.create_string_buffer(256)
    stale = _lm(gtn, G)
    gone = stale._h
    stale.destroy()
    with pytest.raises(ValueError, match="null LM graph handle"):
        _decode(gtn, em, 0, 4, 4, 2, lm=stale)
    assert _untouched()
    for handle in (gone, ctypes.addressof(foreign)):
        stale._h = handle
        try:
            with pytest.raises(ValueError, match="not a live LM graph handle"):
                _decode(gtn, em, 0, 4, 4, 2, lm=stale)
        finally:
            stale._h = None
        assert _untouched()
    assert gtn.debug_ctc_beam_stats() == c0
    got, stats = _decode(gtn, em, 0, 4, 4, 2, lm=lm)  # (the graph itself is fine)
    assert stats == (1, B) and np.isfinite(got[2][:, 0]).all()


def test_torch_entry_and_criteria_abi_equal_the_batch_route(gtn):
    """torch_loss.ctc_beam_decode(lm_graph=) gives the bytes of Batch.ctc_beam_decode(lm=LmGraph), three tensors unless
    return_am_scores; gtn_ctc_beam_decode_graph_n gives them too, am_scores null allowed"""
    import torch
    from gtn_amd import torch_loss
    case = gfp.TORCH_CASE
    seed, B, T, C, blank, W, K, nbest, frames, gkind = case
    em, G, want, err = _want(case)
    lm = _lm(gtn, G)
    x = _dev(em)
    kw = dict(blank=blank, beam_size=W, cutoff_top_n=K, nbest=nbest, lm_weight=lfp.ALPHA, insertion_bonus=lfp.BETA)
    try:
        c0 = gtn.debug_ctc_beam_stats()
        out4 = torch_loss.ctc_beam_decode(x, lm_graph=lm, return_am_scores=True, **kw)
        c1 = gtn.debug_ctc_beam_stats()
        out3 = torch_loss.ctc_beam_decode(x, lm_graph=lm, **kw)
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
    got, _ = _decode(gtn, em, blank, W, K, nbest, lm=lm, pad=0)
    for name, g, o in zip(NAMES, got, out4):
        assert g.tobytes() == o.tobytes(), name
    for g, o in zip(out4, out3):
        assert g.tobytes() == o.cpu().numpy().tobytes()
    # the criteria library's C entry
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    fn = lib.gtn_ctc_beam_decode_graph_n
    fn.argtypes = ([ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p]
                   + [ctypes.c_float] * 2 + [ctypes.c_void_p] * 4)
    fn.restype = ctypes.c_int
    lib.gtn_criteria_last_error.restype = ctypes.c_char_p
    tok = torch.full((B, nbest, T), SENTINEL, dtype=torch.int32, device="cuda:0")
    le = torch.full((B, nbest), SENTINEL, dtype=torch.int32, device="cuda:0")
    sc = torch.full((B, nbest), float("nan"), dtype=torch.float32, device="cuda:0")
    ams = torch.full((B, nbest), float("nan"), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rc = fn(x.data_ptr(), B, T, C, blank, None, W, K, nbest, lm._h, lfp.ALPHA, lfp.BETA, tok.data_ptr(), le.data_ptr(),
            sc.data_ptr(), ams.data_ptr())
    assert rc == 0, lib.gtn_criteria_last_error().decode()
    gtn.synchronize()
    for name, t, o in zip(NAMES, (tok, le, sc, ams), out4):
        assert t.cpu().numpy().tobytes() == o.tobytes(), name
    ams.fill_(float("nan"))
    torch.cuda.synchronize()
    rc = fn(x.data_ptr(), B, T, C, blank, None, W, K, nbest, lm._h, lfp.ALPHA, lfp.BETA, tok.data_ptr(), le.data_ptr(),
            sc.data_ptr(), None)
    assert rc == 0, lib.gtn_criteria_last_error().decode()
    gtn.synchronize()
    assert sc.cpu().numpy().tobytes() == out4[2].tobytes() and torch.isnan(ams).all()
    rc = fn(x.data_ptr(), B, T, C, blank, None, W, K, nbest, None, lfp.ALPHA, lfp.BETA, tok.data_ptr(), le.data_ptr(),
            sc.data_ptr(), None)
    assert rc == -1 and "null LM graph handle" in lib.gtn_criteria_last_error().decode()
