"""Batched CTC prefix beam search with a bigram table fused in (ctc_beam.hip, the LM instantiation of the search kernel,
through gtnx_batch_ctc_beam_decode_lm; gtn_amd.Batch.ctc_beam_decode(lm=...), gtn_amd.torch_loss.ctc_beam_decode(
transitions=...), gtn_ctc_beam_decode_lm_n).

The judge is the float64 yardstick of tests/ctc_beam_lm_fp.py, which tests/test_ctc_beam_lm_cpu.py pins to a brute-force
enumeration.  Tokens and lengths are compared with ==; that is sound because every case here vets on the host
(test_ctc_beam_lm_cpu.py::test_every_gpu_case_vets).  Both score kinds must be within 8 err of float64, err being the
case's host-side distance of the float32 forms from float64 over both kinds -- computed from the host forms, never from
the device.  The largest |device - float64| / err seen on an MI355X is in DESIGN section 23.

All four outputs have guards of sentinels that must survive, as in test_ctc_beam_gpu.py.
"""
import ctypes
import os

import numpy as np
import pytest

import ctc_beam_fp as fp
import ctc_beam_lm_fp as lfp

pytestmark = pytest.mark.gpu
SENTINEL = -7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tokens", "lengths", "scores", "am_scores")


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True, order="C")).to("cuda:0")  # (the cached cases are read-only)


def _decode(gtn, em, blank, W, K, nbest, w=None, alpha=lfp.ALPHA, beta=lfp.BETA, frames=None, rows=None, pad=1,
            address=False, lm=None, am=True):
    """Batch.ctc_beam_decode on Batch.linear with guarded outputs; w: the table as numpy (None: the call without one,
    three outputs), or `lm`: what to hand over in its place.  Returns the outputs as numpy and the (calls, utterances)
    this call counted; _decode.raw keeps the arrays with their guards, also when the call raised"""
    import torch
    B, T, C = em.shape
    em_dev = _dev(em)  # (borrowed by the batch: it must outlive the call)
    ems = gtn.Batch.linear(B, T, C, em_dev, False, True, rows)
    tok = torch.full((B + 2, nbest, T + pad), SENTINEL, dtype=torch.int32, device="cuda:0")
    ln = torch.full((B * nbest + 2,), SENTINEL, dtype=torch.int32, device="cuda:0")
    sc = torch.full((B * nbest + 2,), float("nan"), dtype=torch.float32, device="cuda:0")
    ams = torch.full((B * nbest + 2,), float("nan"), dtype=torch.float32, device="cuda:0")
    table = _dev(w) if w is not None else lm
    torch.cuda.synchronize()
    tv, lv, sv = tok[1:B + 1, :, :T], ln[1:B * nbest + 1].view(B, nbest), sc[1:B * nbest + 1].view(B, nbest)
    av = ams[1:B * nbest + 1].view(B, nbest)
    kw = {} if table is None else dict(lm=table, lm_weight=alpha, insertion_bonus=beta, am_scores_out=av if am else None)
    if address and kw.get("am_scores_out") is not None:
        kw["am_scores_out"] = av.data_ptr()
    c0 = gtn.debug_ctc_beam_stats()
    try:
        if address:
            ems.ctc_beam_decode(tv.data_ptr(), lv.data_ptr(), sv.data_ptr(), frames, blank, W, K, nbest,
                                row_stride=T + pad, **kw)
        else:
            ems.ctc_beam_decode(tv, lv, sv, frames, blank, W, K, nbest, **kw)
    finally:
        gtn.synchronize()
        c1 = gtn.debug_ctc_beam_stats()
        raw = [t.cpu().numpy() for t in (tok, ln, sc, ams)]
        _decode.raw = raw
        assert (raw[0][0] == SENTINEL).all() and (raw[0][B + 1] == SENTINEL).all(), "tokens: guard rows"
        assert (raw[0][:, :, T:] == SENTINEL).all(), "tokens: guard columns"
        assert raw[1][0] == SENTINEL and raw[1][-1] == SENTINEL, "lengths: guards"
        assert np.isnan(raw[2][0]) and np.isnan(raw[2][-1]), "scores: guards"
        assert np.isnan(raw[3][0]) and np.isnan(raw[3][-1]), "am_scores: guards"
        if table is None or not am:
            assert np.isnan(raw[3]).all(), "am_scores: not asked for"
    out = [raw[0][1:B + 1, :, :T], raw[1][1:-1].reshape(B, nbest), raw[2][1:-1].reshape(B, nbest),
           raw[3][1:-1].reshape(B, nbest)]
    return out, (c1[0] - c0[0], c1[1] - c0[1])


def _untouched():
    tok, ln, sc, ams = _decode.raw
    return (tok == SENTINEL).all() and (ln == SENTINEL).all() and np.isnan(sc).all() and np.isnan(ams).all()


def _want(case):
    """(em, w, the float64 outputs, err) of an entry of ctc_beam_lm_fp's case lists"""
    seed, B, T, C, blank, W, K, nbest, frames, holes = case
    em, w, res, _ = lfp.results_of(case)
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
    return em, w, (tokens, lengths, scores, am_scores), lfp.case_err_lm(res, nbest)


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
        print(f"[ctc_beam_lm] {tag} {name}: |device - float64| {dist:.3g}, err {err:.3g}, "
              f"ratio {dist / err if err else 0:.3g}")
        assert dist <= lfp.SCORE_FACTOR * err, (tag, name, dist, err)


def _run_case(gtn, case, **kw):
    seed, B, T, C, blank, W, K, nbest, frames, holes = case
    em, w, want, err = _want(case)
    got, stats = _decode(gtn, em, blank, W, K, nbest, w, frames=None if frames is None else list(frames), **kw)
    assert stats == (1, B)
    _check(str(case[:8]), got, want, err)
    return got


@pytest.mark.parametrize("case", lfp.SHAPE_CASES + lfp.RECREATED_CASES + [lfp.TORCH_CASE],
                         ids=lambda c: "B{1}-T{2}-C{3}-blank{4}-W{5}-K{6}-n{7}-seed{0}".format(*c))
def test_search_matches_the_yardstick(gtn, case):
    """the shapes of the issue (every lanes-per-row variant of the row kernel, T around the 64s, B = 1 .. 65, W = 2 ..
    64, K = 3 .. 32) and the cases where a prefix leaves the list and is created again with the same L"""
    got = _run_case(gtn, case)
    for b in range(case[1]):
        rows = [tuple(got[0][b, r, :got[1][b, r]]) for r in range(case[7]) if np.isfinite(got[2][b, r])]
        assert len(set(rows)) == len(rows), b


@pytest.mark.parametrize("address", [False, True])
def test_row_stride_above_T_and_no_am_scores(gtn, address):
    """rows 5 entries wider than T, as tensor views and as raw device addresses; without am_scores_out nothing is
    written there and the other three outputs are the same bits"""
    case = lfp.TORCH_CASE
    seed, B, T, C, blank, W, K, nbest, frames, holes = case
    _run_case(gtn, case, pad=5, address=address)
    raw = _decode.raw
    em, w, _, _ = _want(case)
    _decode(gtn, em, blank, W, K, nbest, w, pad=5, address=address, am=False)
    for name, r0, r1 in zip(NAMES[:3], raw, _decode.raw):
        assert r0.tobytes() == r1.tobytes(), name


def test_zero_weight_and_bonus_is_the_call_without_a_table(gtn):
    """alpha = beta = 0 with a finite table: every output byte-equal to the call without one, am_scores to scores"""
    for case in (fp.SHAPE_CASES[9], fp.SHAPE_CASES[10], fp.RAGGED_CASE, fp.RECREATED_CASES[0], fp.HOLES_CASE):
        kind, seed, B, T, C, blank, W, K, nbest, fr = case
        em = fp.results_of(case)[0]
        frames = None if fr is None else list(fr)
        _decode(gtn, em, blank, W, K, nbest, frames=frames)
        plain = _decode.raw
        _decode(gtn, em, blank, W, K, nbest, lfp.table_case(seed, C), 0.0, 0.0, frames=frames)
        for name, r0, r1 in zip(NAMES[:3], plain, _decode.raw):
            assert r0.tobytes() == r1.tobytes(), (case, name)
        assert _decode.raw[3][1:-1].tobytes() == _decode.raw[2][1:-1].tobytes(), case


def _forbidden(w, C, y):
    return (len(y) > 0 and np.isneginf(w[y[0]])) or any(np.isneginf(w[C + b * C + a]) for a, b in zip(y, y[1:]))


def test_constraints(gtn):
    """-inf entries are hard constraints: no returned sequence has a forbidden bigram or first label (the search
    without the table returns some); with every start entry -inf only the empty prefix comes back, with the all-blank
    path's score twice"""
    case = lfp.CONSTRAINED_CASE
    seed, B, T, C, blank, W, K, nbest, frames, holes = case
    em, w, _, _ = _want(case)
    got = _run_case(gtn, case)
    free, _ = _decode(gtn, em, blank, W, K, nbest)
    seqs = lambda out: [tuple(out[0][b, r, :out[1][b, r]]) for b in range(B) for r in range(nbest)]
    assert np.isfinite(got[2]).all()
    assert any(_forbidden(w, C, y) for y in seqs(free)) and not any(_forbidden(w, C, y) for y in seqs(got))
    closed = w.copy()
    closed[:C] = -np.inf
    only, _ = _decode(gtn, em, blank, W, K, nbest, closed)
    want = lfp.decode_batch_lm(em, None, blank, W, K, nbest, closed, lfp.ALPHA, lfp.BETA, "f32")
    assert (only[0] == -1).all() and (only[1] == 0).all()
    assert np.isfinite(only[2][:, 0]).all() and np.isneginf(only[2][:, 1:]).all()
    for name, g, x in zip(NAMES, only, want):  # (one path: a float32 sum in frame order, the same in both)
        assert g.tobytes() == x.tobytes(), name
    assert only[2].tobytes() == only[3].tobytes()
    blanks = np.zeros(B, np.float32)
    for t in range(T):
        blanks = (blanks + em[:, t, blank]).astype(np.float32)
    assert only[2][:, 0].tobytes() == blanks.tobytes()


def test_exact_ties(gtn):
    """integer-valued rows at T = 1, an integer-valued table, alpha = 1 and an integer beta: every total is exact, so
    equal totals are ordered stay first, then by rank and label -- all four outputs == the float32 host form"""
    for C, K, W, blank, beta in ((29, 3, 8, 0, 1.0), (65, 32, 64, 64, -2.0), (300, 16, 16, 7, 0.0), (3, 3, 4, 1, 1.0)):
        em = fp.integer_case(C, 65, 1, C)
        w = np.random.default_rng(C + 15000).integers(-2, 2, C + C * C).astype(np.float32)
        nbest = min(W, 4)
        want = lfp.decode_batch_lm(em, None, blank, W, K, nbest, w, 1.0, beta, "f32")
        got, _ = _decode(gtn, em, blank, W, K, nbest, w, 1.0, beta)
        for name, g, x in zip(NAMES, got, want):
            assert g.tobytes() == x.tobytes(), (C, name)


@pytest.mark.parametrize("mode", ["frames", "rows", "both"])
def test_mixed_frame_counts(gtn, mode):
    """per-utterance lengths (T, T - 1, 1 and 0 among them) through `frames`, through Batch.linear(rows=) and through
    both: the yardstick at each length; NaN in every pad row changes no bit of any output; in every mode each utterance
    equals the call on em[b, :T_b] alone, bit for bit"""
    case = lfp.RAGGED_ROWS_CASE if mode == "rows" else lfp.RAGGED_CASE
    seed, B, T, C, blank, W, K, nbest, fr, holes = case
    em, w, want, err = _want(case)
    rows = None if mode == "frames" else [max(f, 1) for f in fr] if mode == "both" else list(fr)
    frames = None if mode == "rows" else list(fr)
    got, stats = _decode(gtn, em, blank, W, K, nbest, w, frames=frames, rows=rows)
    assert stats == (1, B)
    _check(f"ragged {mode}", got, want, err)
    raw = _decode.raw
    poisoned = em.copy()
    for b in range(B):
        poisoned[b, fr[b]:] = np.nan
    _decode(gtn, poisoned, blank, W, K, nbest, w, frames=frames, rows=rows)
    for name, r0, r1 in zip(NAMES, raw, _decode.raw):
        assert r0.tobytes() == r1.tobytes(), name
    for b in range(B):
        if fr[b] == 0:
            assert (got[0][b] == -1).all() and (got[1][b] == 0).all()
            assert np.isneginf(got[2][b]).all() and np.isneginf(got[3][b]).all()
            continue
        alone, _ = _decode(gtn, em[b:b + 1, :fr[b]], blank, W, K, nbest, w)
        assert (got[0][b, :, :fr[b]] == alone[0][0]).all() and (got[0][b, :, fr[b]:] == -1).all(), b
        for k in (1, 2, 3):
            assert got[k][b].tobytes() == alone[k][0].tobytes(), (b, NAMES[k])


@pytest.mark.parametrize("case", lfp.UNPRUNED_CASES, ids=lambda c: "T{2}-C{3}-blank{4}".format(*c))
def test_unpruned_am_scores_are_ctc_score_on_the_device(gtn, case):
    """T <= 3, C <= 4, W = 64, K = C: nothing is pruned, so am_scores is torch_loss.ctc_score of the returned tokens,
    within the 1e-4 max(1, |score|) test_ctc_beam_gpu.py gives its unpruned scores"""
    import torch
    from gtn_amd import torch_loss
    seed, B, T, C, blank, W, K, nbest, _, _ = case
    assert T <= 3 and C <= 4 and W == 64 and K == C
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
                print(f"[ctc_beam_lm] unpruned b={b} r={r} am {s!r} ctc_score {float(ref[b, r])!r}")
                assert abs(s - float(ref[b, r])) <= 1e-4 * max(1.0, abs(s)), (b, r, s, float(ref[b, r]))
                seen += 1
    assert seen >= B


def test_refusals_leave_every_output_untouched(gtn):
    """a table in host memory, a weight that is not finite, a null table through the _lm entry: ValueError, and no
    output has changed"""
    import torch
    B, T, C = 3, 9, 8
    em = fp.continuous_case(83, B, T, C)
    w = lfp.table_case(83, C)
    c0 = gtn.debug_ctc_beam_stats()
    with pytest.raises(ValueError, match="language model table is not memory"):
        _decode(gtn, em, 0, 4, 4, 2, lm=w.ctypes.data, address=True)  # (pageable host memory, by its address)
    assert _untouched()
    with pytest.raises(ValueError, match="lm must be a float32"):
        _decode(gtn, em, 0, 4, 4, 2, lm=torch.from_numpy(w.copy()))  # (a tensor that is not on the device)
    assert _untouched()
    for alpha, beta in ((float("nan"), 0.0), (float("inf"), 0.0), (1.0, float("-inf"))):
        with pytest.raises(ValueError, match="must be finite"):
            _decode(gtn, em, 0, 4, 4, 2, w, alpha, beta)
        assert _untouched()
    with pytest.raises(ValueError, match="null language model table"):
        _decode(gtn, em, 0, 4, 4, 2, lm=0, address=True)
    assert _untouched()
    with pytest.raises(ValueError, match="lm has 71 entries"):
        _decode(gtn, em, 0, 4, 4, 2, w[:-1])
    assert _untouched()
    with pytest.raises(ValueError, match="nbest above beam_size"):
        _decode(gtn, em, 0, 4, 4, 5, w)
    assert _untouched()
    assert gtn.debug_ctc_beam_stats() == c0


def test_torch_entry_equals_the_batch_route(gtn):
    """torch_loss.ctc_beam_decode(transitions=, start=) on a non-contiguous transitions that requires grad: the bits of
    Batch.ctc_beam_decode(lm=_asg_weights(start, transitions)); three tensors unless return_am_scores; start defaults
    to zeros; transitions=None is the call without a table"""
    import torch
    from gtn_amd import torch_loss
    case = lfp.TORCH_CASE
    seed, B, T, C, blank, W, K, nbest, frames, holes = case
    em, w, want, err = _want(case)
    x = _dev(em)
    big = torch.zeros(C, 2 * C, device="cuda:0")
    big[:, ::2] = _dev(w[C:].reshape(C, C))
    tr = big[:, ::2].requires_grad_(True)
    start = _dev(w[:C]).requires_grad_(True)
    assert not tr.is_contiguous()
    kw = dict(blank=blank, beam_size=W, cutoff_top_n=K, nbest=nbest, lm_weight=lfp.ALPHA, insertion_bonus=lfp.BETA)
    try:
        c0 = gtn.debug_ctc_beam_stats()
        out4 = torch_loss.ctc_beam_decode(x, transitions=tr, start=start, return_am_scores=True, **kw)
        c1 = gtn.debug_ctc_beam_stats()
        out3 = torch_loss.ctc_beam_decode(x, transitions=tr, start=start, **kw)
        nostart = torch_loss.ctc_beam_decode(x, transitions=tr, return_am_scores=True, **kw)
        plain = torch_loss.ctc_beam_decode(x, blank=blank, beam_size=W, cutoff_top_n=K, nbest=nbest)
        plain_kw = torch_loss.ctc_beam_decode(x, blank=blank, beam_size=W, cutoff_top_n=K, nbest=nbest, transitions=None)
        torch.cuda.synchronize()
    finally:
        gtn.set_stream(None)
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, B)
    assert len(out4) == 4 and len(out3) == 3 and len(plain) == 3 and len(plain_kw) == 3
    kinds = ((torch.int32, (B, nbest, T)), (torch.int32, (B, nbest)), (torch.float32, (B, nbest)),
             (torch.float32, (B, nbest)))
    for o, (dt, shape) in zip(out4, kinds):
        assert o.dtype == dt and o.shape == shape and o.device == x.device and not o.requires_grad
    out4 = [o.cpu().numpy() for o in out4]
    _check("torch", out4, want, err)
    got, _ = _decode(gtn, em, blank, W, K, nbest, w, pad=0)
    for name, g, o in zip(NAMES, got, out4):
        assert g.tobytes() == o.tobytes(), name
    for g, o in zip(out4, out3):
        assert g.tobytes() == o.cpu().numpy().tobytes()
    for a, b in zip(plain, plain_kw):
        assert torch.equal(a, b)
    w0 = w.copy()
    w0[:C] = 0.0
    got0, _ = _decode(gtn, em, blank, W, K, nbest, w0, pad=0)
    for name, g, o in zip(NAMES, got0, nostart):
        assert g.tobytes() == o.cpu().numpy().tobytes(), name


def test_criteria_abi(gtn):
    """gtn_ctc_beam_decode_lm_n gives the four tensors the Batch API gives; am_scores may be null"""
    import torch
    case = lfp.TORCH_CASE
    seed, B, T, C, blank, W, K, nbest, frames, holes = case
    em, w, want, err = _want(case)
    em_dev, w_dev = _dev(em), _dev(w)
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    fn = lib.gtn_ctc_beam_decode_lm_n
    fn.argtypes = ([ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p]
                   + [ctypes.c_float] * 2 + [ctypes.c_void_p] * 4)
    fn.restype = ctypes.c_int
    lib.gtn_criteria_last_error.restype = ctypes.c_char_p
    tok = torch.full((B, nbest, T), SENTINEL, dtype=torch.int32, device="cuda:0")
    le = torch.full((B, nbest), SENTINEL, dtype=torch.int32, device="cuda:0")
    sc = torch.full((B, nbest), float("nan"), dtype=torch.float32, device="cuda:0")
    ams = torch.full((B, nbest), float("nan"), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rc = fn(em_dev.data_ptr(), B, T, C, blank, None, W, K, nbest, w_dev.data_ptr(), lfp.ALPHA, lfp.BETA, tok.data_ptr(),
            le.data_ptr(), sc.data_ptr(), ams.data_ptr())
    assert rc == 0, lib.gtn_criteria_last_error().decode()
    gtn.synchronize()
    _check("abi", [t.cpu().numpy() for t in (tok, le, sc, ams)], want, err)
    first = sc.cpu().numpy().tobytes()
    rc = fn(em_dev.data_ptr(), B, T, C, blank, None, W, K, nbest, w_dev.data_ptr(), lfp.ALPHA, lfp.BETA, tok.data_ptr(),
            le.data_ptr(), sc.data_ptr(), None)
    assert rc == 0, lib.gtn_criteria_last_error().decode()
    gtn.synchronize()
    assert sc.cpu().numpy().tobytes() == first
    rc = fn(em_dev.data_ptr(), B, T, C, blank, None, W, K, nbest, None, lfp.ALPHA, lfp.BETA, tok.data_ptr(),
            le.data_ptr(), sc.data_ptr(), None)
    assert rc == -1 and "null language model table" in lib.gtn_criteria_last_error().decode()
