"""Batched ASG prefix beam search with N-best output (asg_beam.hip through gtnx_batch_asg_beam_decode;
gtn_amd.Batch.asg_beam_decode, gtn_amd.torch_loss.asg_beam_decode, gtn_asg_beam_decode_n).

The judge is the float64 yardstick of tests/asg_beam_fp.py, which tests/test_asg_beam_cpu.py pins to a brute-force
enumeration, to the oracle and to asg_score's yardstick.  Tokens and lengths are compared with ==; that is sound because
every case here vets on the host (test_asg_beam_cpu.py::test_every_gpu_case_vets).  Scores must be within SCORE_FACTOR
(8) times err of float64, err being the case's host-side distance of the float32 forms from float64 -- computed from the
host forms, never from the device: the rule and the constants of test_ctc_beam_gpu.py.  The largest |device - float64| /
err seen on an MI355X is in DESIGN section 27.

Every output sits between guards of sentinels that must survive: rows and columns around the tokens, elements around
lengths and scores.
"""
import ctypes
import os

import numpy as np
import pytest

import asg_beam_fp as fp

pytestmark = pytest.mark.gpu
SENTINEL = -7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tokens", "lengths", "scores")


def _ids(c):
    return "B{2}-T{3}-C{4}-W{5}-K{6}-n{7}-seed{1}".format(*c)


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True, order="C")).to("cuda:0")  # (the cached cases are read-only)


def _decode(gtn, em, table, W, K, nbest, frames=None, rows=None, pad=1, address=False, raw_table=None, batch=None):
    """Batch.asg_beam_decode on Batch.linear with guarded outputs; table: numpy (or `raw_table`: what to hand over in its
    place).  Returns the outputs as numpy and the (calls, utterances) this call counted; _decode.raw keeps the arrays
    with their guards, also when the call raised"""
    import torch
    B, T, C = em.shape
    em_dev = _dev(em)  # (borrowed by the batch: it must outlive the call)
    ems = batch if batch is not None else gtn.Batch.linear(B, T, C, em_dev, False, True, rows)
    tok = torch.full((B + 2, nbest, T + pad), SENTINEL, dtype=torch.int32, device="cuda:0")
    ln = torch.full((B * nbest + 2,), SENTINEL, dtype=torch.int32, device="cuda:0")
    sc = torch.full((B * nbest + 2,), float("nan"), dtype=torch.float32, device="cuda:0")
    tab = _dev(table) if raw_table is None else raw_table
    torch.cuda.synchronize()
    tv, lv, sv = tok[1:B + 1, :, :T], ln[1:B * nbest + 1].view(B, nbest), sc[1:B * nbest + 1].view(B, nbest)
    c0 = gtn.debug_asg_beam_stats()
    try:
        if address:
            ems.asg_beam_decode(tv.data_ptr(), lv.data_ptr(), sv.data_ptr(), frames,
                                tab.data_ptr() if hasattr(tab, "data_ptr") else tab, W, K, nbest, row_stride=T + pad)
        else:
            ems.asg_beam_decode(tv, lv, sv, frames, tab, W, K, nbest)
    finally:
        gtn.synchronize()
        c1 = gtn.debug_asg_beam_stats()
        raw = [t.cpu().numpy() for t in (tok, ln, sc)]
        _decode.raw = raw
        assert (raw[0][0] == SENTINEL).all() and (raw[0][B + 1] == SENTINEL).all(), "tokens: guard rows"
        assert (raw[0][:, :, T:] == SENTINEL).all(), "tokens: guard columns"
        assert raw[1][0] == SENTINEL and raw[1][-1] == SENTINEL, "lengths: guards"
        assert np.isnan(raw[2][0]) and np.isnan(raw[2][-1]), "scores: guards"
    out = [raw[0][1:B + 1, :, :T], raw[1][1:-1].reshape(B, nbest), raw[2][1:-1].reshape(B, nbest)]
    return out, (c1[0] - c0[0], c1[1] - c0[1])


def _untouched():
    tok, ln, sc = _decode.raw
    return (tok == SENTINEL).all() and (ln == SENTINEL).all() and np.isnan(sc).all()


def _want(case):
    """(em, table, the float64 outputs, err) of an entry of asg_beam_fp's case lists"""
    kind, seed, B, T, C, W, K, nbest, frames, holes = case
    em, table, res, _ = fp.results_of(case)
    return em, table, fp.rows_of(res["f64"], T, nbest), fp.case_err(res, nbest)


WORST = {"ratio": 0.0}


def _check(tag, got, want, err):
    """tokens and lengths == the float64 yardstick; scores within 8 err of it (-inf where it is -inf)"""
    for name, g, w in zip(NAMES[:2], got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (tag, name, bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
    g, w = got[2], want[2]
    assert g.dtype == np.float32 and g.shape == w.shape and not np.isnan(g).any(), tag
    dead = np.isneginf(w)
    assert (np.isneginf(g) == dead).all(), (tag, g, w)
    dist = float(np.abs(g[~dead].astype(np.float64) - w[~dead]).max()) if (~dead).any() else 0.0
    ratio = dist / err if err else 0.0
    WORST["ratio"] = max(WORST["ratio"], ratio)
    print(f"[asg_beam] {tag}: |device - float64| {dist:.3g}, err {err:.3g}, ratio {ratio:.3g}, "
          f"largest ratio so far {WORST['ratio']:.3g}")
    assert dist <= fp.SCORE_FACTOR * err, (tag, dist, err)


def _run_case(gtn, case, **kw):
    kind, seed, B, T, C, W, K, nbest, frames, holes = case
    em, table, want, err = _want(case)
    got, stats = _decode(gtn, em, table, W, K, nbest, frames=None if frames is None else list(frames), **kw)
    assert stats == (1, B)
    _check(str(case[:8]), got, want, err)
    return got


def _no_row_twice(got, case):
    for b in range(case[2]):
        rows = [tuple(got[0][b, r, :got[1][b, r]]) for r in range(case[7]) if np.isfinite(got[2][b, r])]
        assert len(set(rows)) == len(rows), b
        for y in rows:
            assert all(a != c for a, c in zip(y, y[1:])), (b, y)  # (no equal neighbours)


@pytest.mark.parametrize("case", fp.SHAPE_CASES + [fp.REPEAT_CASE], ids=_ids)
def test_search_matches_the_yardstick(gtn, case):
    """the shapes of the issue: C at every head, tail and lanes-per-row variant of the row kernel, C <= K, T around the
    64s, B = 1, 2, 65, W = 1 .. 64, K = 1 and 32, nbest = 1, 2, 4 (nbest = W at T <= 3)"""
    _no_row_twice(_run_case(gtn, case), case)


@pytest.mark.parametrize("case", fp.RECREATED_CASES, ids=_ids)
def test_recreated_prefixes_are_recognised(gtn, case):
    """a prefix that left the list and was created again is still the parent of its child that stayed: the yardstick's
    hypotheses, and no token row twice among the finite slots"""
    _no_row_twice(_run_case(gtn, case), case)


def test_one_label_per_frame_is_exact(gtn):
    """K = 1: no log-add anywhere, so tokens, lengths AND scores equal the float32 host form with =="""
    for case in (fp.K1_CASE, fp.SHAPE_CASES[3]):
        kind, seed, B, T, C, W, K, nbest, frames, holes = case
        assert K == 1
        em, table, _, _ = fp.results_of(case)
        want = fp.decode_batch(em, table, None, W, K, nbest, "f32")
        got, _ = _decode(gtn, em, table, W, K, nbest)
        for name, g, x in zip(NAMES, got, want):
            assert g.dtype == x.dtype and (g == x).all(), (case, name)
        assert np.isfinite(got[2][:, 0]).all() and np.isneginf(got[2][:, 1:]).all()


def test_exact_ties(gtn):
    """integer-valued rows and an integer-valued table at T = 1: every total is exact; top-K ties go to the smaller
    label, equal totals are ordered by parent rank, then label -- all three outputs == the float32 host form"""
    for C, K, W in ((29, 3, 8), (65, 32, 64), (300, 16, 16), (3, 3, 4), (5, 32, 2)):
        em = fp.integer_case(C, 65, 1, C)
        table = np.random.default_rng(C + 15000).integers(-2, 2, C + C * C).astype(np.float32)
        nbest = min(W, 4)
        want = fp.decode_batch(em, table, None, W, K, nbest, "f32")
        got, _ = _decode(gtn, em, table, W, K, nbest)
        for name, g, x in zip(NAMES, got, want):
            assert g.tobytes() == x.tobytes(), (C, name)
        # (ties are there: some utterance has two equal totals among its first two)
        assert any(want[2][b, 0] == want[2][b, 1] for b in range(65)), C


@pytest.mark.parametrize("case", fp.UNPRUNED_CASES, ids=_ids)
def test_unpruned_is_the_enumeration_and_asg_score(gtn, case):
    """T <= 3, C <= 4, W = 64, K = C: nothing is pruned.  Asked for all 64 slots, every hypothesis of the enumeration
    appears once, and each score is within 8 err of Batch.asg_score of the returned tokens, run on the device from the
    returned tensors"""
    import torch
    kind, seed, B, T, C, W, K, nbest, _, _ = case
    assert T <= 3 and C <= 4 and W == 64 and K == C
    _run_case(gtn, case)
    em, table, res, _ = fp.results_of(case)
    err = fp.case_err(res, 64)
    x, tab = _dev(em), _dev(table)
    ems = gtn.Batch.linear(B, T, C, x, False, True)
    tok = torch.full((B, 64, T), SENTINEL, dtype=torch.int32, device="cuda:0")
    ln = torch.full((B, 64), SENTINEL, dtype=torch.int32, device="cuda:0")
    sc = torch.full((B, 64), float("nan"), dtype=torch.float32, device="cuda:0")
    ref = torch.full((B, 64), float("nan"), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ems.asg_beam_decode(tok, ln, sc, None, tab, 64, K, 64)
    ems.asg_score(tab, tok, ln, ref, max_length=T)
    gtn.synchronize()
    tok, ln, sc, ref = (t.cpu().numpy() for t in (tok, ln, sc, ref))
    for b in range(B):
        want = fp.brute_force(em[b], table)
        assert len(want) <= 52
        rows = [tuple(tok[b, r, :ln[b, r]]) for r in range(64) if np.isfinite(sc[b, r])]
        assert sorted(rows) == sorted(want), b
        assert np.isneginf(sc[b, len(rows):]).all() and (ln[b, len(rows):] == 0).all() and (tok[b, len(rows):] == -1).all()
        for r, y in enumerate(rows):
            d_ref, d_64 = abs(float(sc[b, r]) - float(ref[b, r])), abs(float(sc[b, r]) - want[y])
            print(f"[asg_beam] unpruned b={b} r={r}: |beam - asg_score| {d_ref:.3g}, |beam - float64| {d_64:.3g}, "
                  f"err {err:.3g}")
            assert d_ref <= fp.SCORE_FACTOR * err, (b, r, d_ref, err)
            assert d_64 <= fp.SCORE_FACTOR * err, (b, r, d_64, err)


@pytest.mark.parametrize("mode", ["frames", "rows"])
def test_mixed_frame_counts(gtn, mode):
    """per-utterance lengths (T, T - 1, 1 and 0 among them) through `frames` and through Batch.linear(rows=): the
    yardstick at each length; NaN, +inf or other finite values in the pad rows change no bit of any output; T_b == 0
    gives -1 / 0 / -inf"""
    case = fp.RAGGED_ROWS_CASE if mode == "rows" else fp.RAGGED_CASE
    kind, seed, B, T, C, W, K, nbest, fr, holes = case
    em, table, want, err = _want(case)
    rows = list(fr) if mode == "rows" else None
    frames = None if mode == "rows" else list(fr)
    got, stats = _decode(gtn, em, table, W, K, nbest, frames=frames, rows=rows)
    assert stats == (1, B)
    _check(f"ragged {mode}", got, want, err)
    raw = _decode.raw
    for fill in (np.nan, np.inf, 3.5):
        poisoned = em.copy()
        for b in range(B):
            poisoned[b, fr[b]:] = fill
        _decode(gtn, poisoned, table, W, K, nbest, frames=frames, rows=rows)
        for name, r0, r1 in zip(NAMES, raw, _decode.raw):
            assert r0.tobytes() == r1.tobytes(), (name, fill)
    for b in range(B):
        if fr[b] == 0:
            assert (got[0][b] == -1).all() and (got[1][b] == 0).all() and np.isneginf(got[2][b]).all()
    if mode == "frames":
        assert 0 in fr and T in fr and T - 1 in fr and 1 in fr


def test_holes_in_the_emissions(gtn):
    """-inf and NaN emissions: never chosen; the all--inf row kills utterance 1 and no other"""
    case = fp.HOLES_CASE
    got = _run_case(gtn, case)
    assert (got[0][1] == -1).all() and (got[1][1] == 0).all() and np.isneginf(got[2][1]).all()
    for b in (0, 2, 3):
        assert np.isfinite(got[2][b]).all() and (got[1][b] > 0).all()


@pytest.mark.parametrize("case", [fp.CONSTRAINED_CASE, fp.NAN_TABLE_CASE], ids=["minus-inf", "nan"])
def test_holes_in_the_table(gtn, case):
    """-inf table entries forbid a bigram and a first label, NaN entries drop their candidates alike and no NaN reaches
    any output: the yardstick's hypotheses, none of them forbidden, where the search on the table without the holes
    returns a forbidden first label and a forbidden bigram; with every start entry -inf nothing comes back"""
    kind, seed, B, T, C, W, K, nbest, frames, holes = case
    em, table, _, _ = _want(case)
    assert not np.isfinite(table[:C]).all() and not np.isfinite(table[C:]).all()
    got = _run_case(gtn, case)
    free, _ = _decode(gtn, em, fp.table_case(seed, C), W, K, nbest)
    seqs = lambda out: [tuple(out[0][b, r, :out[1][b, r]]) for b in range(B) for r in range(nbest)]
    assert np.isfinite(got[2]).all()
    assert any(fp.forbidden_first(table, y) for y in seqs(free)) and any(fp.forbidden_bigram(table, C, y) for y in seqs(free))
    assert not any(fp.forbidden_first(table, y) or fp.forbidden_bigram(table, C, y) for y in seqs(got))
    closed = table.copy()
    closed[:C] = -np.inf
    none, stats = _decode(gtn, em, closed, W, K, nbest)
    assert stats == (1, B)
    assert (none[0] == -1).all() and (none[1] == 0).all() and np.isneginf(none[2]).all()


def test_two_runs_give_the_same_bits(gtn):
    for case in (fp.REPEAT_CASE, fp.SHAPE_CASES[9]):
        kind, seed, B, T, C, W, K, nbest, frames, holes = case
        em, table, _, _ = _want(case)
        _decode(gtn, em, table, W, K, nbest)
        first = _decode.raw
        _decode(gtn, em, table, W, K, nbest)
        for name, r0, r1 in zip(NAMES, first, _decode.raw):
            assert r0.tobytes() == r1.tobytes(), (case, name)


@pytest.mark.parametrize("address", [False, True])
def test_row_stride_above_M(gtn, address):
    """rows 5 entries wider than M, as tensor views and as raw device addresses: the same bits as dense rows"""
    case = fp.TORCH_CASES[0]
    kind, seed, B, T, C, W, K, nbest, frames, holes = case
    wide = _run_case(gtn, case, pad=5, address=address)
    em, table, _, _ = _want(case)
    dense, stats = _decode(gtn, em, table, W, K, nbest, pad=0)
    assert stats == (1, B)
    for name, g, d in zip(NAMES, wide, dense):
        assert g.tobytes() == d.tobytes(), name


def test_refusals_leave_every_output_untouched(gtn):
    """every refusal that needs the device: ValueError with its text, the guards and the outputs untouched, nothing
    counted"""
    import torch
    B, T, C = 3, 9, 8
    em = fp.continuous_case(83, B, T, C)
    table = fp.table_case(83, C)
    c0 = gtn.debug_asg_beam_stats()
    graphs = gtn.Batch([gtn.linear_graph(T, C) for _ in range(B)])
    with pytest.raises(ValueError, match="not a native linear batch"):
        _decode(gtn, em, table, 4, 4, 2, batch=graphs, address=True)
    assert _untouched()
    for frames, msg in (([T + 1, 1, 1], "a frame count outside 0 .. M"), ([-1, 1, 1], "a frame count outside 0 .. M")):
        with pytest.raises(ValueError, match=msg):
            _decode(gtn, em, table, 4, 4, 2, frames=frames)
        assert _untouched()
    with pytest.raises(ValueError, match="a frame count beyond the rows the batch carries"):
        _decode(gtn, em, table, 4, 4, 2, frames=[T, T, T], rows=[T, T - 1, T])
    assert _untouched()
    with pytest.raises(ValueError, match="row_stride is shorter than the rows of the batch"):
        _decode(gtn, em, table, 4, 4, 2, pad=-1, address=True)
    assert _untouched()
    with pytest.raises(ValueError, match="the table is not memory of the engine's current device"):
        _decode(gtn, em, table, 4, 4, 2, raw_table=table.ctypes.data, address=True)  # (pageable host memory)
    assert _untouched()
    with pytest.raises(ValueError, match="table must be a float32 contiguous CUDA tensor"):
        _decode(gtn, em, table, 4, 4, 2, raw_table=torch.from_numpy(table.copy()))
    assert _untouched()
    with pytest.raises(ValueError, match="table has 71 entries"):
        _decode(gtn, em, table[:-1], 4, 4, 2)
    assert _untouched()
    with pytest.raises(ValueError, match="nbest outside 1 .. beam_size"):
        _decode(gtn, em, table, 4, 4, 5)
    assert _untouched()
    if torch.cuda.device_count() > 1:  # outputs the device may not write: memory of another GPU of the process
        x, tab = _dev(em), _dev(table)
        ems = gtn.Batch.linear(B, T, C, x, False, True)
        tok = torch.full((B, 2, T), SENTINEL, dtype=torch.int32, device="cuda:0")
        sc = torch.full((B, 2), float("nan"), dtype=torch.float32, device="cuda:0")
        other = torch.full((B, 2), SENTINEL, dtype=torch.int32, device="cuda:1")
        with pytest.raises(ValueError, match="an output pointer is not memory"):
            ems.asg_beam_decode(tok, other.data_ptr(), sc, None, tab, 4, 4, 2)
        gtn.synchronize()
        assert (tok == SENTINEL).all() and sc.isnan().all() and (other == SENTINEL).all()
    assert gtn.debug_asg_beam_stats() == c0


def test_shapes_beyond_the_trie_and_the_key_are_refused(gtn):
    """M * beam_size must fit an int (a one-label batch of 2^25 rows at beam_size 64) and a label must fit the key's 19
    bits (one row of 2^19 + 1 labels): refused by the shapes, lengths and scores untouched, nothing counted"""
    import torch
    ln = torch.full((4,), SENTINEL, dtype=torch.int32, device="cuda:0")
    sc = torch.full((4,), float("nan"), dtype=torch.float32, device="cuda:0")
    tok = torch.full((4, 1), SENTINEL, dtype=torch.int32, device="cuda:0")
    tab = torch.zeros(2, device="cuda:0")
    c0 = gtn.debug_asg_beam_stats()
    M = 1 << 25
    x = torch.zeros(1, M, 1, device="cuda:0")
    ems = gtn.Batch.linear(1, M, 1, x, False, True)
    with pytest.raises(ValueError, match="rows times beam_size does not fit an int"):
        ems.asg_beam_decode(tok.data_ptr(), ln[1:], sc[1:], None, tab, 64, 1, 1, row_stride=M)
    C = (1 << 19) + 1
    x = torch.zeros(1, 1, C, device="cuda:0")
    ems = gtn.Batch.linear(1, 1, C, x, False, True)
    with pytest.raises(ValueError, match="more than 2\\^19 labels"):
        ems.asg_beam_decode(tok[1:2].data_ptr(), ln[1:], sc[1:], None, tab.data_ptr(), 4, 4, 1, row_stride=1)
    gtn.synchronize()
    assert (ln == SENTINEL).all() and sc.isnan().all() and (tok == SENTINEL).all()
    assert gtn.debug_asg_beam_stats() == c0


@pytest.mark.parametrize("case", fp.TORCH_CASES, ids=_ids)
def test_torch_entry(gtn, case):
    """torch_loss.asg_beam_decode: the bits of the batch call (transitions non-contiguous and requiring grad, start
    given or defaulting to zeros), input_lengths with a 0 among them, and its outputs feed torch_loss.asg_score and
    torch_loss.edit_distance as they are"""
    import torch
    from gtn_amd import torch_loss
    kind, seed, B, T, C, W, K, nbest, frames, holes = case
    em, table, want, err = _want(case)
    x = _dev(em)
    big = torch.zeros(C, 2 * C, device="cuda:0")
    big[:, ::2] = _dev(table[C:].reshape(C, C))
    tr = big[:, ::2].requires_grad_(True)
    start = _dev(table[:C]).requires_grad_(True)
    assert not tr.is_contiguous()
    lengths_in = None if frames is None else list(frames)
    kw = dict(input_lengths=lengths_in, beam_size=W, cutoff_top_n=K, nbest=nbest)
    try:
        c0 = gtn.debug_asg_beam_stats()
        out = torch_loss.asg_beam_decode(x, tr, start, **kw)
        c1 = gtn.debug_asg_beam_stats()
        nostart = torch_loss.asg_beam_decode(x, tr, **kw)
        rescored = torch_loss.asg_score(x, tr, out[0], out[1], start=start, input_lengths=lengths_in)
        ref = torch.zeros(B, 3, dtype=torch.int32, device="cuda:0")
        ref_len = torch.full((B,), 3, dtype=torch.int32, device="cuda:0")
        dist = torch_loss.edit_distance(out[0], out[1], ref, ref_len)
        torch.cuda.synchronize()
    finally:
        gtn.set_stream(None)
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, B)
    kinds = ((torch.int32, (B, nbest, T)), (torch.int32, (B, nbest)), (torch.float32, (B, nbest)))
    for o, (dt, shape) in zip(out, kinds):
        assert o.dtype == dt and o.shape == shape and o.device == x.device and not o.requires_grad
    got = [o.cpu().numpy() for o in out]
    _check("torch", got, want, err)
    direct, _ = _decode(gtn, em, table, W, K, nbest, frames=lengths_in, pad=0)
    for name, g, o in zip(NAMES, direct, got):
        assert g.tobytes() == o.tobytes(), name
    t0 = table.copy()
    t0[:C] = 0.0
    direct0, _ = _decode(gtn, em, t0, W, K, nbest, frames=lengths_in, pad=0)
    for name, g, o in zip(NAMES, direct0, nostart):
        assert g.tobytes() == o.cpu().numpy().tobytes(), name
    if frames is not None:
        b0 = list(frames).index(0)
        assert (got[0][b0] == -1).all() and (got[1][b0] == 0).all() and np.isneginf(got[2][b0]).all()
    # the chain: the rescored rows are finite where the beam's are, and the distances are those of the lengths' rows
    rescored, dist = rescored.detach().cpu().numpy(), dist.cpu().numpy()
    live = np.isfinite(got[2])
    assert rescored.shape == (B, nbest) and np.isfinite(rescored[live]).all()
    assert (rescored[live] >= got[2][live] - 1e-3 * np.maximum(1.0, np.abs(got[2][live]))).all()  # (pruning only loses mass)
    assert dist.shape == (B, nbest) and (dist >= 0).all()
    for b in range(B):
        for r in range(nbest):
            y = got[0][b, r, :got[1][b, r]]
            assert dist[b, r] == max(len(y), 3) - min(3, int((y == 0).sum())), (b, r)


def test_criteria_abi(gtn):
    """gtn_asg_beam_decode_n gives the three tensors the Batch API gives"""
    import torch
    case = fp.TORCH_CASES[0]
    kind, seed, B, T, C, W, K, nbest, frames, holes = case
    em, table, want, err = _want(case)
    em_dev, w_dev = _dev(em), _dev(table)
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    fn = lib.gtn_asg_beam_decode_n
    fn.argtypes = ([ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3
                   + [ctypes.c_void_p] * 3)
    fn.restype = ctypes.c_int
    lib.gtn_criteria_last_error.restype = ctypes.c_char_p
    tok = torch.full((B, nbest, T), SENTINEL, dtype=torch.int32, device="cuda:0")
    le = torch.full((B, nbest), SENTINEL, dtype=torch.int32, device="cuda:0")
    sc = torch.full((B, nbest), float("nan"), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rc = fn(em_dev.data_ptr(), B, T, C, w_dev.data_ptr(), None, W, K, nbest, tok.data_ptr(), le.data_ptr(), sc.data_ptr())
    assert rc == 0, lib.gtn_criteria_last_error().decode()
    gtn.synchronize()
    _check("abi", [t.cpu().numpy() for t in (tok, le, sc)], want, err)
    rc = fn(em_dev.data_ptr(), B, T, C, None, None, W, K, nbest, tok.data_ptr(), le.data_ptr(), sc.data_ptr())
    assert rc == -1 and "null table pointer" in lib.gtn_criteria_last_error().decode()
