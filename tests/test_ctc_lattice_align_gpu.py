"""Batched CTC Viterbi alignment of device-resident token lattices (ctc_lattice_align.hip through
gtnx_batch_ctc_lattice_align; gtn_amd.torch_loss.ctc_lattice_align, Batch.ctc_lattice_align, gtn_ctc_lattice_align_n).

The judge is the float32 transcription of tests/ctc_lattice_align_fp.py, which tests/test_ctc_lattice_align_cpu.py pins
to an enumeration of the lattice's paths, to the oracle and to ctc_token_align_fp.  The contract makes
every output reproducible bit for bit, so every comparison is of bits: scores, path lengths, the four path rows, the
token scores and the frame rows, fills included; the rows handed over are wider than P and M and lie between guard words,
and nothing outside the widths may change.  The cases are those of ctc_lattice_fp (both sides of every width of
ctc_lattice_config, in-degrees 0 to 511, the deep lattice, ragged frame counts, invalid lattices beside valid ones) and
the tie cases packed into one batch."""
import numpy as np
import pytest

import ctc_lattice_align_fp as fp
import ctc_lattice_fp as lfp
import ctc_token_align_fp as tfp

pytestmark = pytest.mark.gpu
NEG = -np.inf
GUARD_I, GUARD_F = 77, 5.0


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True, order="C")).to("cuda:0")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    """two Results (or tuples of arrays, None for an output not asked for) have the same bits"""
    for x, y in zip(a, b):
        if x is None or y is None:
            if not (x is None and y is None):
                return False
        elif not (x.shape == y.shape and x.dtype == y.dtype and (_bits(x) == _bits(y)).all()):
            return False
    return True


def _run(gtn, case, P=None, token_scores=True, frame_arcs=True, arcs=None, row_pad=0, out_pad=3, frame_pad=5):
    """Batch.ctc_lattice_align on raw addresses: rows out_pad / frame_pad wider than P / M, a guard word on either side
    of every buffer.  Checks the guards, the columns beyond the widths and that the inputs are only read; returns the
    Result as numpy arrays (None for an output not asked for)."""
    import torch
    B, M, C = case.em.shape
    A = case.arcs.shape[1]
    P = fp.default_max_path(case) if P is None else P
    flat = (case.arcs if arcs is None else arcs).reshape(B, 3 * A)
    wide = np.zeros((B, 3 * A + row_pad), dtype=np.int32)  # (valid arcs of label 0 behind the rows: they would count if read)
    wide[:, 1::3] = 1
    wide[:, :3 * A] = flat
    x, a = _dev(case.em), _dev(wide)
    w = None if case.weights is None else _dev(case.weights)
    na, nn_ = _dev(case.num_arcs), _dev(case.num_nodes)
    keep = x.clone(), a.clone(), (None if w is None else w.clone()), na.clone(), nn_.clone()
    OS, FS = P + out_pad, M + frame_pad

    def buf(n, dtype, fill):
        return torch.full((n + 2,), fill, dtype=dtype, device="cuda:0")
    scores, plen = buf(B, torch.float32, GUARD_F), buf(B, torch.int32, GUARD_I)
    rows = [buf(B * OS, torch.int32, GUARD_I) for _ in range(4)]
    tsc = buf(B * OS, torch.float32, GUARD_F) if token_scores else None
    fa = buf(B * FS, torch.int32, GUARD_I) if frame_arcs else None
    ems = gtn.Batch.linear(B, M, C, x, calc_grad=False, borrow=True)

    def ptr(t):
        return None if t is None else t[1:].data_ptr()
    torch.cuda.synchronize()  # (the call runs on the engine's stream: the uploads and the guard fills come first)
    ems.ctc_lattice_align(a.data_ptr(), na.data_ptr(), nn_.data_ptr(), ptr(scores), ptr(plen), *(ptr(r) for r in rows),
                          ptr(tsc), ptr(fa), None if w is None else w.data_ptr(), case.frames, case.blank,
                          case.max_states, A=A, row_stride=3 * A + row_pad, P=P, out_stride=OS, frame_stride=FS)
    gtn.synchronize()
    for t, k in zip((x, a, w, na, nn_), keep):  # only read
        assert t is None or (t.view(torch.int32) == k.view(torch.int32)).all()

    def take(t, width, stride, guard):
        if t is None:
            return None
        h = t.cpu().numpy()
        assert h[0] == guard and h[-1] == guard, "a guard word was written"
        h = h[1:-1].reshape(B, stride)
        assert (h[:, width:] == guard).all(), "a column beyond the width was written"
        return np.ascontiguousarray(h[:, :width])
    return fp.Result(take(scores, 1, 1, GUARD_F)[:, 0], take(plen, 1, 1, GUARD_I)[:, 0],
                     *(take(r, P, OS, GUARD_I) for r in rows), take(tsc, P, OS, GUARD_F), take(fa, M, FS, GUARD_I))


def _report(name, got, want):
    for field, g, w in zip(fp.Result._fields, got, want):
        if g is not None and not (_bits(g) == _bits(w)).all():
            bad = np.argwhere(_bits(g) != _bits(w))
            print(name, field, "differs at", bad[:5].tolist(), "got", g[tuple(bad[0])], "want", w[tuple(bad[0])])


# ---- bit equality with the transcription ----
@pytest.mark.parametrize("name", fp.ALL_GPU_CASES)
def test_every_output_has_the_bits_of_the_transcription(gtn, name):
    case, want = fp.case(name), fp.result(name)
    got = _run(gtn, case)
    _report(name, got, want)
    assert _same(got, want)
    assert np.isfinite(got.scores).any() and not np.isnan(got.scores).any()


def test_the_tie_cases_have_the_bits_of_the_transcription(gtn):
    case, want = fp.tie_batch(), fp.tie_result()
    got = _run(gtn, case)
    _report("ties", got, want)
    assert _same(got, want)
    assert np.isfinite(got.scores).sum() >= len(got.scores) // 2
    # ... and with rows shorter than the paths: the true length, the head of the path
    cut = _run(gtn, case, P=2)
    assert _same(cut, fp.evaluate(case, P=2)) and (cut.path_len == got.path_len).all() and cut.path_len.max() > 2


FRAME_COUNTS = (1, 2, 63, 64, 65, 129)


def _frames_case():
    """one mid-sized lattice (6 nodes, 41 arcs, one of them from the start to the end) under 1 .. 129 frames: the
    64-frame store blocks of frame_arcs end at each of them"""
    rng = np.random.default_rng(129)
    C, blank, K = 8, 0, 6
    arcs = np.concatenate([fp.random_lattice(rng, K, 40, C, blank, max_span=5)[0], [[0, K - 1, 3]]])
    arcs = fp.sort_by_dst(arcs)[0]
    w = rng.normal(0.0, 1.0, len(arcs)).astype(np.float32)
    B = len(FRAME_COUNTS)
    em = tfp.continuous(130, B, max(FRAME_COUNTS), C)
    for b, f in enumerate(FRAME_COUNTS):
        em[b, f:] = np.nan
    a, na, nn_, ws = fp.pack([(arcs, K, w)] * B)
    return fp.Case(em, a, na, nn_, ws, blank, FRAME_COUNTS, 256, None)  # (four waves: the walk waits behind a barrier)


def test_frame_counts_around_the_store_blocks(gtn):
    case = _frames_case()
    want = fp.evaluate(case)
    got = _run(gtn, case)
    _report("frames", got, want)
    assert _same(got, want) and np.isfinite(got.scores).all()
    for b, f in enumerate(FRAME_COUNTS):
        assert (got.frame_arcs[b, f:] == -1).all() and (got.frame_arcs[b, :f] >= 0).any()


# ---- chains, and chaining into ctc_token_align ----
def _torch_align(case, **kw):
    from gtn_amd import torch_loss
    w = None if case.weights is None else _dev(case.weights)
    return torch_loss.ctc_lattice_align(_dev(case.em), _dev(case.arcs), _dev(case.num_arcs), _dev(case.num_nodes), w,
                                        blank=case.blank, input_lengths=case.frames, max_states=case.max_states, **kw)


@pytest.mark.parametrize("kind", ["continuous", "integer"])
def test_a_chain_lattice_has_the_bits_of_ctc_token_align(gtn, kind):
    from gtn_amd import torch_loss
    rng = np.random.default_rng(11)
    B, T, C, blank = 6, 40, 12, 0
    em = tfp.continuous(41, B, T, C) if kind == "continuous" else tfp.integer(41, B, T, C, -2, 1)
    hyps = [rng.integers(1, C, n).astype(np.int32) for n in (5, 20, 1, 9, 0, 41)]  # (the last does not fit)
    hyps[3][3] = hyps[3][2]  # a repeat
    arcs, na, nn_, _ = fp.pack([fp.chain_lattice(y) for y in hyps])
    L = arcs.shape[1]
    tokens = np.zeros((B, L), np.int32)
    for b, y in enumerate(hyps):
        tokens[b, :len(y)] = y
    lengths = np.array([len(y) for y in hyps], np.int32)
    case = fp.Case(em, arcs, na, nn_, None, blank, None, 2 * L + 1, None)
    got = [t.cpu().numpy() for t in _torch_align(case, max_path=L, return_token_scores=True, return_frames=True)]
    want = [t.cpu().numpy() for t in torch_loss.ctc_token_align(_dev(em), _dev(tokens), _dev(lengths), blank=blank,
                                                                 max_length=L, return_token_scores=True,
                                                                 return_frames=True)]
    scores, plen, parcs, ptok, starts, ends, tsc, fa = got
    assert (_bits(scores) == _bits(want[0])).all(), (scores, want[0])
    assert np.isfinite(scores[:5]).all() and np.isneginf(scores[5])
    assert (plen == np.where(np.isfinite(scores), lengths, 0)).all()
    for b in range(5):
        n = lengths[b]
        assert (parcs[b, :n] == np.arange(n)).all() and (ptok[b, :n] == hyps[b]).all() and (parcs[b, n:] == -1).all()
    if kind == "continuous":
        assert (starts == want[1]).all() and (ends == want[2]).all() and (fa == want[4]).all()
        assert (_bits(tsc) == _bits(want[3])).all()


@pytest.mark.parametrize("name", ["indeg8-c37", "c256", "edges", "ragged"])
def test_the_path_tokens_chain_into_ctc_token_align(gtn, name):
    """ctc_token_align of (path_tokens, path_len) gives the score less the path's weights, and the same spans where no
    token equals blank (such a token ties with the blank beside it)"""
    from gtn_amd import torch_loss
    case = fp.case(name)
    scores, plen, parcs, ptok, starts, ends = _torch_align(case)
    ts, tst, ten = torch_loss.ctc_token_align(_dev(case.em), ptok, plen, blank=case.blank, input_lengths=case.frames,
                                              max_length=max(1, min(ptok.shape[1], case.em.shape[1])))
    scores, plen, parcs, ptok, starts, ends, ts, tst, ten = (t.cpu().numpy() for t in (scores, plen, parcs, ptok, starts,
                                                                                      ends, ts, tst, ten))
    checked = 0
    for b in range(len(scores)):
        if not np.isfinite(scores[b]):
            continue
        n = plen[b]
        wp = 0.0 if case.weights is None else float(np.sum(case.weights[b, parcs[b, :n]].astype(np.float64)))
        want = float(scores[b]) - wp
        assert abs(float(ts[b]) - want) <= fp.SCORE_GATE * max(1.0, abs(float(scores[b]))), (name, b, ts[b], want)
        if (ptok[b, :n] != case.blank).all():
            assert (tst[b, :n] == starts[b, :n]).all() and (ten[b, :n] == ends[b, :n]).all(), (name, b)
            checked += 1
    assert checked >= 2


# ---- invariance ----
@pytest.mark.parametrize("name", ["s65", "indeg8-c37", "s1024"])
def test_two_calls_give_the_same_bits(gtn, name):
    assert _same(_run(gtn, fp.case(name)), _run(gtn, fp.case(name)))


@pytest.mark.parametrize("name,utts", [("indeg8-c37", 2), ("indeg8-c37", 0), ("edges", 5)])
def test_slices_give_the_bits_of_the_unsliced_run(gtn, monkeypatch, name, utts):
    """a lowered scratch cap: the utterances run in slices (two of three; one at a time, the cap below a single
    utterance's back-pointers; five of sixteen)"""
    case = fp.case(name)
    per_utt = 2 * case.em.shape[1] * case.max_states  # bytes of an utterance's back-pointers
    monkeypatch.delenv("GTNX_CTC_LATTICE_ALIGN_SCRATCH_BYTES", raising=False)
    want = _run(gtn, case)
    monkeypatch.setenv("GTNX_CTC_LATTICE_ALIGN_SCRATCH_BYTES", str(per_utt * utts + 64 if utts else 1000))
    assert _same(_run(gtn, case), want) and _same(want, fp.result(name))


def test_pad_rows_are_never_read(gtn):
    a, b, c = (_run(gtn, lfp._ragged_case(pad)) for pad in (np.nan, 123.0, np.inf))
    assert _same(a, b) and _same(a, c) and _same(a, fp.result("ragged"))


def test_what_lies_past_num_arcs_is_never_read_and_a_wider_row_stride_changes_nothing(gtn):
    case = fp.case("indeg8-c37")
    want = _run(gtn, case)
    arcs = case.arcs.copy()
    past = np.arange(arcs.shape[1])[None, :] >= case.num_arcs[:, None]
    assert past.any()
    arcs[past] = np.random.default_rng(3).integers(-5, 10 ** 6, (int(past.sum()), 3))
    w = case.weights.copy()
    w[past] = np.nan
    assert _same(_run(gtn, case._replace(weights=w), arcs=arcs), want)
    assert _same(_run(gtn, case, row_pad=7), want)


def test_the_optional_outputs_change_nothing(gtn):
    case = fp.case("indeg8-c37")
    want = _run(gtn, case)
    for ts, fa in ((False, False), (True, False), (False, True)):
        got = _run(gtn, case, token_scores=ts, frame_arcs=fa)
        assert (got.token_scores is None) == (not ts) and (got.frame_arcs is None) == (not fa)
        assert _same(got[:6], want[:6])
        assert ts is False or _same([got.token_scores], [want.token_scores])
        assert fa is False or _same([got.frame_arcs], [want.frame_arcs])
    assert _same(_run(gtn, case, out_pad=0, frame_pad=0), want)  # rows exactly P and M wide


def test_invalid_lattices_leave_their_neighbours_bits_alone(gtn):
    case = fp.case("edges")
    whole = _run(gtn, case)
    fin = np.isfinite(whole.scores)
    valid = np.nonzero(fin)[0]
    alone = _run(gtn, fp.Case(case.em[valid], case.arcs[valid], case.num_arcs[valid], case.num_nodes[valid],
                              case.weights[valid], case.blank, None, case.max_states, None))
    assert _same(alone, [f[valid] for f in whole])
    assert (whole.path_len[~fin] == 0).all() and (whole.path_arcs[~fin] == -1).all()
    assert (whole.frame_arcs[~fin] == -1).all() and np.isneginf(whole.token_scores[~fin]).all()


# ---- the routes ----
def test_the_native_and_the_batch_route_agree_and_the_counter_counts(gtn):
    case, want = fp.case("indeg8-c37"), fp.result("indeg8-c37")
    B = case.em.shape[0]
    c0 = gtn.debug_ctc_lattice_align_stats()
    via_batch = _run(gtn, case)
    c1 = gtn.debug_ctc_lattice_align_stats()
    out = _torch_align(case, return_token_scores=True, return_frames=True)
    c2 = gtn.debug_ctc_lattice_align_stats()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, B) and (c2[0] - c1[0], c2[1] - c1[1]) == (1, B)
    native = [t.cpu().numpy() for t in out]
    assert _same(native, via_batch) and _same(native, want)
    short = _torch_align(case)
    assert len(short) == 6 and _same([t.cpu().numpy() for t in short], want[:6])
    # tensors in the place of addresses
    import torch
    P, M = want.path_arcs.shape[1], case.em.shape[1]
    # (the batch BORROWS x and the call runs on the engine's stream: the inputs stay alive, and uploaded, until it is done)
    x, a, na, nn_, w = (_dev(v) for v in (case.em, case.arcs, case.num_arcs, case.num_nodes, case.weights))
    ems = gtn.Batch.linear(*case.em.shape, x, calc_grad=False, borrow=True)
    s, n = torch.empty(B, device="cuda:0"), torch.empty(B, dtype=torch.int32, device="cuda:0")
    rows = [torch.empty(B, P, dtype=torch.int32, device="cuda:0") for _ in range(4)]
    fa = torch.empty(B, M, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ems.ctc_lattice_align(a, na, nn_, s, n, *rows, None, fa, w, blank=case.blank, max_states=case.max_states)
    gtn.synchronize()
    got = [t.cpu().numpy() for t in (s, n, *rows)] + [None, fa.cpu().numpy()]
    assert _same(got[:6], want[:6]) and (got[7] == want.frame_arcs).all()


def test_a_lattice_without_an_arc_row_is_the_empty_path(gtn):
    import torch
    from gtn_amd import torch_loss
    case = fp.case("edges")
    x = _dev(case.em[:2])
    out = torch_loss.ctc_lattice_align(x, torch.zeros(2, 0, 3, dtype=torch.int32, device="cuda:0"),
                                       torch.zeros(2, dtype=torch.int64, device="cuda:0"),
                                       torch.tensor([1, 2], dtype=torch.int64, device="cuda:0"), blank=case.blank,
                                       return_frames=True)
    scores, plen, parcs, ptok, starts, ends, fa = (t.cpu().numpy() for t in out)
    s = case.em[0, 0, case.blank]
    for t in range(1, case.em.shape[1]):
        s = np.float32(s + case.em[0, t, case.blank])
    assert scores[0] == s and np.isneginf(scores[1]) and (plen == 0).all() and parcs.shape == (2, 1)
    assert (parcs == -1).all() and (ptok == -1).all() and (starts == -1).all() and (ends == -1).all() and (fa == -1).all()


def test_what_needs_the_device_is_refused_there(gtn):
    """not a native linear batch, a frame count outside 0 .. M, blank >= C, frame rows shorter than M: invalid arguments,
    nothing is launched and nothing is written"""
    import torch
    case = fp.case("edges")
    B, T, C = case.em.shape
    x, arcs, na, nn_ = _dev(case.em), _dev(case.arcs), _dev(case.num_arcs), _dev(case.num_nodes)
    s, n = torch.zeros(B, device="cuda:0"), torch.zeros(B, dtype=torch.int32, device="cuda:0")
    rows = [torch.zeros(B, 4, dtype=torch.int32, device="cuda:0") for _ in range(4)]
    fa = torch.zeros(B, T, dtype=torch.int32, device="cuda:0")
    ems = gtn.Batch.linear(B, T, C, x, calc_grad=False, borrow=True)
    c0 = gtn.debug_ctc_lattice_align_stats()
    with pytest.raises(ValueError, match="frame count outside"):
        ems.ctc_lattice_align(arcs, na, nn_, s, n, *rows, frames=[T + 1] + [1] * (B - 1))
    with pytest.raises(ValueError, match="blank is not below"):
        ems.ctc_lattice_align(arcs, na, nn_, s, n, *rows, blank=C)
    with pytest.raises(ValueError, match="frame_stride is shorter"):
        ems.ctc_lattice_align(arcs.data_ptr(), na.data_ptr(), nn_.data_ptr(), s.data_ptr(), n.data_ptr(),
                              *(r.data_ptr() for r in rows), None, fa.data_ptr(), A=case.arcs.shape[1],
                              row_stride=3 * case.arcs.shape[1], P=4, frame_stride=T - 1)
    with pytest.raises(ValueError, match="not a native linear batch"):
        gtn.Batch([gtn.linear_graph(T, C) for _ in range(B)]).ctc_lattice_align(arcs, na, nn_, s, n, *rows)
    gtn.synchronize()
    assert gtn.debug_ctc_lattice_align_stats() == c0
    assert (s == 0).all() and (n == 0).all() and all((r == 0).all() for r in rows) and (fa == 0).all()
