"""Batched CTC token alignment of device-resident hypotheses (ctc_token_align.hip through gtnx_batch_ctc_token_align;
gtn_amd.torch_loss.ctc_token_align, Batch.ctc_token_align, gtn_ctc_token_align_n).

The judge is the float32 yardstick of tests/ctc_token_align_fp.py, which tests/test_ctc_token_align_cpu.py pins to the
oracle's shortest_path on tie-heavy inputs, to ctc_align_fp64 and to an enumeration.  The contract fixes every addition,
every maximum and every tie, so EVERY device output is compared with the yardstick bit for bit: there is no tolerance.
The cases sit at the kernel's edges: the widths of ctc_score_config, the frame counts around a back-pointer word and a
store of 64 frames, two states a frame (the reach of a word row), ties, pairs without a path."""
import numpy as np
import pytest

import ctc_token_align_fp as fp

pytestmark = pytest.mark.gpu
NEG = -np.inf
NAMES = ("scores", "starts", "ends", "token_scores", "frame_tokens")


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True, order="C")).to("cuda:0")


def _run(case, tokens=None, lengths=None, token_scores=True, frames=True):
    """torch_loss.ctc_token_align on a case: the outputs as numpy arrays, in the order of fp.Result (None: not asked for)"""
    import torch
    from gtn_amd import torch_loss
    tok = _dev(case.tokens) if tokens is None else tokens
    ln = _dev(case.lengths) if lengths is None else lengths
    before = tok.cpu().numpy().copy()
    out = list(torch_loss.ctc_token_align(_dev(case.em), tok, ln, blank=case.blank, input_lengths=case.frames,
                                          max_length=case.max_length, return_token_scores=token_scores,
                                          return_frames=frames))
    torch.cuda.synchronize()
    assert (tok.cpu().numpy() == before).all()  # only read
    got = [o.cpu().numpy() for o in out[:3]]
    got.append(out[3].cpu().numpy() if token_scores else None)
    got.append(out[-1].cpu().numpy() if frames else None)
    return got


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        if g is None or w is None:
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        diff = _bits(g) != _bits(w)
        assert not diff.any(), (what, name, np.argwhere(diff)[:5].tolist(), g[diff][:5], w[diff][:5])


@pytest.mark.parametrize("name", fp.ALL_GPU_CASES)
def test_every_output_has_the_bits_of_the_yardstick(gtn, name):
    case, want = fp.case(name), fp.result(name)
    _same(_run(case), want, name)
    assert (want.scores > NEG).any()


def test_against_the_existing_aligner(gtn):
    """tokens above blank: frame_tokens is the `tokens` plane of ctc_forced_align on the same targets and the score has
    the same bits, with continuous emissions and with ties everywhere"""
    from gtn_amd import torch_loss
    for name in ("align-continuous", "align-zero"):
        case = fp.case(name)
        got = _run(case)
        targets = [case.tokens[b, 0, :case.lengths[b, 0]].tolist() for b in range(case.em.shape[0])]
        _, tokens, scores = torch_loss.ctc_forced_align(_dev(case.em), targets, blank=case.blank, input_lengths=case.frames)
        assert (got[4][:, 0] == tokens.cpu().numpy()).all(), name
        assert (_bits(got[0][:, 0]) == _bits(scores.cpu().numpy())).all(), name


def test_pad_rows_and_elements_past_a_length_are_never_read(gtn):
    a = _run(fp._nopath_case(np.nan))
    b = _run(fp._nopath_case(123.0))
    c = _run(fp._nopath_case(np.inf, garbage=3))
    _same(a, b)
    _same(a, c)
    _same(a, fp.result("nopath"))


def test_the_outputs_are_written_exactly_over_their_widths(gtn):
    """sentinel columns beyond L and M, rows further apart than they are wide, raw addresses and tensor views"""
    import torch
    case, want = fp.case("nopath"), fp.result("nopath")
    B, M, C = case.em.shape
    N, L = case.tokens.shape[1:]
    x, tok, ln = _dev(case.em), _dev(case.tokens), _dev(case.lengths)
    ems = gtn.Batch.linear(B, M, C, x, calc_grad=False, borrow=True)
    fr = case.frames

    def fresh():
        return (torch.full((B * N + 2,), 5.0, device="cuda:0"),
                torch.full((B, N, L + 3), 77, dtype=torch.int32, device="cuda:0"),
                torch.full((B, N, L + 3), 77, dtype=torch.int32, device="cuda:0"),
                torch.full((B, N, L + 3), 7.5, device="cuda:0"),
                torch.full((B, N, M + 5), 77, dtype=torch.int32, device="cuda:0"))

    def check(sc, st, en, ts, ft):
        gtn.synchronize()
        s = sc.cpu().numpy()
        assert s[0] == 5.0 and s[-1] == 5.0, "guards"
        for t, width, guard in ((st, L, 77), (en, L, 77), (ts, L, 7.5), (ft, M, 77)):
            assert (t[:, :, width:] == guard).all(), "a column beyond the width was written"
        _same([s[1:-1].reshape(B, N), st[:, :, :L].cpu().numpy(), en[:, :, :L].cpu().numpy(), ts[:, :, :L].cpu().numpy(),
               ft[:, :, :M].cpu().numpy()], want)
    c0 = gtn.debug_ctc_token_align_stats()
    sc, st, en, ts, ft = fresh()
    ems.ctc_token_align(tok.data_ptr(), ln.data_ptr(), sc[1:].data_ptr(), st.data_ptr(), en.data_ptr(), ts.data_ptr(),
                        ft.data_ptr(), fr, case.blank, case.max_length, N=N, L=L, row_stride=L, out_stride=L + 3,
                        frame_stride=M + 5)
    check(sc, st, en, ts, ft)
    sc, st, en, ts, ft = fresh()
    ems.ctc_token_align(tok, ln, sc[1:-1].reshape(B, N), st[:, :, :L], en[:, :, :L], ts[:, :, :L], ft[:, :, :M], fr,
                        case.blank, case.max_length)
    check(sc, st, en, ts, ft)
    c1 = gtn.debug_ctc_token_align_stats()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (2, 2 * B * N)


def test_forms_and_optional_outputs(gtn):
    """[B, L] against [B, 1, L]; int64 lengths; the optional outputs off and on leave the others' bits alone"""
    import torch
    case, want = fp.case("flat"), fp.result("flat")
    B = case.em.shape[0]
    full = _run(case)
    _same(full, want)
    flat = _run(case, tokens=_dev(case.tokens[:, 0]), lengths=_dev(case.lengths[:, 0].astype(np.int64)))
    assert flat[0].shape == (B,) and flat[1].shape == (B, 30) and flat[4].shape == (B, 50)
    _same([f.reshape(w.shape) for f, w in zip(flat, want)], want)
    for ts, ft in ((False, False), (True, False), (False, True)):
        got = _run(case, token_scores=ts, frames=ft)
        assert (got[3] is None) == (not ts) and (got[4] is None) == (not ft)
        _same(got, want)
    c = fp.case("words")
    _same(_run(c, lengths=_dev(c.lengths.astype(np.int64))), fp.result("words"))
    # rows without an element, and no pairs at all
    from gtn_amd import torch_loss
    x = _dev(case.em)
    s, st, en = torch_loss.ctc_token_align(x, torch.zeros(B, 2, 0, dtype=torch.int32, device="cuda:0"),
                                           torch.zeros(B, 2, dtype=torch.int32, device="cuda:0"), blank=case.blank)
    assert st.shape == (B, 2, 0) and en.shape == (B, 2, 0) and torch.isfinite(s).all()
    c0 = gtn.debug_ctc_token_align_stats()
    s, st, en, ft = torch_loss.ctc_token_align(x, torch.zeros(B, 0, 8, dtype=torch.int32, device="cuda:0"),
                                               torch.zeros(B, 0, dtype=torch.int32, device="cuda:0"), return_frames=True)
    assert s.shape == (B, 0) and st.shape == (B, 0, 8) and ft.shape == (B, 0, 50)
    assert gtn.debug_ctc_token_align_stats() == c0


@pytest.mark.parametrize("pairs", [5, 1, 0])
def test_slices_give_the_bits_of_the_unsliced_run(gtn, monkeypatch, pairs):
    """a lowered scratch cap: slices of five pairs that cut utterances of three apart, of one pair, and a cap below a
    single pair's words"""
    case = fp.case("slices")
    per_pair = 4 * ((int(case.frames.max()) + 15) // 16) * (2 * case.max_length + 1)  # bytes of a pair's words
    monkeypatch.delenv("GTNX_CTC_TOKEN_ALIGN_SCRATCH_BYTES", raising=False)
    want = _run(case)
    _same(want, fp.result("slices"))
    monkeypatch.setenv("GTNX_CTC_TOKEN_ALIGN_SCRATCH_BYTES", str(per_pair * pairs + 8 if pairs else 100))
    c0 = gtn.debug_ctc_token_align_stats()
    _same(_run(case), want)
    c1 = gtn.debug_ctc_token_align_stats()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, 12)  # (a sliced call is one call)


@pytest.mark.parametrize("name", ["ties", "words", "width-383"])
def test_two_calls_give_the_same_bits(gtn, name):
    _same(_run(fp.case(name)), _run(fp.case(name)))


def test_the_native_route_and_the_batch_route_agree(gtn, monkeypatch):
    from gtn_amd import torch_loss
    case = fp.case("nopath")
    assert torch_loss._native() and hasattr(torch_loss._native(), "gtn_ctc_token_align_n")
    native = _run(case)
    monkeypatch.setattr(torch_loss, "_NATIVE", False)
    c0 = gtn.debug_ctc_token_align_stats()
    batch = _run(case)
    assert gtn.debug_ctc_token_align_stats()[0] == c0[0] + 1
    _same(native, batch)


def test_what_needs_the_device_is_refused_there(gtn):
    """not a native linear batch, a frame count outside 0 .. M, blank >= C, frame_stride < M: invalid arguments, nothing
    is launched and nothing written"""
    import torch
    case = fp.case("nopath")
    B, M, C = case.em.shape
    N, L = case.tokens.shape[1:]
    x, tok, ln = _dev(case.em), _dev(case.tokens), _dev(case.lengths)
    sc = torch.zeros(B, N, device="cuda:0")
    st = torch.zeros(B, N, L, dtype=torch.int32, device="cuda:0")
    en = torch.zeros(B, N, L, dtype=torch.int32, device="cuda:0")
    ft = torch.zeros(B, N, M, dtype=torch.int32, device="cuda:0")
    ems = gtn.Batch.linear(B, M, C, x, calc_grad=False, borrow=True)
    c0 = gtn.debug_ctc_token_align_stats()
    with pytest.raises(ValueError, match="frame count outside"):
        ems.ctc_token_align(tok, ln, sc, st, en, frames=[M + 1] + [1] * (B - 1))
    with pytest.raises(ValueError, match="blank is not below"):
        ems.ctc_token_align(tok, ln, sc, st, en, blank=C)
    with pytest.raises(ValueError, match="frame_stride is shorter"):
        ems.ctc_token_align(tok.data_ptr(), ln.data_ptr(), sc.data_ptr(), st.data_ptr(), en.data_ptr(), None,
                            ft.data_ptr(), N=N, L=L, row_stride=L, frame_stride=M - 1)
    with pytest.raises(ValueError, match="not a native linear batch"):
        gtn.Batch([gtn.linear_graph(M, C) for _ in range(B)]).ctc_token_align(tok, ln, sc, st, en)
    gtn.synchronize()
    assert gtn.debug_ctc_token_align_stats() == c0
    assert (sc == 0).all() and (st == 0).all() and (en == 0).all() and (ft == 0).all()


def test_after_the_beam_search(gtn):
    """ctc_beam_decode(nbest=3) -> ctc_token_align: every hypothesis's frame tokens, collapsed, spell the hypothesis, and
    the best path scores no more than all paths together (1e-4 max(1, |score|) for ctc_score's float32 log-add)"""
    import torch
    from gtn_amd import torch_loss
    B, T, C, blank = 4, 40, 10, 0
    x = torch.log_softmax(_dev(fp.continuous(41, B, T, C)), dim=2)
    frames = [40, 25, 40, 7]
    tokens, lengths, beam = torch_loss.ctc_beam_decode(x, blank=blank, input_lengths=frames, beam_size=8, cutoff_top_n=6,
                                                       nbest=3)
    scores, starts, ends, tsc, ft = torch_loss.ctc_token_align(x, tokens, lengths, blank=blank, input_lengths=frames,
                                                               return_token_scores=True, return_frames=True)
    total = torch_loss.ctc_score(x, tokens, lengths, blank=blank, input_lengths=frames)
    tk, ln, ft, st, en = (t.cpu().numpy() for t in (tokens, lengths, ft, starts, ends))
    sc, tot, have = scores.cpu().numpy(), total.cpu().numpy(), np.isfinite(beam.cpu().numpy())
    assert have[:, 0].all() and have.sum() > B
    for b in range(B):
        for k in range(3):
            if not have[b, k]:
                continue
            n = ln[b, k]
            assert np.isfinite(sc[b, k])
            row = ft[b, k, :frames[b]]
            on = row[row >= 0]
            idx = on[np.concatenate([[True], np.diff(on) != 0])] if on.size else on
            assert idx.tolist() == list(range(n)) and (ft[b, k, frames[b]:] == -1).all()
            assert (tk[b, k][idx] == tk[b, k, :n]).all()
            assert ((en[b, k, :n] - st[b, k, :n]) == np.bincount(on, minlength=n)).all()
            assert sc[b, k] <= tot[b, k] + 1e-4 * max(1.0, abs(tot[b, k]))
    conf = torch.exp(tsc / (ends - starts).clamp(min=1))  # the usual per-token confidence
    assert ((conf > 0) & (conf <= 1))[starts >= 0].all()
