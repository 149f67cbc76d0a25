"""Batched ASG token alignment of device-resident hypotheses (asg_token_align.hip through gtnx_batch_asg_token_align;
gtn_amd.torch_loss.asg_token_align, Batch.asg_token_align, gtn_asg_token_align_n).

The judge is the float32 yardstick of tests/asg_token_align_fp.py, which tests/test_asg_token_align_cpu.py pins to the
oracle's shortest_path on integer-valued inputs and to two float64 forms on continuous ones.  The contract fixes every
addition, every maximum and every tie, so EVERY device output is compared with the yardstick bit for bit: there is no
tolerance.  The cases sit at the kernel's edges: the widths of asg_score_config, the frame counts around a back-pointer
word and a store of 64 frames, one position a frame (the reach of a word row), ties, pairs without a path."""
import ctypes

import numpy as np
import pytest

import asg_token_align_fp as fp

pytestmark = pytest.mark.gpu
NEG = -np.inf
NAMES = ("scores", "starts", "ends", "token_scores", "frame_tokens")


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True, order="C")).to("cuda:0")


def _run(case, tokens=None, lengths=None, token_scores=True, frames=True):
    """torch_loss.asg_token_align on a case: the outputs as numpy arrays, in the order of fp.Result (None: not asked for)"""
    import torch
    from gtn_amd import torch_loss
    tok = _dev(case.tokens) if tokens is None else tokens
    ln = _dev(case.lengths) if lengths is None else lengths
    x, tr, st = _dev(case.em), _dev(case.trans), _dev(case.start)
    before = [t.cpu().numpy().copy() for t in (tok, x, tr, st)]
    out = list(torch_loss.asg_token_align(x, tr, tok, ln, start=st, input_lengths=case.frames,
                                          max_length=case.max_length, return_token_scores=token_scores,
                                          return_frames=frames))
    torch.cuda.synchronize()
    for t, b in zip((tok, x, tr, st), before):  # only read
        assert (t.cpu().numpy().view(np.uint32 if b.dtype == np.float32 else b.dtype) ==
                b.view(np.uint32 if b.dtype == np.float32 else b.dtype)).all()
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


@pytest.mark.parametrize("name", ["align-c8", "align-c300", "align-c8-zero"])
def test_against_the_existing_aligner(gtn, name):
    """where asg_forced_align's launch applies (C in {8, 300}, U + 1 in {2, 65, 129, 512}): frame_tokens is its `tokens`
    plane and the score has the same bits, with continuous inputs and with ties everywhere"""
    from gtn_amd import torch_loss
    case = fp.case(name)
    got = _run(case)
    B = case.em.shape[0]
    targets = [case.tokens[b, 0, :case.lengths[b, 0]].tolist() for b in range(B)]
    f0 = gtn.debug_align_stats()
    labels, tokens, scores = torch_loss.asg_forced_align(_dev(case.em), _dev(case.trans), targets, start=_dev(case.start),
                                                         input_lengths=case.frames)
    f1 = gtn.debug_align_stats()
    assert (f1[0] - f0[0], f1[1] - f0[1]) == (B, 0)  # (its kernel, not the path-graph route)
    assert (got[4][:, 0] == tokens.cpu().numpy()).all()
    assert (_bits(got[0][:, 0]) == _bits(scores.cpu().numpy())).all()
    lab = labels.cpu().numpy()
    for b in range(B):
        f = int(case.frames[b])
        assert (case.tokens[b, 0][got[4][b, 0, :f]] == lab[b, :f]).all()


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
    x, ln = _dev(case.em), _dev(case.lengths)
    wide = torch.full((B, N, L + 2), 10 ** 6, dtype=torch.int32, device="cuda:0")  # (a row stride above the width)
    wide[:, :, :L] = _dev(case.tokens)
    table = _dev(fp.table_of(case.start, case.trans))
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
    c0 = gtn.debug_asg_token_align_stats()
    sc, st, en, ts, ft = fresh()
    ems.asg_token_align(wide.data_ptr(), ln.data_ptr(), sc[1:].data_ptr(), st.data_ptr(), en.data_ptr(), ts.data_ptr(),
                        ft.data_ptr(), fr, table.data_ptr(), case.max_length, N=N, L=L, row_stride=L + 2,
                        out_stride=L + 3, frame_stride=M + 5)
    check(sc, st, en, ts, ft)
    sc, st, en, ts, ft = fresh()
    ems.asg_token_align(wide[:, :, :L], ln, sc[1:-1].reshape(B, N), st[:, :, :L], en[:, :, :L], ts[:, :, :L],
                        ft[:, :, :M], fr, table, case.max_length)
    check(sc, st, en, ts, ft)
    c1 = gtn.debug_asg_token_align_stats()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (2, 2 * B * N)


def test_forms_and_optional_outputs(gtn):
    """[B, L] against [B, 1, L]; int64 lengths; each optional output alone leaves the others' bits alone"""
    import torch
    from gtn_amd import torch_loss
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
    # rows without an element (no path: there is no empty alignment), and no pairs at all
    x, tr = _dev(case.em), _dev(case.trans)
    s, st, en = torch_loss.asg_token_align(x, tr, torch.zeros(B, 2, 0, dtype=torch.int32, device="cuda:0"),
                                           torch.zeros(B, 2, dtype=torch.int32, device="cuda:0"))
    assert st.shape == (B, 2, 0) and en.shape == (B, 2, 0) and torch.isneginf(s).all()
    c0 = gtn.debug_asg_token_align_stats()
    s, st, en, ft = torch_loss.asg_token_align(x, tr, torch.zeros(B, 0, 8, dtype=torch.int32, device="cuda:0"),
                                               torch.zeros(B, 0, dtype=torch.int32, device="cuda:0"), return_frames=True)
    assert s.shape == (B, 0) and st.shape == (B, 0, 8) and ft.shape == (B, 0, 50)
    assert gtn.debug_asg_token_align_stats() == c0


@pytest.mark.parametrize("pairs", [5, 1, 0])
def test_slices_give_the_bits_of_the_unsliced_run(gtn, monkeypatch, pairs):
    """a lowered scratch cap: slices of five pairs that cut utterances of three apart, of one pair, and a cap below a
    single pair's words"""
    case = fp.case("slices")
    per_pair = 4 * ((int(case.frames.max()) + 31) // 32) * case.max_length  # bytes of a pair's words
    monkeypatch.delenv("GTNX_ASG_TOKEN_ALIGN_SCRATCH_BYTES", raising=False)
    want = _run(case)
    _same(want, fp.result("slices"))
    monkeypatch.setenv("GTNX_ASG_TOKEN_ALIGN_SCRATCH_BYTES", str(per_pair * pairs + 8 if pairs else 100))
    c0 = gtn.debug_asg_token_align_stats()
    _same(_run(case), want)
    c1 = gtn.debug_asg_token_align_stats()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, 12)  # (a sliced call is one call)


@pytest.mark.parametrize("name", ["ties-01", "words", "width-769"])
def test_two_calls_give_the_same_bits(gtn, name):
    _same(_run(fp.case(name)), _run(fp.case(name)))


def test_the_native_route_and_the_batch_route_agree(gtn, monkeypatch):
    """... with a 0 among the input lengths"""
    from gtn_amd import torch_loss
    case = fp.case("nopath")
    assert 0 in case.frames.tolist()
    assert torch_loss._native() and hasattr(torch_loss._native(), "gtn_asg_token_align_n")
    c0 = gtn.debug_asg_token_align_stats()
    native = _run(case)
    monkeypatch.setattr(torch_loss, "_NATIVE", False)
    batch = _run(case)
    assert gtn.debug_asg_token_align_stats()[0] == c0[0] + 2
    _same(native, batch)
    _same(native, fp.result("nopath"))


def test_the_criteria_abi(gtn):
    """gtn_asg_token_align_n called as a C program would call it"""
    import torch
    from gtn_amd import torch_loss
    case, want = fp.case("alphabet-5"), fp.result("alphabet-5")
    B, T, C = case.em.shape
    N, L = case.tokens.shape[1:]
    lib = torch_loss._native()
    x, tok, ln = _dev(case.em), _dev(case.tokens), _dev(case.lengths)
    table = _dev(fp.table_of(case.start, case.trans))
    sc = torch.empty(B, N, device="cuda:0")
    st = torch.empty(B, N, L, dtype=torch.int32, device="cuda:0")
    en = torch.empty(B, N, L, dtype=torch.int32, device="cuda:0")
    ts = torch.empty(B, N, L, device="cuda:0")
    ft = torch.empty(B, N, T, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    gtn.set_stream(None)
    fr = np.ascontiguousarray(case.frames, dtype=np.int32)
    rc = lib.gtn_asg_token_align_n(x.data_ptr(), B, T, C, table.data_ptr(), fr.ctypes.data, tok.data_ptr(),
                                   ln.data_ptr(), N, L, fp.max_length_of(case), sc.data_ptr(), st.data_ptr(),
                                   en.data_ptr(), ts.data_ptr(), ft.data_ptr())
    assert rc == 0, lib.gtn_criteria_last_error().decode()
    gtn.synchronize()
    _same([t.cpu().numpy() for t in (sc, st, en, ts, ft)], want)
    rc = lib.gtn_asg_token_align_n(x.data_ptr(), B, T, C, None, fr.ctypes.data, tok.data_ptr(), ln.data_ptr(), N, L,
                                   fp.max_length_of(case), sc.data_ptr(), st.data_ptr(), en.data_ptr(), None, None)
    assert rc != 0 and "[gtnx_batch_asg_token_align] null table pointer" in lib.gtn_criteria_last_error().decode()


def test_what_needs_the_device_is_refused_there(gtn):
    """not a native linear batch, a frame count outside 0 .. M, frame_stride < M, a table in host memory, an output on
    another device: invalid arguments, nothing is launched and nothing written"""
    import torch
    case = fp.case("nopath")
    B, M, C = case.em.shape
    N, L = case.tokens.shape[1:]
    x, tok, ln = _dev(case.em), _dev(case.tokens), _dev(case.lengths)
    table = _dev(fp.table_of(case.start, case.trans))
    sc = torch.zeros(B, N, device="cuda:0")
    st = torch.zeros(B, N, L, dtype=torch.int32, device="cuda:0")
    en = torch.zeros(B, N, L, dtype=torch.int32, device="cuda:0")
    ft = torch.zeros(B, N, M, dtype=torch.int32, device="cuda:0")
    ems = gtn.Batch.linear(B, M, C, x, calc_grad=False, borrow=True)
    c0 = gtn.debug_asg_token_align_stats()
    with pytest.raises(ValueError, match=r"\[gtnx_batch_asg_token_align\] a frame count outside 0 \.\. M"):
        ems.asg_token_align(tok, ln, sc, st, en, frames=[M + 1] + [1] * (B - 1), table=table)
    with pytest.raises(ValueError, match=r"\[gtnx_batch_asg_token_align\] frame_stride is shorter than the rows"):
        ems.asg_token_align(tok.data_ptr(), ln.data_ptr(), sc.data_ptr(), st.data_ptr(), en.data_ptr(), None,
                            ft.data_ptr(), None, table.data_ptr(), N=N, L=L, row_stride=L, frame_stride=M - 1)
    with pytest.raises(ValueError, match=r"\[gtnx_batch_asg_token_align\] not a native linear batch"):
        gtn.Batch([gtn.linear_graph(M, C) for _ in range(B)]).asg_token_align(tok, ln, sc, st, en, table=table.data_ptr())
    host = torch.from_numpy(fp.table_of(case.start, case.trans))
    for t in (host, host.pin_memory()):
        with pytest.raises(ValueError, match=r"\[gtnx_batch_asg_token_align\] the table is not memory of the engine's"):
            ems.asg_token_align(tok, ln, sc, st, en, None, ft, table=t.data_ptr())
    with pytest.raises(ValueError, match="table has 55 entries"):
        ems.asg_token_align(tok, ln, sc, st, en, table=table[:-1])
    if torch.cuda.device_count() > 1:
        other = torch.zeros(B, N, L, dtype=torch.int32, device="cuda:1")
        with pytest.raises(ValueError, match="output pointer is not memory"):
            ems.asg_token_align(tok.data_ptr(), ln.data_ptr(), sc.data_ptr(), st.data_ptr(), other.data_ptr(),
                                table=table.data_ptr(), N=N, L=L, row_stride=L)
        assert (other == 0).all()
    gtn.synchronize()
    assert gtn.debug_asg_token_align_stats() == c0
    assert (sc == 0).all() and (st == 0).all() and (en == 0).all() and (ft == 0).all()


@pytest.mark.parametrize("name", ["slices", "ties-01", "ties-zero", "nopath"])
def test_against_the_score_of_all_alignments(gtn, name):
    """Batch.asg_score on the same device tensors: the pairs without a path are its -inf pairs, and the best alignment
    scores no more than all alignments together.  In exact arithmetic max <= log-sum; in float32 that is certain where
    every sum of the max-plus recursion is exact -- integer-valued inputs: log-add never returns less than its larger
    argument and rounding is monotone, so alpha_logadd >= alpha_max by induction over the frames -- so the inequality is
    asserted on the integer-valued cases; the continuous case (nopath) checks the dead pairs only"""
    import torch
    case = fp.case(name)
    B, M, C = case.em.shape
    N, L = case.tokens.shape[1:]
    x, tok, ln = _dev(case.em), _dev(case.tokens), _dev(case.lengths)
    table = _dev(fp.table_of(case.start, case.trans))
    ems = gtn.Batch.linear(B, M, C, x, calc_grad=False, borrow=True)
    total = torch.empty(B, N, device="cuda:0")
    best = torch.empty(B, N, device="cuda:0")
    st = torch.empty(B, N, L, dtype=torch.int32, device="cuda:0")
    en = torch.empty(B, N, L, dtype=torch.int32, device="cuda:0")
    U = fp.max_length_of(case)
    ems.asg_score(table, tok, ln, total, case.frames, U)
    ems.asg_token_align(tok, ln, best, st, en, None, None, case.frames, table, U)
    gtn.synchronize()
    best, total = best.cpu().numpy(), total.cpu().numpy()
    assert (np.isneginf(best) == np.isneginf(total)).all() and not np.isnan(best).any()
    assert (best > NEG).any()
    if name != "nopath":
        assert (best <= total).all()
    else:
        assert np.isneginf(best).sum() >= 15


def _decode_inputs():
    rng = np.random.default_rng(51)
    B, T, C = 4, 40, 12
    return (rng.normal(0, 2, (B, T, C)).astype(np.float32), rng.normal(0, 1, (C, C)).astype(np.float32),
            rng.normal(0, 1, C).astype(np.float32), [40, 25, 33, 7])


def test_after_the_viterbi_decode(gtn):
    """asg_decode(collapse=True) -> asg_token_align with L = T, nothing downloaded on the way: the decoded path is the
    best alignment of its collapsed sequence, so tokens[frame_tokens] are asg_decode's frame labels.  The two scores are
    float32 sums of the same 3 T_b terms (0, then per frame a weight and an emission) in two orders: each lies within
    (3 T_b - 1) 2^-24 sum |terms| of the float64 path sum, the two within twice that of each other"""
    from gtn_amd import torch_loss
    em, trans, start, frames = _decode_inputs()
    x, tr, s0 = _dev(em), _dev(trans), _dev(start)
    labels, dscores, collapsed, lengths = torch_loss.asg_decode(x, tr, start=s0, input_lengths=frames, collapse=True)
    scores, starts, ends, ft = torch_loss.asg_token_align(x, tr, collapsed, lengths, start=s0, input_lengths=frames,
                                                          return_frames=True)
    lab, col, ln, ft = (t.cpu().numpy() for t in (labels, collapsed, lengths, ft))
    sc, dsc, st, en = (t.cpu().numpy() for t in (scores, dscores, starts, ends))
    for b, f in enumerate(frames):
        assert (col[b][ft[b, :f]] == lab[b, :f]).all() and (ft[b, f:] == -1).all()
        n = int(ln[b])
        assert st[b, 0] == 0 and en[b, n - 1] == f and (en[b, :n - 1] == st[b, 1:n]).all()
        path = lab[b, :f]
        terms = [float(start[path[0]])] + [float(trans[path[t], path[t - 1]]) for t in range(1, f)]
        terms += [float(em[b, t, path[t]]) for t in range(f)]
        total, mass = float(np.sum(terms)), float(np.sum(np.abs(terms)))
        bound = 2 * (3 * f - 1) * 2.0 ** -24 * mass
        print(b, f, float(sc[b]), float(dsc[b]), total, bound)
        assert abs(float(sc[b]) - total) <= bound
        assert abs(float(sc[b]) - float(dsc[b])) <= bound


def test_after_the_beam_search(gtn):
    """asg_beam_decode(nbest=3) -> asg_token_align -> asg_score on the tensors the search left on the device: every
    hypothesis's frame tokens cover its tokens in order, a slot without a hypothesis has no path, and the best alignment
    scores no more than all of them together (1e-4 max(1, |score|) for asg_score's float32 log-add)"""
    import torch
    from gtn_amd import torch_loss
    em, trans, start, frames = _decode_inputs()
    x, tr, s0 = torch.log_softmax(_dev(em), dim=2), _dev(trans), _dev(start)
    tokens, lengths, beam = torch_loss.asg_beam_decode(x, tr, start=s0, input_lengths=frames, beam_size=8, cutoff_top_n=6,
                                                       nbest=3)
    scores, starts, ends, tsc, ft = torch_loss.asg_token_align(x, tr, tokens, lengths, start=s0, input_lengths=frames,
                                                               return_token_scores=True, return_frames=True)
    total = torch_loss.asg_score(x, tr, tokens, lengths, start=s0, input_lengths=frames)
    ln, ft, st, en = (t.cpu().numpy() for t in (lengths, ft, starts, ends))
    sc, tot, have = scores.cpu().numpy(), total.cpu().numpy(), np.isfinite(beam.cpu().numpy())
    assert have[:, 0].all() and have.sum() > len(frames)
    for b, f in enumerate(frames):
        for k in range(3):
            if not have[b, k]:
                assert np.isneginf(sc[b, k]) and (ft[b, k] == -1).all() and (st[b, k] == -1).all()
                continue
            n = ln[b, k]
            assert np.isfinite(sc[b, k])
            row = ft[b, k, :f]
            assert row[0] == 0 and row[-1] == n - 1 and set(np.diff(row).tolist()) <= {0, 1}
            assert (ft[b, k, f:] == -1).all()
            assert ((en[b, k, :n] - st[b, k, :n]) == np.bincount(row, minlength=n)).all()
            assert sc[b, k] <= tot[b, k] + 1e-4 * max(1.0, abs(tot[b, k]))
    conf = torch.exp(tsc / (ends - starts).clamp(min=1))  # the usual per-token confidence
    assert ((conf > 0) & (conf <= 1))[starts >= 0].all()
