"""Batched CTC scores of device-resident hypotheses and their weighted gradient (ctc_score.hip through
gtnx_batch_ctc_score / _grad; gtn_amd.torch_loss.ctc_score, Batch.ctc_score, gtn_ctc_score_n).

The judge is the float64 yardstick of tests/ctc_score_fp.py, which tests/test_ctc_score_cpu.py pins to an enumeration of
alignments, to ctc_loss_fp64 and to the oracle.  The gate is the project's float64 gate: scores within 1e-4 max(1,
|score|), -inf exactly where the yardstick has it, gradients within 1e-4 absolute for weights in [-1, 1].  The cases sit
at the kernel's edges (one wave, the widths, the lengths at which the states a lane works on change); the CPU file shows
that a float32 transcription of the kernel stays inside the gate on each of them.  Bit-equality is asked wherever the
contract promises it: run to run, sliced against unsliced, one pad content against another, one form against another."""
import numpy as np
import pytest

import ctc_score_fp as fp

pytestmark = pytest.mark.gpu
NEG = -np.inf


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True, order="C")).to("cuda:0")


def _run(case, grad=True, tokens=None, lengths=None):
    """torch_loss.ctc_score on a case: (scores, gradient of sum(weights * scores) or None) as numpy arrays"""
    import torch
    from gtn_amd import torch_loss
    x = _dev(case.em).requires_grad_(grad)
    tok = _dev(case.tokens) if tokens is None else tokens
    ln = _dev(case.lengths) if lengths is None else lengths
    out = torch_loss.ctc_score(x, tok, ln, blank=case.blank, input_lengths=case.frames, max_length=case.max_length)
    g = None
    if grad:
        out.backward(_dev(case.weights).reshape(out.shape))
        g = x.grad.cpu().numpy()
    torch.cuda.synchronize()
    assert (tok.cpu().numpy() == (case.tokens if tokens is None else tokens.cpu().numpy())).all()  # only read
    return out.detach().cpu().numpy(), g


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and (a.view(np.uint32) == b.view(np.uint32)).all()


@pytest.mark.parametrize("name", fp.ALL_GPU_CASES)
def test_scores_and_gradients_against_float64(gtn, name):
    case, want = fp.case(name), fp.result(name, False)
    B, T, C = case.em.shape
    scores, grad = _run(case)
    scores = scores.reshape(want.scores.shape)
    print(name, "score error", fp.score_err(scores, want.scores), "gradient error", fp.grad_err(grad, want.grad))
    assert not np.isnan(scores).any()
    assert (np.isneginf(scores) == np.isneginf(want.scores)).all(), (scores, want.scores)
    assert fp.score_ok(scores, want.scores)
    assert np.isfinite(grad).all()
    assert fp.grad_err(grad, want.grad) <= fp.GRAD_GATE
    if case.frames is not None:
        for b, f in enumerate(case.frames):
            assert (grad[b, f:] == 0).all(), "a pad row has a gradient"
    # a pair without a score, or with a weight of exactly 0, adds nothing: utterances made of such pairs stay 0
    dead = np.isneginf(want.scores) | (np.asarray(case.weights).reshape(want.scores.shape) == 0)
    for b in range(B):
        if dead[b].all():
            assert (grad[b] == 0).all()


def test_pad_rows_are_never_read(gtn):
    a = _run(fp._ragged_case(np.nan))
    b = _run(fp._ragged_case(123.0))
    c = _run(fp._ragged_case(np.inf))
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])
    assert _same_bits(a[0], c[0]) and _same_bits(a[1], c[1])


def test_elements_past_a_length_are_never_read(gtn):
    case = fp.case("c37-holes")
    tok = case.tokens.copy()
    L = tok.shape[-1]
    past = np.arange(L)[None, None, :] >= np.asarray(case.lengths)[:, :, None]
    tok[past] = np.random.default_rng(3).integers(-5, 10 ** 6, int(past.sum()))
    a, b = _run(case), _run(case._replace(tokens=tok))
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])


@pytest.mark.parametrize("name", ["lens-c5", "c37-holes", "wide-u1023"])
def test_two_calls_give_the_same_bits(gtn, name):
    a, b = _run(fp.case(name)), _run(fp.case(name))
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])


def test_flat_form_and_int64_lengths(gtn):
    case = fp.case("c2-repeats")  # N = 1
    a = _run(case)
    tok, ln = _dev(case.tokens[:, 0]), _dev(case.lengths[:, 0].astype(np.int64))
    b = _run(case, tokens=tok, lengths=ln)
    assert b[0].shape == (7,) and _same_bits(a[0].reshape(7), b[0]) and _same_bits(a[1], b[1])
    c = _run(fp.case("lens-c5"), lengths=_dev(fp.case("lens-c5").lengths.astype(np.int64)))
    d = _run(fp.case("lens-c5"))
    assert _same_bits(c[0], d[0]) and _same_bits(c[1], d[1])


def test_raw_addresses_and_a_row_stride_above_the_width(gtn):
    import torch
    case = fp.case("c37-holes")
    B, T, C = case.em.shape
    N, L = case.tokens.shape[1:]
    want = _run(case)
    wide = np.full((B, N, L + 5), 7, dtype=np.int32)  # (valid labels behind the rows: they would count if read)
    wide[:, :, :L] = case.tokens
    x, tok, ln = _dev(case.em), _dev(wide), _dev(case.lengths.astype(np.int32))
    w = _dev(case.weights)
    scores = torch.full((B * N + 2,), 5.0, device="cuda:0")
    grad = torch.full((B * T * C + 2,), 5.0, device="cuda:0")
    ems = gtn.Batch.linear(B, T, C, x, calc_grad=False, borrow=True)
    c0 = gtn.debug_ctc_score_stats()
    ems.ctc_score(tok.data_ptr(), ln.data_ptr(), scores[1:].data_ptr(), None, case.blank, None, N=N, L=L,
                  row_stride=L + 5)
    ems.ctc_score_grad(tok.data_ptr(), ln.data_ptr(), w.data_ptr(), grad[1:].data_ptr(), None, case.blank, None, N=N,
                       L=L, row_stride=L + 5)
    gtn.synchronize()
    c1 = gtn.debug_ctc_score_stats()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (2, 2 * B * N)
    s, g = scores.cpu().numpy(), grad.cpu().numpy()
    assert s[0] == 5.0 and s[-1] == 5.0 and g[0] == 5.0 and g[-1] == 5.0, "guards"
    assert _same_bits(s[1:-1].reshape(B, N), want[0]) and _same_bits(g[1:-1].reshape(B, T, C), want[1])
    # the same through tensors: a view whose rows are further apart than they are wide
    s2 = torch.empty(B, N, device="cuda:0")
    ems.ctc_score(tok[:, :, :L], ln, s2, blank=case.blank)
    gtn.synchronize()
    assert _same_bits(s2.cpu().numpy(), want[0])


@pytest.mark.parametrize("name,pairs", [("lens-c5", 2), ("lens-c5", 0), ("c37-holes", 5)])
def test_slices_give_the_bits_of_the_unsliced_run(gtn, monkeypatch, name, pairs):
    """a lowered scratch cap: the pairs run in slices that cut utterances apart (two pairs of three; one pair, the cap
    below a single pair's rows; five of four)"""
    case = fp.case(name)
    per_pair = 4 * case.em.shape[1] * (2 * fp.default_max_length(case) + 1)  # bytes of a pair's alpha rows
    monkeypatch.delenv("GTNX_CTC_SCORE_SCRATCH_BYTES", raising=False)
    want = _run(case)
    monkeypatch.setenv("GTNX_CTC_SCORE_SCRATCH_BYTES", str(per_pair * pairs + 64 if pairs else 1000))
    got = _run(case)
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])


def test_without_requires_grad_nothing_but_the_forward_launches(gtn):
    import torch
    case = fp.case("edges")
    c0 = gtn.debug_ctc_score_stats()
    _run(case, grad=False)
    c1 = gtn.debug_ctc_score_stats()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, 12)
    _run(case, grad=True)
    c2 = gtn.debug_ctc_score_stats()
    assert (c2[0] - c1[0], c2[1] - c1[1]) == (2, 24)
    # no pairs at all: nothing launches, the gradient is zeros
    from gtn_amd import torch_loss
    x = _dev(case.em).requires_grad_(True)
    out = torch_loss.ctc_score(x, torch.zeros(3, 0, 8, dtype=torch.int32, device="cuda:0"),
                               torch.zeros(3, 0, dtype=torch.int32, device="cuda:0"))
    assert out.shape == (3, 0)
    out.sum().backward()
    assert (x.grad == 0).all() and gtn.debug_ctc_score_stats() == c2


def test_what_needs_the_device_is_refused_there(gtn):
    """not a native linear batch, a frame count outside 0 .. M, blank >= C: invalid arguments, nothing is launched"""
    import torch
    case = fp.case("edges")
    B, T, C = case.em.shape
    x, tok, ln = _dev(case.em), _dev(case.tokens), _dev(case.lengths)
    out = torch.zeros(B, 4, device="cuda:0")
    ems = gtn.Batch.linear(B, T, C, x, calc_grad=False, borrow=True)
    c0 = gtn.debug_ctc_score_stats()
    with pytest.raises(ValueError, match="frame count outside"):
        ems.ctc_score(tok, ln, out, frames=[T + 1, 1, 1])
    with pytest.raises(ValueError, match="frame count outside"):
        ems.ctc_score(tok, ln, out, frames=[-1, 1, 1])
    with pytest.raises(ValueError, match="blank is not below"):
        ems.ctc_score(tok, ln, out, blank=C)
    with pytest.raises(ValueError, match="not a native linear batch"):
        gtn.Batch([gtn.linear_graph(T, C) for _ in range(B)]).ctc_score(tok, ln, out)
    gtn.synchronize()
    assert gtn.debug_ctc_score_stats() == c0 and (out == 0).all()


def test_score_is_the_normaliser_minus_ctc_loss(gtn):
    """ctc_loss(x, [y]) == forwardScore(x) - ctc_score(x, y): the route the parent commit offers"""
    import torch
    from gtn_amd import torch_loss
    rng = np.random.default_rng(8)
    B, T, C, blank = 3, 40, 12, 0
    em = fp.continuous_case(31, B, T, C)
    hyps = [fp.tokens_of(rng, n, C, blank, "random") for n in (5, 20, 1)]
    tokens, lengths = fp.pack(hyps, B, 1, 24)
    x = _dev(em)
    score = torch_loss.ctc_score(x, _dev(tokens), _dev(lengths), blank=blank).reshape(B).cpu().numpy().astype(np.float64)
    loss = torch_loss.ctc_loss(x, [h.tolist() for h in hyps], blank=blank).cpu().numpy().astype(np.float64)
    norm = torch.logsumexp(x.double(), dim=2).sum(dim=1).cpu().numpy()
    print("score", score, "normaliser - loss", norm - loss)
    assert (np.abs(score - (norm - loss)) <= fp.SCORE_GATE * np.maximum(1.0, np.abs(score))).all()


def test_an_unpruned_beam_scores_the_same(gtn):
    import torch
    from gtn_amd import torch_loss
    em = fp.continuous_case(5, 2, 3, 3)
    x = _dev(em)
    tokens, lengths, beam = torch_loss.ctc_beam_decode(x, blank=0, beam_size=64, cutoff_top_n=3, nbest=8)
    score = torch_loss.ctc_score(x, tokens, lengths, blank=0)
    beam, score = beam.cpu().numpy().astype(np.float64), score.cpu().numpy().astype(np.float64)
    have = np.isfinite(beam)
    assert have.sum() >= 10 and np.isfinite(score).all()  # (a slot without a hypothesis scores as the empty sequence)
    print("beam", beam[have], "score", score[have])
    assert (np.abs(beam[have] - score[have]) <= fp.SCORE_GATE * np.maximum(1.0, np.abs(score[have]))).all()


def test_the_mwer_chain(gtn):
    """ctc_beam_decode -> ctc_score -> edit_distance -> softmax-weighted risk -> backward, nothing downloaded on the
    way; the gradient equals the float64 chain over the same hypotheses"""
    import torch
    from gtn_amd import torch_loss
    B, T, C, blank, nbest = 3, 30, 12, 0, 4
    em = fp.continuous_case(77, B, T, C)
    rng = np.random.default_rng(4)
    refs = [fp.tokens_of(rng, n, C, blank, "random") for n in (6, 9, 4)]
    ref, ref_len = fp.pack(refs, B, 1, 12)
    x = _dev(em).requires_grad_(True)
    tokens, lengths, beam = torch_loss.ctc_beam_decode(x, blank=blank, beam_size=8, cutoff_top_n=6, nbest=nbest)
    score = torch_loss.ctc_score(x, tokens, lengths, blank=blank, max_length=T)
    score = torch.where(beam == NEG, beam, score)  # (slots without a hypothesis)
    err = torch_loss.edit_distance(tokens, lengths, _dev(ref[:, 0]), _dev(ref_len[:, 0])).float()
    p = torch.softmax(score, dim=1)
    risk = (p * (err - err.mean(dim=1, keepdim=True))).sum()
    risk.backward()
    grad = x.grad.cpu().numpy()
    assert np.isfinite(grad).all() and np.isfinite(risk.item())
    # the float64 chain over the same hypotheses
    tk, ln, e = tokens.cpu().numpy(), lengths.cpu().numpy(), err.cpu().numpy().astype(np.float64)
    have = np.isfinite(beam.cpu().numpy())
    assert have[:, 0].all()
    want, want_risk = np.zeros((B, T, C)), 0.0
    for b in range(B):
        pairs = [fp.pair_fp64(em[b], tk[b, k, :ln[b, k]], blank) for k in range(nbest)]
        z = np.array([s if have[b, k] else NEG for k, (s, _) in enumerate(pairs)])
        pk = np.exp(z - np.max(z))
        pk /= pk.sum()
        d = e[b] - e[b].mean()
        want_risk += float(np.sum(pk * d))
        for k in range(nbest):
            if have[b, k]:
                want[b] += pk[k] * (d[k] - np.sum(pk * d)) * pairs[k][1]
    print("risk", risk.item(), want_risk, "gradient error", np.abs(grad - want).max(), "largest", np.abs(want).max())
    assert abs(risk.item() - want_risk) <= 1e-4 * max(1.0, abs(want_risk))
    assert np.abs(grad - want).max() <= 1e-4
    assert np.abs(want).max() > 1e-3  # (the chain has a gradient to speak of)
