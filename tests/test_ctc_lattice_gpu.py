"""Batched CTC scores of device-resident token lattices and their gradients (ctc_lattice.hip through
gtnx_batch_ctc_lattice_score / _grad; gtn_amd.torch_loss.ctc_lattice_score / ctc_lattice_loss, Batch.ctc_lattice_score,
gtn_ctc_lattice_score_n).

The judge is the float64 yardstick of tests/ctc_lattice_fp.py, which tests/test_ctc_lattice_cpu.py pins to the
enumeration of lattice paths, to ctc_score's yardstick and to the oracle.  The gate is the project's float64 gate: scores
within 1e-4 max(1, |score|), -inf exactly where the yardstick has it, both gradients within 1e-4 absolute for grad_out in
[-1, 1].  The cases sit at the kernel's edges (one wave, the widths, the state counts at which the states a lane works
on change, in-degrees from 0 to 511, a deep lattice); the CPU file shows that a float32 transcription of the kernel stays
inside the gate on each of them.  Bit-equality is asked wherever the contract promises it: run to run, sliced against
unsliced, one pad content against another, what lies past num_arcs, one row stride against another."""
import numpy as np
import pytest

import ctc_lattice_fp as fp

pytestmark = pytest.mark.gpu
NEG = -np.inf


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True, order="C")).to("cuda:0")


def _run(case, grad=True, arcs=None):
    """torch_loss.ctc_lattice_score on a case: (scores, d sum(gout * scores) / d emissions, the same / d arc weights or
    None) as numpy arrays"""
    import torch
    from gtn_amd import torch_loss
    x = _dev(case.em).requires_grad_(grad)
    a = _dev(case.arcs if arcs is None else arcs)
    w = None if case.weights is None else _dev(case.weights).requires_grad_(grad)
    keep = a.clone(), (None if w is None else w.detach().clone())
    out = torch_loss.ctc_lattice_score(x, a, _dev(case.num_arcs), _dev(case.num_nodes), w, blank=case.blank,
                                       input_lengths=case.frames, max_states=case.max_states)
    g = gw = None
    if grad:
        out.backward(_dev(case.gout))
        g = x.grad.cpu().numpy()
        gw = None if w is None else w.grad.cpu().numpy()
    torch.cuda.synchronize()
    assert (a == keep[0]).all() and (w is None or (w.detach().view(torch.int32) == keep[1].view(torch.int32)).all())  # only read
    return out.detach().cpu().numpy(), g, gw


def _same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and (a.view(np.uint32) == b.view(np.uint32)).all()


def _same(a, b):
    return all(_same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", fp.ALL_GPU_CASES)
def test_scores_and_gradients_against_float64(gtn, name):
    case, want = fp.case(name), fp.result(name, False)
    B, T, C = case.em.shape
    scores, grad, garc = _run(case)
    print(name, "score error", fp.score_err(scores, want.scores), "gradient error", fp.grad_err(grad, want.grad),
          "arc gradient error", None if garc is None else fp.grad_err(garc, want.garc))
    assert not np.isnan(scores).any()
    assert (np.isneginf(scores) == np.isneginf(want.scores)).all(), (scores, want.scores)
    assert fp.score_ok(scores, want.scores)
    assert np.isfinite(grad).all()
    assert fp.grad_err(grad, want.grad) <= fp.GRAD_GATE
    if garc is not None:
        assert np.isfinite(garc).all()
        assert fp.grad_err(garc, want.garc) <= fp.GRAD_GATE
        past = np.arange(case.arcs.shape[1])[None, :] >= np.clip(case.num_arcs, 0, None)[:, None]
        assert (garc[past] == 0).all(), "an entry at or past num_arcs is not 0"
    if case.frames is not None:
        for b, f in enumerate(case.frames):
            assert (grad[b, f:] == 0).all(), "a pad row has a gradient"
    # an utterance without a score, or with a weight of exactly 0, has exactly zero gradients
    for b in range(B):
        if np.isneginf(want.scores[b]) or case.gout[b] == 0:
            assert (grad[b] == 0).all() and (garc is None or (garc[b] == 0).all())


def test_a_chain_is_ctc_score_and_its_loss_ctc_loss(gtn):
    import torch
    from gtn_amd import torch_loss
    rng = np.random.default_rng(8)
    B, T, C, blank = 4, 40, 12, 0
    em = fp.continuous_case(31, B, T, C)
    hyps = [rng.integers(1, C, n).astype(np.int32) for n in (5, 20, 1, 9)]
    hyps[3][3] = hyps[3][2]  # a repeat
    arcs, na, nn_, _ = fp.pack([fp.chain_lattice(y) for y in hyps])
    tokens = np.zeros((B, 20), np.int32)
    for b, y in enumerate(hyps):
        tokens[b, :len(y)] = y
    lengths = np.array([len(y) for y in hyps], np.int32)
    x1, x2, x3, x4 = (_dev(em).requires_grad_(True) for _ in range(4))
    gout = _dev(rng.uniform(-1, 1, B).astype(np.float32))
    lat = torch_loss.ctc_lattice_score(x1, _dev(arcs), _dev(na), _dev(nn_), blank=blank)
    ref = torch_loss.ctc_score(x2, _dev(tokens), _dev(lengths), blank=blank)
    lat.backward(gout)
    ref.backward(gout)
    s, r = lat.detach().cpu().numpy().astype(np.float64), ref.detach().cpu().numpy().astype(np.float64)
    print("lattice", s, "ctc_score", r, "gradient difference", (x1.grad - x2.grad).abs().max().item())
    assert (np.abs(s - r) <= fp.SCORE_GATE * np.maximum(1.0, np.abs(r))).all()
    assert (x1.grad - x2.grad).abs().max().item() <= fp.GRAD_GATE
    loss = torch_loss.ctc_lattice_loss(x3, _dev(arcs), _dev(na), _dev(nn_), blank=blank)
    want = torch_loss.ctc_loss(x4, [h.tolist() for h in hyps], blank=blank)
    loss.backward(gout)
    want.backward(gout)
    a, b = loss.detach().cpu().numpy().astype(np.float64), want.detach().cpu().numpy().astype(np.float64)
    print("lattice loss", a, "ctc_loss", b, "gradient difference", (x3.grad - x4.grad).abs().max().item())
    assert (np.abs(a - b) <= fp.SCORE_GATE * np.maximum(1.0, np.abs(b))).all()
    assert (x3.grad - x4.grad).abs().max().item() <= fp.GRAD_GATE


def test_the_loss_of_a_padded_batch(gtn):
    """ctc_lattice_loss with input_lengths: the normaliser stops at T_b, NaN pad rows give no NaN and no gradient"""
    import torch
    from gtn_amd import torch_loss
    case, want = fp.case("ragged"), fp.result("ragged", False)
    x = _dev(case.em).requires_grad_(True)
    loss = torch_loss.ctc_lattice_loss(x, _dev(case.arcs), _dev(case.num_arcs), _dev(case.num_nodes), blank=case.blank,
                                       input_lengths=case.frames, max_states=case.max_states)
    fin = np.isfinite(want.scores)
    loss[torch.from_numpy(fin).to("cuda:0")].sum().backward()
    got = loss.detach().cpu().numpy().astype(np.float64)
    norm = np.array([np.sum(np.logaddexp.reduce(case.em[b, :f].astype(np.float64), axis=1))
                     for b, f in enumerate(case.frames)])
    assert (np.isposinf(got) == ~fin).all()
    assert (np.abs(got[fin] - (norm - want.scores)[fin]) <= fp.SCORE_GATE * np.maximum(1.0, np.abs(got[fin]))).all()
    g = x.grad.cpu().numpy()
    assert np.isfinite(g).all()
    for b, f in enumerate(case.frames):
        assert (g[b, f:] == 0).all()


@pytest.mark.parametrize("name", ["s65", "indeg8-c37", "s1024"])
def test_two_calls_give_the_same_bits(gtn, name):
    assert _same(_run(fp.case(name)), _run(fp.case(name)))


@pytest.mark.parametrize("name,utts", [("indeg8-c37", 2), ("indeg8-c37", 0), ("edges", 5)])
def test_slices_give_the_bits_of_the_unsliced_run(gtn, monkeypatch, name, utts):
    """a lowered scratch cap: the utterances run in slices (two of three; one at a time, the cap below a single
    utterance's rows; five of sixteen)"""
    case = fp.case(name)
    per_utt = 4 * case.em.shape[1] * case.max_states  # bytes of an utterance's alpha rows
    monkeypatch.delenv("GTNX_CTC_LATTICE_SCRATCH_BYTES", raising=False)
    want = _run(case)
    monkeypatch.setenv("GTNX_CTC_LATTICE_SCRATCH_BYTES", str(per_utt * utts + 64 if utts else 1000))
    assert _same(_run(case), want)


def test_pad_rows_are_never_read(gtn):
    a, b, c = _run(fp._ragged_case(np.nan)), _run(fp._ragged_case(123.0)), _run(fp._ragged_case(np.inf))
    assert _same(a, b) and _same(a, c)


def test_what_lies_past_num_arcs_is_never_read(gtn):
    case = fp.case("indeg8-c37")
    arcs = case.arcs.copy()
    past = np.arange(arcs.shape[1])[None, :] >= case.num_arcs[:, None]
    assert past.any()
    arcs[past] = np.random.default_rng(3).integers(-5, 10 ** 6, (int(past.sum()), 3))
    w = case.weights.copy()
    w[past] = np.nan
    assert _same(_run(case), _run(case._replace(weights=w), arcs=arcs))


def test_raw_addresses_a_row_stride_above_the_width_and_the_counter(gtn):
    import torch
    case = fp.case("indeg8-c37")
    B, T, C = case.em.shape
    A = case.arcs.shape[1]
    want = _run(case)
    wide = np.zeros((B, 3 * A + 7), dtype=np.int32)  # (valid arcs of label 0 behind the rows: they would count if read)
    wide[:, 1::3] = 1
    wide[:, :3 * A] = case.arcs.reshape(B, 3 * A)
    x, arcs, w = _dev(case.em), _dev(wide), _dev(case.weights)
    na, nn_, gout = _dev(case.num_arcs), _dev(case.num_nodes), _dev(case.gout)
    scores = torch.full((B + 2,), 5.0, device="cuda:0")
    grad = torch.full((B * T * C + 2,), 5.0, device="cuda:0")
    garc = torch.full((B * A + 2,), 5.0, device="cuda:0")
    ems = gtn.Batch.linear(B, T, C, x, calc_grad=False, borrow=True)
    c0 = gtn.debug_ctc_lattice_score_stats()
    ems.ctc_lattice_score(arcs.data_ptr(), na.data_ptr(), nn_.data_ptr(), scores[1:].data_ptr(), w.data_ptr(), None,
                          case.blank, case.max_states, A=A, row_stride=3 * A + 7)
    c1 = gtn.debug_ctc_lattice_score_stats()
    ems.ctc_lattice_score_grad(arcs.data_ptr(), na.data_ptr(), nn_.data_ptr(), gout.data_ptr(), grad[1:].data_ptr(),
                               garc[1:].data_ptr(), w.data_ptr(), None, case.blank, case.max_states, A=A,
                               row_stride=3 * A + 7)
    gtn.synchronize()
    c2 = gtn.debug_ctc_lattice_score_stats()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, B) and (c2[0] - c1[0], c2[1] - c1[1]) == (1, B)
    s, g, ga = scores.cpu().numpy(), grad.cpu().numpy(), garc.cpu().numpy()
    assert s[0] == 5.0 and s[-1] == 5.0 and g[0] == 5.0 and g[-1] == 5.0 and ga[0] == 5.0 and ga[-1] == 5.0, "guards"
    assert _same_bits(s[1:-1], want[0]) and _same_bits(g[1:-1].reshape(B, T, C), want[1])
    assert _same_bits(ga[1:-1].reshape(B, A), want[2])
    assert (arcs.cpu().numpy() == wide).all() and _same_bits(w.cpu().numpy(), case.weights)  # only read
    # the same through tensors, and without the arcs' gradient: the emission gradient has the same bits
    s2 = torch.empty(B, device="cuda:0")
    g2 = torch.empty(B, T, C, device="cuda:0")
    ems.ctc_lattice_score(_dev(case.arcs), na, nn_, s2, w, blank=case.blank, max_states=case.max_states)
    ems.ctc_lattice_score_grad(_dev(case.arcs), na, nn_, gout, g2, None, w, blank=case.blank, max_states=case.max_states)
    gtn.synchronize()
    assert _same_bits(s2.cpu().numpy(), want[0]) and _same_bits(g2.cpu().numpy(), want[1])


def test_invalid_lattices_leave_their_neighbours_bits_alone(gtn):
    """the utterances of the edges case one by one against the whole batch: -inf and zeros beside valid ones"""
    case = fp.case("edges")
    whole = _run(case)
    fin = np.isfinite(fp.result("edges", False).scores)
    assert (np.isneginf(whole[0]) == ~fin).all()
    valid = np.nonzero(fin)[0]
    alone = _run(fp.Case(case.em[valid], case.arcs[valid], case.num_arcs[valid], case.num_nodes[valid],
                         case.weights[valid], case.blank, None, case.max_states, case.gout[valid]))
    assert _same_bits(alone[0], whole[0][valid]) and _same_bits(alone[1], whole[1][valid])
    assert _same_bits(alone[2], whole[2][valid])
    assert (whole[1][~fin] == 0).all() and (whole[2][~fin] == 0).all()


def test_without_requires_grad_nothing_but_the_forward_launches(gtn):
    import torch
    from gtn_amd import torch_loss
    case = fp.case("edges")
    B = case.em.shape[0]
    c0 = gtn.debug_ctc_lattice_score_stats()
    _run(case, grad=False)
    c1 = gtn.debug_ctc_lattice_score_stats()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, B)
    _run(case, grad=True)
    c2 = gtn.debug_ctc_lattice_score_stats()
    assert (c2[0] - c1[0], c2[1] - c1[1]) == (2, 2 * B)
    # weights that require no gradient get none; a lattice without an arc row at all (A == 0) scores its blanks
    x = _dev(case.em[:2]).requires_grad_(True)
    out = torch_loss.ctc_lattice_score(x, torch.zeros(2, 0, 3, dtype=torch.int32, device="cuda:0"),
                                       torch.zeros(2, dtype=torch.int64, device="cuda:0"),
                                       torch.tensor([1, 2], dtype=torch.int64, device="cuda:0"), blank=case.blank)
    out[0].backward()
    want = float(np.sum(case.em[0, :, case.blank].astype(np.float64)))
    assert abs(out[0].item() - want) <= fp.SCORE_GATE * max(1.0, abs(want)) and out[1].item() == NEG
    assert (x.grad[1] == 0).all() and x.grad[0].sum().item() == pytest.approx(case.em.shape[1], abs=1e-3)


def test_what_needs_the_device_is_refused_there(gtn):
    """not a native linear batch, a frame count outside 0 .. M, blank >= C: invalid arguments, nothing is launched"""
    import torch
    case = fp.case("edges")
    B, T, C = case.em.shape
    x, arcs, na, nn_ = _dev(case.em), _dev(case.arcs), _dev(case.num_arcs), _dev(case.num_nodes)
    out = torch.zeros(B, device="cuda:0")
    ems = gtn.Batch.linear(B, T, C, x, calc_grad=False, borrow=True)
    c0 = gtn.debug_ctc_lattice_score_stats()
    with pytest.raises(ValueError, match="frame count outside"):
        ems.ctc_lattice_score(arcs, na, nn_, out, frames=[T + 1] + [1] * (B - 1))
    with pytest.raises(ValueError, match="blank is not below"):
        ems.ctc_lattice_score(arcs, na, nn_, out, blank=C)
    with pytest.raises(ValueError, match="not a native linear batch"):
        gtn.Batch([gtn.linear_graph(T, C) for _ in range(B)]).ctc_lattice_score(arcs, na, nn_, out)
    gtn.synchronize()
    assert gtn.debug_ctc_lattice_score_stats() == c0 and (out == 0).all()


def test_the_word_piece_training_step(gtn):
    """decomposition_lattice -> pack_lattices -> ctc_lattice_loss -> backward with learned arc weights: the loss and both
    gradients against float64"""
    import torch
    import gtn_amd
    from gtn_amd import torch_loss
    pieces = fp.the_pieces()
    words = ["the", "thee", "he", "tthe"]
    arcs, na, nn_, _ = gtn_amd.pack_lattices([gtn_amd.decomposition_lattice(wd, pieces) for wd in words])
    B, T, C, blank = len(words), 12, 7, 6
    em = fp.continuous_case(5, B, T, C)
    rng = np.random.default_rng(6)
    piece_score = rng.normal(0.0, 1.0, C).astype(np.float32)  # one learned score per piece
    theta = _dev(piece_score).requires_grad_(True)
    x = _dev(em).requires_grad_(True)
    a = _dev(arcs)
    w = theta[a[:, :, 2].long()]  # [B, A]: the weight of an arc is the score of its piece
    loss = torch_loss.ctc_lattice_loss(x, a, _dev(na), _dev(nn_), w, blank=blank)
    loss.sum().backward()
    want_theta = np.zeros(C)
    for b in range(B):
        n = na[b]
        s, d, l = (arcs[b, :n, i].astype(np.int64) for i in range(3))
        z, g, ga = fp.lattice_fp64(em[b], s, d, l, piece_score[l].astype(np.float64), int(nn_[b]), blank)
        norm = float(np.sum(np.logaddexp.reduce(em[b].astype(np.float64), axis=1)))
        assert abs(loss[b].item() - (norm - z)) <= fp.SCORE_GATE * max(1.0, abs(norm - z))
        soft = np.exp(em[b].astype(np.float64) - np.logaddexp.reduce(em[b].astype(np.float64), axis=1)[:, None])
        assert np.abs(x.grad[b].cpu().numpy() - (soft - g)).max() <= fp.GRAD_GATE
        np.add.at(want_theta, l, -ga)
    print("piece gradient", theta.grad.cpu().numpy(), want_theta)
    # (a piece's gradient is the sum of its arcs' gradients over the batch, each within the gate)
    uses = np.bincount(np.concatenate([arcs[b, :na[b], 2] for b in range(B)]), minlength=C)
    assert (np.abs(theta.grad.cpu().numpy() - want_theta) <= np.maximum(uses, 1) * fp.GRAD_GATE).all()
