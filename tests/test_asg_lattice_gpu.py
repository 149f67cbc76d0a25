"""Batched ASG scores of device-resident token lattices and their gradients (asg_lattice.hip through
gtnx_batch_asg_lattice_score / _grad; gtn_amd.torch_loss.asg_lattice_score / asg_full_connect / asg_lattice_loss,
Batch.asg_lattice_score, gtn_asg_lattice_score_n).

The judge is the float64 yardstick of tests/asg_lattice_fp.py, which tests/test_asg_lattice_cpu.py pins to the
enumeration of lattice paths, to asg_score's yardstick and to the oracle.  The gates are the project's (asg_score_fp):
scores within 1e-4 max(1, |score|), -inf exactly where the yardstick has it, emission and arc gradients within 1e-4
absolute for grad_out in [-1, 1], the table gradient within 1e-4 max(1, |want|) per entry.  The cases sit at the kernel's
edges (one wave, the widths, the state counts at which the arcs a lane works on change, in-degrees from 0 to 511 with
1.83 M edges, max_edges met and missed by one, a deep lattice); the CPU file shows that a float32 transcription of the
kernel stays inside the gates on each of them.  Bit-equality is asked wherever the contract promises it: run to run,
sliced against unsliced (table gradient included), one pad content against another, what lies past num_arcs, one row
stride against another, one gradient alone against all three."""
import numpy as np
import pytest

import asg_lattice_fp as fp

pytestmark = pytest.mark.gpu
NEG = -np.inf


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True, order="C")).to("cuda:0")


def _run(case, grad=("em", "table", "arc"), arcs=None):
    """torch_loss.asg_lattice_score on a case: (scores, d sum(gout * scores) / d emissions, the same / d table [C + C *
    C], the same / d arc weights) as numpy arrays, None for what `grad` leaves out or the case has not"""
    import torch
    from gtn_amd import torch_loss
    x = _dev(case.em).requires_grad_("em" in grad)
    tr = _dev(case.trans).requires_grad_("table" in grad)
    st = _dev(case.start).requires_grad_("table" in grad)
    a = _dev(case.arcs if arcs is None else arcs)
    w = None if case.weights is None else _dev(case.weights).requires_grad_("arc" in grad)
    keep = [t.detach().clone() for t in (x, tr, st, a)] + [None if w is None else w.detach().clone()]
    out = torch_loss.asg_lattice_score(x, tr, a, _dev(case.num_arcs), _dev(case.num_nodes), w, start=st,
                                       input_lengths=case.frames, max_states=case.max_states, max_edges=case.max_edges)
    g = gt = gw = None
    if grad and (out.requires_grad):
        out.backward(_dev(case.gout))
        g = x.grad.cpu().numpy() if "em" in grad else None
        gt = np.concatenate([st.grad.cpu().numpy(), tr.grad.cpu().numpy().reshape(-1)]) if "table" in grad else None
        gw = w.grad.cpu().numpy() if w is not None and "arc" in grad else None
    torch.cuda.synchronize()
    for t, k in zip((x, tr, st, a, w), keep):  # the inputs are only read
        assert t is None or (t.detach().view(torch.int32) == k.view(torch.int32)).all()
    return out.detach().cpu().numpy(), g, gt, gw


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
    scores, grad, gtable, garc = _run(case)
    print(name, "score error", fp.score_err(scores, want.scores), "gradient error", fp.grad_err(grad, want.grad),
          "table gradient error", fp.table_err(gtable, want.gtable),
          "arc gradient error", None if garc is None else fp.grad_err(garc, want.garc))
    assert not np.isnan(scores).any()
    assert (np.isneginf(scores) == np.isneginf(want.scores)).all(), (scores, want.scores)
    assert fp.score_ok(scores, want.scores)
    assert np.isfinite(grad).all() and np.isfinite(gtable).all()
    assert fp.grad_err(grad, want.grad) <= fp.GRAD_GATE
    assert fp.table_err(gtable, want.gtable) <= fp.TABLE_GATE
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


def test_a_chain_is_asg_score_and_its_loss_asg_loss(gtn):
    import torch
    from gtn_amd import torch_loss
    rng = np.random.default_rng(8)
    B, T, C = 4, 30, 7
    em, trans, start = fp.model_of(rng, B, T, C)
    hyps = [rng.integers(0, C, n).astype(np.int32) for n in (5, 20, 1, 9)]
    hyps[3][3] = hyps[3][2]  # a repeat
    arcs, na, nn_, _ = fp.pack([fp.chain_lattice(y) for y in hyps])
    tokens = np.zeros((B, 20), np.int32)
    for b, y in enumerate(hyps):
        tokens[b, :len(y)] = y
    lengths = np.array([len(y) for y in hyps], np.int32)

    def leaves():
        return (_dev(em).requires_grad_(True), _dev(trans).requires_grad_(True), _dev(start).requires_grad_(True))

    def table_grad(tr, st):
        return np.concatenate([st.grad.cpu().numpy(), tr.grad.cpu().numpy().reshape(-1)])
    gout = _dev(rng.uniform(-1, 1, B).astype(np.float32))
    (x1, tr1, st1), (x2, tr2, st2) = leaves(), leaves()
    lat = torch_loss.asg_lattice_score(x1, tr1, _dev(arcs), _dev(na), _dev(nn_), start=st1)
    ref = torch_loss.asg_score(x2, tr2, _dev(tokens), _dev(lengths), start=st2)
    lat.backward(gout)
    ref.backward(gout)
    s, r = lat.detach().cpu().numpy().astype(np.float64), ref.detach().cpu().numpy().astype(np.float64)
    terr = fp.table_err(table_grad(tr1, st1), table_grad(tr2, st2).astype(np.float64))
    print("lattice", s, "asg_score", r, "gradient difference", (x1.grad - x2.grad).abs().max().item(), "table", terr)
    assert (np.abs(s - r) <= fp.SCORE_GATE * np.maximum(1.0, np.abs(r))).all()
    assert (x1.grad - x2.grad).abs().max().item() <= fp.GRAD_GATE
    assert terr <= fp.TABLE_GATE
    (x3, tr3, st3), (x4, tr4, st4) = leaves(), leaves()
    loss = torch_loss.asg_lattice_loss(x3, tr3, _dev(arcs), _dev(na), _dev(nn_), start=st3)
    want = torch_loss.asg_loss(x4, tr4, [h.tolist() for h in hyps], start=st4)
    loss.sum().backward()
    want.sum().backward()
    a, b = loss.detach().cpu().numpy().astype(np.float64), want.detach().cpu().numpy().astype(np.float64)
    terr = fp.table_err(table_grad(tr3, st3), table_grad(tr4, st4).astype(np.float64))
    print("lattice loss", a, "asg_loss", b, "gradient difference", (x3.grad - x4.grad).abs().max().item(), "table", terr)
    assert (np.abs(a - b) <= fp.SCORE_GATE * np.maximum(1.0, np.abs(b))).all()
    assert (x3.grad - x4.grad).abs().max().item() <= fp.GRAD_GATE
    assert terr <= fp.TABLE_GATE


def test_the_full_connect_term_and_the_loss_of_a_padded_batch(gtn):
    """asg_full_connect with input_lengths against float64; asg_lattice_loss is +inf where the score is -inf; a
    non-uniform upstream gradient is refused for the table under reduction="none" """
    import torch
    from asg_loss_fp import asg_terms_fp64
    from gtn_amd import torch_loss
    case, want = fp.case("ragged"), fp.result("ragged", False)
    B, T, C = case.em.shape
    frames = [max(f, 1) for f in case.frames]
    x = _dev(np.nan_to_num(case.em, nan=0.0)).requires_grad_(True)
    tr, st = _dev(case.trans).requires_grad_(True), _dev(case.start).requires_grad_(True)
    fcc = torch_loss.asg_full_connect(x, tr, start=st, input_lengths=frames)
    ref = np.array([asg_terms_fp64(np.nan_to_num(case.em[b, :f], nan=0.0), case.trans, case.start, [0])["fcc"]
                    for b, f in enumerate(frames)])
    got = fcc.detach().cpu().numpy().astype(np.float64)
    print("full-connect", got, ref)
    assert (np.abs(got - ref) <= fp.SCORE_GATE * np.maximum(1.0, np.abs(ref))).all()
    with pytest.raises(RuntimeError, match="uniform upstream"):
        fcc.backward(_dev(case.gout))
    loss = torch_loss.asg_lattice_loss(x, tr, _dev(case.arcs), _dev(case.num_arcs), _dev(case.num_nodes), start=st,
                                       input_lengths=frames, max_states=case.max_states)
    fin = np.isfinite(want.scores) & (np.array(case.frames) >= 1)
    got = loss.detach().cpu().numpy().astype(np.float64)
    assert np.isposinf(got[~np.isfinite(want.scores) & (np.array(case.frames) >= 1)]).all()
    assert (np.abs(got[fin] - (ref - want.scores)[fin]) <= fp.SCORE_GATE * np.maximum(1.0, np.abs(got[fin]))).all()


@pytest.mark.parametrize("name", ["s65", "indeg8-c37", "s1024"])
def test_two_calls_give_the_same_bits(gtn, name):
    assert _same(_run(fp.case(name)), _run(fp.case(name)))


@pytest.mark.parametrize("name,utts", [("indeg8-c37", 2), ("indeg8-c37", 0), ("edges", 5)])
def test_slices_give_the_bits_of_the_unsliced_run(gtn, monkeypatch, name, utts):
    """a lowered scratch cap: the utterances run in slices (two of three; one at a time, the cap below a single
    utterance's rows; five of twenty), and the table launch of a slice carries on from the one before"""
    case = fp.case(name)
    per_utt = 4 * (case.em.shape[1] * case.max_states + fp.max_edges_of(case) + 5 * case.max_states)  # bytes
    monkeypatch.delenv("GTNX_ASG_LATTICE_SCRATCH_BYTES", raising=False)
    want = _run(case)
    monkeypatch.setenv("GTNX_ASG_LATTICE_SCRATCH_BYTES", str(per_utt * utts + 64 if utts else 1000))
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


@pytest.mark.parametrize("only", ["em", "table", "arc"])
def test_each_gradient_alone_has_the_bits_of_all_three(gtn, only):
    case = fp.case("indeg8-c37")
    whole = _run(case)
    alone = _run(case, grad=(only,))
    index = {"em": 1, "table": 2, "arc": 3}[only]
    assert _same_bits(alone[0], whole[0]) and _same_bits(alone[index], whole[index])
    assert all(alone[i] is None for i in (1, 2, 3) if i != index)


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
    table = _dev(fp.table_of(case.start, case.trans))
    na, nn_, gout = _dev(case.num_arcs), _dev(case.num_nodes), _dev(case.gout)
    scores = torch.full((B + 2,), 5.0, device="cuda:0")
    grad = torch.full((B * T * C + 2,), 5.0, device="cuda:0")
    gtab = torch.full((C + C * C + 2,), 5.0, device="cuda:0")
    garc = torch.full((B * A + 2,), 5.0, device="cuda:0")
    ems = gtn.Batch.linear(B, T, C, x, calc_grad=False, borrow=True)
    c0 = gtn.debug_asg_lattice_score_stats()
    ems.asg_lattice_score(table.data_ptr(), arcs.data_ptr(), na.data_ptr(), nn_.data_ptr(), scores[1:].data_ptr(),
                          w.data_ptr(), None, case.max_states, None, A=A, row_stride=3 * A + 7)
    c1 = gtn.debug_asg_lattice_score_stats()
    ems.asg_lattice_score_grad(table.data_ptr(), arcs.data_ptr(), na.data_ptr(), nn_.data_ptr(), gout.data_ptr(),
                               grad[1:].data_ptr(), gtab[1:].data_ptr(), garc[1:].data_ptr(), w.data_ptr(), None,
                               case.max_states, None, A=A, row_stride=3 * A + 7)
    gtn.synchronize()
    c2 = gtn.debug_asg_lattice_score_stats()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, B) and (c2[0] - c1[0], c2[1] - c1[1]) == (1, B)
    s, g, gt, ga = scores.cpu().numpy(), grad.cpu().numpy(), gtab.cpu().numpy(), garc.cpu().numpy()
    for guarded in (s, g, gt, ga):
        assert guarded[0] == 5.0 and guarded[-1] == 5.0, "guards"
    assert _same_bits(s[1:-1], want[0]) and _same_bits(g[1:-1].reshape(B, T, C), want[1])
    assert _same_bits(gt[1:-1], want[2]) and _same_bits(ga[1:-1].reshape(B, A), want[3])
    assert (arcs.cpu().numpy() == wide).all() and _same_bits(w.cpu().numpy(), case.weights)  # only read
    # the same through tensors, with the emission gradient alone
    s2 = torch.empty(B, device="cuda:0")
    g2 = torch.empty(B, T, C, device="cuda:0")
    ems.asg_lattice_score(table, _dev(case.arcs), na, nn_, s2, w, max_states=case.max_states)
    ems.asg_lattice_score_grad(table, _dev(case.arcs), na, nn_, gout, g2, arc_weights=w, max_states=case.max_states)
    gtn.synchronize()
    assert _same_bits(s2.cpu().numpy(), want[0]) and _same_bits(g2.cpu().numpy(), want[1])


def test_invalid_lattices_leave_their_neighbours_bits_alone(gtn):
    """the utterances of the edges case one by one against the whole batch: -inf and zeros beside valid ones"""
    case = fp.case("edges")
    whole = _run(case)
    fin = np.isfinite(fp.result("edges", False).scores)
    assert (np.isneginf(whole[0]) == ~fin).all()
    valid = np.nonzero(fin)[0]
    alone = _run(case._replace(em=case.em[valid], arcs=case.arcs[valid], num_arcs=case.num_arcs[valid],
                               num_nodes=case.num_nodes[valid], weights=case.weights[valid],
                               frames=tuple(case.frames[b] for b in valid), gout=case.gout[valid]))
    assert _same_bits(alone[0], whole[0][valid]) and _same_bits(alone[1], whole[1][valid])
    assert _same_bits(alone[2], whole[2]) and _same_bits(alone[3], whole[3][valid])  # (the table: they add nothing)
    assert (whole[1][~fin] == 0).all() and (whole[3][~fin] == 0).all()


def test_without_requires_grad_nothing_but_the_forward_launches(gtn):
    import torch
    from gtn_amd import torch_loss
    case = fp.case("edges")
    B = case.em.shape[0]
    c0 = gtn.debug_asg_lattice_score_stats()
    _run(case, grad=())
    c1 = gtn.debug_asg_lattice_score_stats()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, B)
    _run(case)
    c2 = gtn.debug_asg_lattice_score_stats()
    assert (c2[0] - c1[0], c2[1] - c1[1]) == (2, 2 * B)
    # a lattice without an arc row at all (A == 0) has no alignment, and zero gradients
    x = _dev(case.em[:2]).requires_grad_(True)
    out = torch_loss.asg_lattice_score(x, _dev(case.trans), torch.zeros(2, 0, 3, dtype=torch.int32, device="cuda:0"),
                                       torch.zeros(2, dtype=torch.int64, device="cuda:0"),
                                       torch.tensor([1, 2], dtype=torch.int64, device="cuda:0"))
    out.sum().backward()
    assert out.tolist() == [NEG, NEG] and (x.grad == 0).all()


def test_what_needs_the_device_is_refused_there(gtn):
    """not a native linear batch, a frame count outside 0 .. M, a table in host memory: nothing is launched"""
    import torch
    case = fp.case("edges")
    B, T, C = case.em.shape
    x, arcs, na, nn_ = _dev(case.em), _dev(case.arcs), _dev(case.num_arcs), _dev(case.num_nodes)
    table = _dev(fp.table_of(case.start, case.trans))
    out = torch.zeros(B, device="cuda:0")
    ems = gtn.Batch.linear(B, T, C, x, calc_grad=False, borrow=True)
    c0 = gtn.debug_asg_lattice_score_stats()
    with pytest.raises(ValueError, match="frame count outside"):
        ems.asg_lattice_score(table, arcs, na, nn_, out, frames=[T + 1] + [1] * (B - 1))
    with pytest.raises(ValueError, match="table has"):
        ems.asg_lattice_score(table[:-1].contiguous(), arcs, na, nn_, out)
    host = np.zeros(C + C * C, np.float32)
    with pytest.raises(ValueError, match="table is not memory"):
        ems.asg_lattice_score(host.ctypes.data, arcs, na, nn_, out)
    with pytest.raises(ValueError, match="not a native linear batch"):
        gtn.Batch([gtn.linear_graph(T, C) for _ in range(B)]).asg_lattice_score(table.data_ptr(), arcs, na, nn_, out)
    gtn.synchronize()
    assert gtn.debug_asg_lattice_score_stats() == c0 and (out == 0).all()


def test_the_word_piece_training_step_lowers_the_loss(gtn):
    """decomposition_lattice -> pack_lattices -> asg_lattice_loss -> backward -> an SGD step on the transitions and the
    piece weights: the loss and the piece gradient against float64, and the step lowers the loss"""
    import torch
    import gtn_amd
    from asg_loss_fp import asg_terms_fp64
    from gtn_amd import torch_loss
    pieces = fp.the_pieces()
    words = ["the", "thee", "he", "tthe"]
    arcs, na, nn_, _ = gtn_amd.pack_lattices([gtn_amd.decomposition_lattice(wd, pieces) for wd in words])
    B, T, C = len(words), 12, 7
    rng = np.random.default_rng(6)
    em, trans, start = fp.model_of(rng, B, T, C)
    piece_score = rng.normal(0.0, 1.0, C).astype(np.float32)  # one learned score per piece
    theta = _dev(piece_score).requires_grad_(True)
    tr = _dev(trans).requires_grad_(True)
    x, st, a = _dev(em), _dev(start), _dev(arcs)

    def total():
        w = theta[a[:, :, 2].long()]  # [B, A]: the weight of an arc is the score of its piece
        return torch_loss.asg_lattice_loss(x, tr, a, _dev(na), _dev(nn_), w, start=st)
    loss = total()
    loss.sum().backward()
    want_theta = np.zeros(C)
    for b in range(B):
        n = na[b]
        s, d, l = (arcs[b, :n, i].astype(np.int64) for i in range(3))
        z, _, ga, _ = fp.lattice_fp64(em[b], trans, start, s, d, l, piece_score[l].astype(np.float64), int(nn_[b]))
        want = asg_terms_fp64(em[b], trans, start, [0])["fcc"] - z
        assert abs(loss[b].item() - want) <= fp.SCORE_GATE * max(1.0, abs(want))
        np.add.at(want_theta, l, -ga)
    print("piece gradient", theta.grad.cpu().numpy(), want_theta)
    uses = np.bincount(np.concatenate([arcs[b, :na[b], 2] for b in range(B)]), minlength=C)
    assert (np.abs(theta.grad.cpu().numpy() - want_theta) <= np.maximum(uses, 1) * fp.GRAD_GATE).all()
    assert tr.grad.abs().max().item() > 0
    before = loss.sum().item()
    with torch.no_grad():
        theta -= 0.1 * theta.grad
        tr -= 0.1 * tr.grad
    after = total().sum().item()
    print("loss before", before, "after", after)
    assert after < before
