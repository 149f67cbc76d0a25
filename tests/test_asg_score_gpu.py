"""Batched ASG scores of device-resident hypotheses and their weighted gradients (asg_score.hip through
gtnx_batch_asg_score / _grad; gtn_amd.torch_loss.asg_score, Batch.asg_score, gtn_asg_score_n).

The judge is the float64 yardstick tests/asg_loss_fp.py: fal_fp64 (through tests/asg_score_fp.py), which
tests/test_asg_score_cpu.py pins to an enumeration of alignments and to the oracle.  The gates are the project's float64
gates: scores within 1e-4 max(1, |score|), -inf exactly where the yardstick has it, emission gradients within 1e-4
absolute for weights in [-1, 1], table gradients within 1e-4 max(1, |want|) per entry.  The cases sit at the kernel's
edges (one wave, the widths, the lengths at which a lane gets another position, max_length and one above); the CPU file
shows that a float32 transcription of the kernels stays inside the gates on each of them.  Bit-equality is asked
wherever the contract promises it: run to run, sliced against unsliced, one pad content against another, one form
against another."""
import numpy as np
import pytest

import asg_score_fp as fp
from asg_loss_fp import fal_fp64

pytestmark = pytest.mark.gpu
NEG = -np.inf


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True, order="C")).to("cuda:0")


def _run(case, grad=True, tokens=None, lengths=None, want=("em", "trans", "start")):
    """torch_loss.asg_score on a case: (scores, d / d emissions, d / d table [C + C * C]) of sum(weights * scores) as
    numpy arrays; the gradients are None where not asked for"""
    import torch
    from gtn_amd import torch_loss
    x = _dev(case.em).requires_grad_(grad and "em" in want)
    tr = _dev(case.trans).requires_grad_(grad and "trans" in want)
    st = _dev(case.start).requires_grad_(grad and "start" in want)
    tok = _dev(case.tokens) if tokens is None else tokens
    ln = _dev(case.lengths) if lengths is None else lengths
    out = torch_loss.asg_score(x, tr, tok, ln, start=st, input_lengths=case.frames, max_length=case.max_length)
    g, gt = None, None
    if grad:
        out.backward(_dev(case.weights).reshape(out.shape))
        g = x.grad.cpu().numpy() if x.grad is not None else None
        if tr.grad is not None and st.grad is not None:
            gt = np.concatenate([st.grad.cpu().numpy().reshape(-1), tr.grad.cpu().numpy().reshape(-1)])
    torch.cuda.synchronize()
    assert (tok.cpu().numpy() == (case.tokens if tokens is None else tokens.cpu().numpy())).all()  # only read
    return out.detach().cpu().numpy(), g, gt


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and (a.view(np.uint32) == b.view(np.uint32)).all()


def _same(a, b):
    return all(_same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", fp.ALL_GPU_CASES)
def test_scores_and_gradients_against_float64(gtn, name):
    case, want = fp.case(name), fp.result(name, False)
    B, T, C = case.em.shape
    scores, grad, gtable = _run(case)
    scores = scores.reshape(want.scores.shape)
    print(name, "score error", fp.score_err(scores, want.scores), "gradient error", fp.grad_err(grad, want.grad),
          "table error", fp.table_err(gtable, want.gtable))
    assert not np.isnan(scores).any()
    assert (np.isneginf(scores) == np.isneginf(want.scores)).all(), (scores, want.scores)
    assert fp.score_ok(scores, want.scores)
    assert np.isfinite(grad).all() and np.isfinite(gtable).all()
    assert fp.grad_err(grad, want.grad) <= fp.GRAD_GATE
    assert fp.table_err(gtable, want.gtable) <= fp.TABLE_GATE
    if case.frames is not None:
        for b, f in enumerate(case.frames):
            assert (grad[b, f:] == 0).all(), "a pad row has a gradient"
    # a pair without a score, or with a weight of exactly 0, adds nothing: utterances made of such pairs stay 0, and
    # so do the table entries no live pair touches
    dead = np.isneginf(want.scores) | (np.asarray(case.weights).reshape(want.scores.shape) == 0)
    for b in range(B):
        if dead[b].all():
            assert (grad[b] == 0).all()
    assert (gtable[want.gtable == 0] == 0).all()


def test_pad_rows_are_never_read(gtn):
    a = _run(fp._frames_case(np.nan))
    b = _run(fp._frames_case(123.0))
    c = _run(fp._frames_case(np.inf))
    assert _same(a, b) and _same(a, c)


@pytest.mark.parametrize("name", ["c33", "edges"])
def test_elements_past_a_length_are_never_read(gtn, name):
    case = fp.case(name)
    tok = case.tokens.copy()
    L = tok.shape[-1]
    past = np.arange(L)[None, None, :] >= np.asarray(case.lengths)[:, :, None]
    assert past.any()
    tok[past] = 2 ** 30  # (poison: as an address it would lie gigabytes outside the table)
    assert _same(_run(case), _run(case._replace(tokens=tok)))


@pytest.mark.parametrize("name", ["edges", "c33", "wide-u1024"])
def test_two_calls_give_the_same_bits(gtn, name):
    assert _same(_run(fp.case(name)), _run(fp.case(name)))


def test_flat_form_and_int64_lengths(gtn):
    case = fp.case("wide-u65")  # N = 1
    B = case.em.shape[0]
    a = _run(case)
    tok, ln = _dev(case.tokens[:, 0]), _dev(case.lengths[:, 0].astype(np.int64))
    b = _run(case, tokens=tok, lengths=ln)
    assert b[0].shape == (B,) and _same_bits(a[0].reshape(B), b[0]) and _same(a[1:], b[1:])
    c33 = fp.case("c33")
    assert c33.lengths.dtype == np.int64
    assert _same(_run(c33), _run(c33, lengths=_dev(c33.lengths.astype(np.int32))))


def test_raw_addresses_and_a_row_stride_above_the_width(gtn):
    import torch
    case = fp.case("c4")
    B, T, C = case.em.shape
    N, L = case.tokens.shape[1:]
    want = _run(case)
    wide = np.full((B, N, L + 5), 3, dtype=np.int32)  # (valid labels behind the rows: they would count if read)
    wide[:, :, :L] = case.tokens
    x, tok, ln = _dev(case.em), _dev(wide), _dev(case.lengths.astype(np.int32))
    w, table = _dev(case.weights), _dev(fp.table_of(case.start, case.trans))
    scores = torch.full((B * N + 2,), 5.0, device="cuda:0")
    grad = torch.full((B * T * C + 2,), 5.0, device="cuda:0")
    gtab = torch.full((C + C * C + 2,), 5.0, device="cuda:0")
    ems = gtn.Batch.linear(B, T, C, x, calc_grad=False, borrow=True)
    c0 = gtn.debug_asg_score_stats()
    ems.asg_score(table.data_ptr(), tok.data_ptr(), ln.data_ptr(), scores[1:].data_ptr(), None, None, N=N, L=L,
                  row_stride=L + 5)
    ems.asg_score_grad(table.data_ptr(), tok.data_ptr(), ln.data_ptr(), w.data_ptr(), grad[1:].data_ptr(),
                       gtab[1:].data_ptr(), None, None, N=N, L=L, row_stride=L + 5)
    gtn.synchronize()
    c1 = gtn.debug_asg_score_stats()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (2, 2 * B * N)
    s, g, t = scores.cpu().numpy(), grad.cpu().numpy(), gtab.cpu().numpy()
    assert s[0] == 5.0 and s[-1] == 5.0 and g[0] == 5.0 and g[-1] == 5.0 and t[0] == 5.0 and t[-1] == 5.0, "guards"
    assert _same_bits(s[1:-1].reshape(B, N), want[0]) and _same_bits(g[1:-1].reshape(B, T, C), want[1])
    assert _same_bits(t[1:-1], want[2])
    # either gradient alone has the bits it has beside the other
    g2 = torch.empty(B, T, C, device="cuda:0")
    t2 = torch.empty(C + C * C, device="cuda:0")
    ems.asg_score_grad(table, tok[:, :, :L], ln, w, grad_out=g2)
    ems.asg_score_grad(table, tok[:, :, :L], ln, w, grad_table_out=t2)
    # the same through tensors: a view whose rows are further apart than they are wide
    s2 = torch.empty(B, N, device="cuda:0")
    ems.asg_score(table, tok[:, :, :L], ln, s2)
    gtn.synchronize()
    assert _same_bits(s2.cpu().numpy(), want[0]) and _same_bits(g2.cpu().numpy(), want[1])
    assert _same_bits(t2.cpu().numpy(), want[2])


@pytest.mark.parametrize("name,pairs", [("c4", 2), ("c4", 0), ("c33", 3), ("edges", 5)])
def test_slices_give_the_bits_of_the_unsliced_run(gtn, monkeypatch, name, pairs):
    """a lowered scratch cap: the pairs run in slices that cut utterances apart (two pairs of four; one pair, the cap
    below a single pair's rows; three of four; five of four)"""
    case = fp.case(name)
    per_pair = 4 * case.em.shape[1] * fp.default_max_length(case)  # bytes of a pair's alpha rows
    monkeypatch.delenv("GTNX_ASG_SCORE_SCRATCH_BYTES", raising=False)
    want = _run(case)
    monkeypatch.setenv("GTNX_ASG_SCORE_SCRATCH_BYTES", str(per_pair * pairs + 64 if pairs else 100))
    got = _run(case)
    assert _same(got, want)


def test_without_requires_grad_nothing_but_the_forward_launches(gtn):
    import torch
    case = fp.case("edges")
    c0 = gtn.debug_asg_score_stats()
    _run(case, grad=False)
    c1 = gtn.debug_asg_score_stats()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, 12)
    full = _run(case, grad=True)
    c2 = gtn.debug_asg_score_stats()
    assert (c2[0] - c1[0], c2[1] - c1[1]) == (2, 24)
    # only what requires_grad asks for: the emissions alone, the transitions alone -- one gradient call each
    only_em = _run(case, want=("em",))
    assert only_em[2] is None and _same_bits(only_em[1], full[1])
    from gtn_amd import torch_loss
    x, tr = _dev(case.em), _dev(case.trans).requires_grad_(True)
    out = torch_loss.asg_score(x, tr, _dev(case.tokens), _dev(case.lengths), start=_dev(case.start))
    out.backward(_dev(case.weights))
    C = case.em.shape[2]
    assert _same_bits(tr.grad.cpu().numpy().reshape(-1), full[2][C:])
    c3 = gtn.debug_asg_score_stats()
    assert (c3[0] - c2[0], c3[1] - c2[1]) == (4, 48)
    # no pairs at all: nothing launches, the gradients are zeros
    x = _dev(case.em).requires_grad_(True)
    tr = _dev(case.trans).requires_grad_(True)
    out = torch_loss.asg_score(x, tr, torch.zeros(3, 0, 8, dtype=torch.int32, device="cuda:0"),
                               torch.zeros(3, 0, dtype=torch.int32, device="cuda:0"))
    assert out.shape == (3, 0)
    out.sum().backward()
    assert (x.grad == 0).all() and (tr.grad == 0).all() and gtn.debug_asg_score_stats() == c3


def test_what_needs_the_device_is_refused_there(gtn):
    """not a native linear batch, a frame count outside 0 .. M, a table in host memory, an output on another device:
    invalid arguments, nothing is launched"""
    import torch
    case = fp.case("edges")
    B, T, C = case.em.shape
    x, tok, ln = _dev(case.em), _dev(case.tokens), _dev(case.lengths)
    table = _dev(fp.table_of(case.start, case.trans))
    out = torch.zeros(B, 4, device="cuda:0")
    ems = gtn.Batch.linear(B, T, C, x, calc_grad=False, borrow=True)
    c0 = gtn.debug_asg_score_stats()
    with pytest.raises(ValueError, match="frame count outside"):
        ems.asg_score(table, tok, ln, out, frames=[T + 1, 1, 1])
    with pytest.raises(ValueError, match="frame count outside"):
        ems.asg_score(table, tok, ln, out, frames=[-1, 1, 1])
    with pytest.raises(ValueError, match="not a native linear batch"):
        gtn.Batch([gtn.linear_graph(T, C) for _ in range(B)]).asg_score(table.data_ptr(), tok, ln, out)
    host = torch.from_numpy(fp.table_of(case.start, case.trans))
    with pytest.raises(ValueError, match="table is not memory of the engine's current device"):
        ems.asg_score(host.data_ptr(), tok, ln, out)
    pinned = host.pin_memory()
    with pytest.raises(ValueError, match="table is not memory of the engine's current device"):
        ems.asg_score(pinned.data_ptr(), tok, ln, out)
    with pytest.raises(ValueError, match="table has 29 entries"):
        ems.asg_score(table[:-1], tok, ln, out)
    if torch.cuda.device_count() > 1:
        other = torch.zeros(B, 4, device="cuda:1")
        with pytest.raises(ValueError, match="output pointer is not memory"):
            ems.asg_score(table, tok, ln, other.data_ptr(), N=4, L=8, row_stride=8)
        other_g = torch.zeros(C + C * C, device="cuda:1")
        with pytest.raises(ValueError, match="output pointer is not memory"):
            ems.asg_score_grad(table, tok, ln, _dev(case.weights), None, other_g.data_ptr(), N=4, L=8, row_stride=8)
        assert (other == 0).all() and (other_g == 0).all()
    gtn.synchronize()
    assert gtn.debug_asg_score_stats() == c0 and (out == 0).all()


def _loss_case():
    """two hypotheses per utterance, the targets of two asg_loss calls: B = 3, T = 30, C = 7"""
    rng = np.random.default_rng(8)
    B, T, C = 3, 30, 7
    em, trans, start = fp.model_of(rng, B, T, C)
    y1 = [rng.integers(0, C, n) for n in (5, 20, 1)]
    y2 = [rng.integers(0, C, n) for n in (7, 18, 2)]
    return em, trans, start, y1, y2


def test_non_uniform_seeds_reach_transitions_and_start(gtn):
    """the case asg_loss(reduction="none") refuses: a different upstream gradient per hypothesis"""
    import torch
    from gtn_amd import torch_loss
    em, trans, start, y1, _ = _loss_case()
    B, T, C = em.shape
    tokens, lengths = fp.pack(y1, B, 1, 24)
    g = np.array([0.75, -1.0, 0.25], dtype=np.float32)
    x = _dev(em).requires_grad_(True)
    tr = _dev(trans).requires_grad_(True)
    st = _dev(start).requires_grad_(True)
    with pytest.raises(RuntimeError, match="uniform upstream"):  # (what this entry point is for)
        torch_loss.asg_loss(x, tr, [y.tolist() for y in y1], start=st, reduction="none").backward(_dev(g))
    x.grad = tr.grad = st.grad = None
    torch_loss.asg_score(x, tr, _dev(tokens[:, 0]), _dev(lengths[:, 0]), start=st).backward(_dev(g))
    want_em, want_tab = np.zeros((B, T, C)), np.zeros(C + C * C)
    for b in range(B):
        _, g_em, g_tr = fal_fp64(em[b], trans, start, y1[b])
        want_em[b] = float(g[b]) * g_em
        want_tab += float(g[b]) * g_tr
    got_tab = np.concatenate([st.grad.cpu().numpy(), tr.grad.cpu().numpy().reshape(-1)])
    print("gradient error", fp.grad_err(x.grad.cpu().numpy(), want_em), "table error", fp.table_err(got_tab, want_tab))
    assert tuple(tr.grad.shape) == (C, C) and tuple(st.grad.shape) == (C,)
    assert fp.grad_err(x.grad.cpu().numpy(), want_em) <= fp.GRAD_GATE
    assert fp.table_err(got_tab, want_tab) <= fp.TABLE_GATE
    assert np.abs(want_tab[:C]).max() > 0.2 and np.abs(want_tab[C:]).max() > 0.2


def test_a_difference_of_asg_losses_is_a_difference_of_scores(gtn):
    """asg_loss(x, tr, [y1]) - asg_loss(x, tr, [y2]) == asg_score(y2) - asg_score(y1): the full-connect term cancels;
    so do its gradients"""
    import torch
    from gtn_amd import torch_loss
    em, trans, start, y1, y2 = _loss_case()
    B, T, C = em.shape
    tokens, lengths = fp.pack([y for pair in zip(y1, y2) for y in pair], B, 2, 24)

    def leaves():
        return (_dev(em).requires_grad_(True), _dev(trans).requires_grad_(True), _dev(start).requires_grad_(True))
    x, tr, st = leaves()
    diff = (torch_loss.asg_loss(x, tr, [y.tolist() for y in y1], start=st)
            - torch_loss.asg_loss(x, tr, [y.tolist() for y in y2], start=st))
    diff.sum().backward()
    x2, tr2, st2 = leaves()
    score = torch_loss.asg_score(x2, tr2, _dev(tokens), _dev(lengths), start=st2)
    (score[:, 1] - score[:, 0]).sum().backward()
    d, s = diff.detach().cpu().numpy().astype(np.float64), score.detach().cpu().numpy().astype(np.float64)
    print("loss difference", d, "score difference", s[:, 1] - s[:, 0])
    assert (np.abs(d - (s[:, 1] - s[:, 0])) <= fp.SCORE_GATE * np.maximum(1.0, np.abs(s).max(axis=1))).all()
    assert fp.grad_err(x2.grad.cpu().numpy(), x.grad.cpu().numpy().astype(np.float64)) <= fp.GRAD_GATE
    got = np.concatenate([st2.grad.cpu().numpy(), tr2.grad.cpu().numpy().reshape(-1)])
    want = np.concatenate([st.grad.cpu().numpy(), tr.grad.cpu().numpy().reshape(-1)]).astype(np.float64)
    print("table error", fp.table_err(got, want))
    assert fp.table_err(got, want) <= fp.TABLE_GATE


def test_the_asg_chain(gtn):
    """asg_decode(collapse=True) -> asg_score with L = T, nothing downloaded on the way: the decoded path is one
    alignment of its collapsed sequence"""
    import torch
    from gtn_amd import torch_loss
    rng = np.random.default_rng(12)
    B, T, C = 4, 40, 9
    em, trans, start = fp.model_of(rng, B, T, C, sigma=1.0)
    trans += 1.5 * np.eye(C, dtype=np.float32)  # (runs: the collapsed sequences are shorter than T)
    frames = [40, 17, 1, 33]
    x, tr, st = _dev(em), _dev(trans), _dev(start)
    labels, path, collapsed, lengths = torch_loss.asg_decode(x, tr, start=st, input_lengths=frames, collapse=True)
    c0 = gtn.debug_asg_score_stats()
    score = torch_loss.asg_score(x, tr, collapsed, lengths, start=st, input_lengths=frames)
    c1 = gtn.debug_asg_score_stats()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, B) and tuple(score.shape) == (B,) and collapsed.shape[1] == T
    s, p = score.cpu().numpy().astype(np.float64), path.cpu().numpy().astype(np.float64)
    tk, ln = collapsed.cpu().numpy(), lengths.cpu().numpy()
    assert np.isfinite(s).all() and (ln >= 1).all() and (ln < np.array(frames)).any()
    want = np.array([fal_fp64(em[b, :frames[b]], trans, start, tk[b, :ln[b]])[0] for b in range(B)])
    print("score", s, "float64", want, "path", p)
    gate = fp.SCORE_GATE * np.maximum(1.0, np.abs(want))
    assert (np.abs(s - want) <= gate).all()
    assert (s >= p - gate).all()
