"""Batched ASG Viterbi alignment of device-resident token lattices (asg_lattice_align.hip through
gtnx_batch_asg_lattice_align; torch_loss.asg_lattice_align, Batch.asg_lattice_align, gtn_asg_lattice_align_n).  The judge
is the float32 transcription of tests/asg_lattice_align_fp.py: the contract makes every output
reproducible bit for bit, so every comparison is of bits, fills included; the rows handed over are wider than P and M
and lie between guard words, and nothing outside the widths may change."""
import numpy as np
import pytest

import asg_lattice_align_fp as fp
import asg_lattice_fp as afp
from ctc_lattice_fp import chain_lattice, pack, sort_by_dst

pytestmark = pytest.mark.gpu
GUARD_I, GUARD_F = 77, 5.0


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True, order="C")).to("cuda:0")


def _run(gtn, case, P=None, optional=True, arcs=None, em=None, row_pad=0, out_pad=3, frame_pad=5):
    """Batch.asg_lattice_align on raw addresses, rows wider than P / M between guard words.  Checks the guards, the
    columns beyond the widths and that the inputs are only read; returns the Result (None: an output not asked for)."""
    import torch
    B, M, C = case.em.shape
    A = case.arcs.shape[1]
    P = fp.default_max_path(case) if P is None else P
    wide = np.zeros((B, 3 * A + row_pad), dtype=np.int32)  # (valid arcs of label 0 behind the rows: they would count if read)
    wide[:, 1::3] = 1
    wide[:, :3 * A] = (case.arcs if arcs is None else arcs).reshape(B, 3 * A)
    x, a, table = _dev(case.em if em is None else em), _dev(wide), _dev(afp.table_of(case.start, case.trans))
    w = None if case.weights is None else _dev(case.weights)
    na, nn_ = _dev(case.num_arcs), _dev(case.num_nodes)
    ins = [t for t in (x, a, table, w, na, nn_) if t is not None]
    keep = [t.clone() for t in ins]
    OS, FS = P + out_pad, M + frame_pad

    buf = lambda n, dtype, fill: torch.full((n + 2,), fill, dtype=dtype, device="cuda:0")  # noqa: E731
    scores, plen = buf(B, torch.float32, GUARD_F), buf(B, torch.int32, GUARD_I)
    rows = [buf(B * OS, torch.int32, GUARD_I) for _ in range(4)]
    tsc = buf(B * OS, torch.float32, GUARD_F) if optional else None
    fa = buf(B * FS, torch.int32, GUARD_I) if optional else None

    ptr = lambda t: None if t is None else t[1:].data_ptr()  # noqa: E731
    torch.cuda.synchronize()  # (the call runs on the engine's stream: the uploads and the guard fills come first)
    gtn.Batch.linear(B, M, C, x, calc_grad=False, borrow=True).asg_lattice_align(
        table.data_ptr(), a.data_ptr(), na.data_ptr(), nn_.data_ptr(), ptr(scores), ptr(plen), *(ptr(r) for r in rows),
        ptr(tsc), ptr(fa), None if w is None else w.data_ptr(), case.frames, case.max_states, case.max_edges, A=A,
        row_stride=3 * A + row_pad, P=P, out_stride=OS, frame_stride=FS)
    gtn.synchronize()
    for t, k in zip(ins, keep):  # only read
        assert (t.view(torch.int32) == k.view(torch.int32)).all()

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


def _check(name, got, want):
    for field, g, w in zip(fp.Result._fields, got, want):
        if g is not None:
            assert g.shape == w.shape and g.dtype == w.dtype, (name, field)
            bad = np.argwhere(np.ascontiguousarray(g).view(np.uint32) != np.ascontiguousarray(w).view(np.uint32))
            assert not len(bad), (name, field, bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


@pytest.mark.parametrize("name", afp.ALL_GPU_CASES + ("ties",))
def test_every_output_has_the_bits_of_the_transcription(gtn, name):
    case = fp.tie_batch() if name == "ties" else afp.case(name)
    got = _run(gtn, case)
    _check(name, got, fp.evaluate(case) if name == "ties" else fp.result(name))
    assert np.isfinite(got.scores).any() and not np.isnan(got.scores).any()


def test_frame_counts_around_the_store_blocks_and_a_truncating_width(gtn):
    """the diamond of the tie lattices (its arc 0 -> 3 fits one frame; weights that favour its three-arc path) under
    1 .. 129 frames, four waves wide: the 64-frame store blocks of frame_arcs end at each of the counts"""
    FRAME_COUNTS = (1, 2, 63, 64, 65, 129)
    B, C = len(FRAME_COUNTS), fp.TIE_C
    arcs, w = sort_by_dst(fp.TIE_LATTICES[8][1], [0, -4, 0, -8, -4, 0])
    a, na, nn_, ws = pack([(arcs, 4, w)] * B)
    em, trans, start = afp.model_of(np.random.default_rng(129), B, max(FRAME_COUNTS), C)
    for b, f in enumerate(FRAME_COUNTS):
        em[b, f:] = np.nan
    case = afp.Case(em, trans, start, a, na, nn_, ws, FRAME_COUNTS, 256, None, None)
    got = _run(gtn, case)
    _check("frames", got, fp.evaluate(case))
    assert np.isfinite(got.scores).all() and got.path_len[0] == 1 and got.path_len.max() == 3
    cut = _run(gtn, case, P=2)
    _check("frames, P = 2", cut, fp.evaluate(case, P=2))
    assert (cut.path_len == got.path_len).all()


def test_the_bits_do_not_depend_on_what_the_contract_says_they_do_not(gtn, monkeypatch):
    case, want = afp.case("ragged"), fp.result("ragged")
    A = case.arcs.shape[1]
    _check("run to run", _run(gtn, case), want)
    _check("run to run", _run(gtn, case), want)
    monkeypatch.setenv("GTNX_ASG_LATTICE_ALIGN_SCRATCH_BYTES", "1")  # (every utterance alone)
    _check("sliced", _run(gtn, case), want)
    monkeypatch.delenv("GTNX_ASG_LATTICE_ALIGN_SCRATCH_BYTES")
    _check("pads", _run(gtn, case, em=afp._ragged_case(pad=1e30).em), want)
    junk = case.arcs.copy()
    past = np.arange(A)[None, :] >= np.maximum(case.num_arcs, 0)[:, None]
    junk[past] = np.random.default_rng(5).integers(-2 ** 31, 2 ** 31 - 1, (int(past.sum()), 3))
    _check("garbage past num_arcs", _run(gtn, case, arcs=junk), want)
    _check("row stride", _run(gtn, case, row_pad=7), want)
    _check("no optional outputs", _run(gtn, case, optional=False), want)


def _args(case):
    """the leading arguments of torch_loss.asg_lattice_align and asg_lattice_score alike"""
    return (_dev(case.em), _dev(case.trans), _dev(case.arcs), _dev(case.num_arcs), _dev(case.num_nodes),
            None if case.weights is None else _dev(case.weights), _dev(case.start), case.frames, case.max_states,
            case.max_edges)


@pytest.mark.parametrize("name", ["indeg8-c37", "ragged", "edges"])
def test_the_device_calls_agree_with_each_other(gtn, name, monkeypatch):
    from gtn_amd import torch_loss
    case, want = afp.case(name), fp.result(name)
    B = len(case.num_arcs)
    before = gtn.debug_asg_lattice_align_stats()
    native = [t.cpu().numpy() for t in torch_loss.asg_lattice_align(*_args(case), return_token_scores=True, return_frames=True)]
    monkeypatch.setenv("GTN_AMD_PYTHON_CRITERIA", "1")
    monkeypatch.setattr(torch_loss, "_NATIVE", None)
    python = [t.cpu().numpy() for t in torch_loss.asg_lattice_align(*_args(case), return_token_scores=True, return_frames=True)]
    monkeypatch.undo()
    _check("native route", fp.Result(*native), want)
    _check("python route", fp.Result(*python), want)
    assert gtn.debug_asg_lattice_align_stats() == (before[0] + 2, before[1] + 2 * B)
    # the path's own alignment: asg_token_align of the returned tokens gives the score less the path's weights
    scores, plen, parcs, ptoks = (_dev(v) for v in native[:4])
    pair = torch_loss.asg_token_align(_dev(case.em), _dev(case.trans), ptoks, plen, _dev(case.start), case.frames,
                                      max_length=ptoks.shape[1])[0].cpu().numpy()
    wsum = np.array([0.0 if case.weights is None else case.weights[b, native[2][b, :native[1][b]]].sum(dtype=np.float64)
                     for b in range(B)])
    has = native[1] > 0
    assert has.any() and afp.score_ok(pair[has], (native[0] - wsum)[has])
    total = torch_loss.asg_lattice_score(*_args(case)).cpu().numpy()
    # (max <= log-sum is exact arithmetic's; the two float32 chains round apart, so it is asked within the score gate)
    assert ((total == -np.inf) == ~has).all() and (native[0][has] <= total[has] + afp.SCORE_GATE * np.abs(total[has])).all()


def test_a_chain_lattice_has_the_spans_of_asg_token_align(gtn):
    from gtn_amd import torch_loss
    em, trans, start, y = fp.chain_model()
    a, na, nn_, _ = pack([chain_lattice(y)])
    got = torch_loss.asg_lattice_align(*_args(afp.Case(em, trans, start, a, na, nn_, None, None, 64, None, None)),
                                       return_frames=True)
    want = torch_loss.asg_token_align(_dev(em), _dev(trans), _dev(y[None]), _dev(np.array([11], np.int32)), _dev(start),
                                      return_frames=True)
    assert afp.score_ok(got[0].cpu().numpy(), want[0].cpu().numpy())
    for g, w in zip((got[4], got[5], got[6]), want[1:]):
        assert (g == w).all()
