"""Batched edit distance with device-resident output (edit_distance.hip through gtnx_batch_edit_distance;
gtn_amd.edit_distance, gtn_amd.torch_loss.edit_distance, gtn_edit_distance_n).

The judge is the textbook table and the contract's walk back of tests/edit_distance_fp.py, which
tests/test_edit_distance_cpu.py pins to the unmodified reference.  Distances and counts are integers: every comparison
is ==.

`dist` and `ops` are dense arrays (the call has no stride for them): their guards are an element before and after, and
they must survive.  The input rows carry guard columns behind L and U (strides larger than the widths), and from each
length on they hold tokens of the row's own alphabet, which would change the answer if they were read."""
import numpy as np
import pytest

import edit_distance_fp as fp

pytestmark = pytest.mark.gpu
SENTINEL = -7


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True, order="C")).to("cuda:0")


def _run(gtn, case, with_ops, address=False, arrays=None):
    """gtn.edit_distance on the case's guarded arrays.  Returns (dist [B, N], ops [B, N, 3] or None, (calls, pairs)
    counted by this call)"""
    import torch
    hyp, hl, ref, rl = arrays if arrays is not None else case.arrays()
    B, N, L, U = case.B, case.N, case.L, case.U
    hyp_d, hl_d, ref_d, rl_d = _dev(hyp), _dev(hl), _dev(ref), _dev(rl)
    dist = torch.full((B * N + 2,), SENTINEL, dtype=torch.int32, device="cuda:0")
    ops = torch.full((3 * B * N + 2,), SENTINEL, dtype=torch.int32, device="cuda:0")
    dv, ov = dist[1:B * N + 1].view(B, N), ops[1:3 * B * N + 1].view(B, N, 3)
    torch.cuda.synchronize()
    c0 = gtn.debug_edit_distance_stats()
    try:
        if address:
            gtn.edit_distance(hyp_d.data_ptr(), hl_d.data_ptr(), ref_d.data_ptr(), rl_d.data_ptr(), dv.data_ptr(),
                              ov.data_ptr() if with_ops else None, B=B, N=N, L=L, U=U, hyp_stride=hyp.shape[2],
                              ref_stride=ref.shape[1])
        else:
            gtn.edit_distance(hyp_d[:, :, :L], hl_d, ref_d[:, :U], rl_d, dv, ov if with_ops else None)
    finally:
        gtn.synchronize()
        c1 = gtn.debug_edit_distance_stats()
        d, o = dist.cpu().numpy(), ops.cpu().numpy()
        _run.raw = (d, o)
        assert d[0] == SENTINEL and d[-1] == SENTINEL, "dist: guards"
        assert o[0] == SENTINEL and o[-1] == SENTINEL, "ops: guards"
        if not with_ops:
            assert (o == SENTINEL).all(), "ops written without being asked for"
        # the inputs are only read
        assert (hyp_d.cpu().numpy() == hyp).all() and (ref_d.cpu().numpy() == ref).all()
        assert (hl_d.cpu().numpy() == hl).all() and (rl_d.cpu().numpy() == rl).all()
    return d[1:-1].reshape(B, N), (o[1:-1].reshape(B, N, 3) if with_ops else None), (c1[0] - c0[0], c1[1] - c0[1])


def _cap(monkeypatch, case):
    if case.cap is not None:
        monkeypatch.setenv("GTNX_EDIT_DISTANCE_SCRATCH_BYTES", str(case.cap))
    else:
        monkeypatch.delenv("GTNX_EDIT_DISTANCE_SCRATCH_BYTES", raising=False)


@pytest.mark.parametrize("case", fp.gpu_cases(), ids=repr)
def test_distances_and_counts_equal_the_table(gtn, case, monkeypatch):
    """every pair against its own table; with and without ops the same dist bit for bit; counters advance by
    (1, B * N) per launched call"""
    _cap(monkeypatch, case)
    want_dist, want_ops = fp.expected(case)
    plain, none, counted = _run(gtn, case, False)
    assert none is None and counted == (1, case.B * case.N)
    bad = np.argwhere(plain != want_dist)
    assert bad.size == 0, (case, bad[:5].tolist(), plain[tuple(bad[0])], want_dist[tuple(bad[0])])
    dist, ops, counted = _run(gtn, case, True)
    assert counted == (1, case.B * case.N)
    assert (dist == plain).all()
    bad = np.argwhere((ops != want_ops).any(axis=2))
    assert bad.size == 0, (case, bad[:5].tolist(), ops[tuple(bad[0])], want_ops[tuple(bad[0])])
    assert (ops.sum(axis=2) == dist).all()


def _case(name):
    return next(c for c in fp.gpu_cases() if c.name == name)


def test_sliced_call_equals_the_unsliced_one(gtn, monkeypatch):
    case = _case("sliced")
    monkeypatch.delenv("GTNX_EDIT_DISTANCE_SCRATCH_BYTES", raising=False)
    whole = _run(gtn, case, True)
    monkeypatch.setenv("GTNX_EDIT_DISTANCE_SCRATCH_BYTES", str(case.cap))
    sliced = _run(gtn, case, True)
    monkeypatch.setenv("GTNX_EDIT_DISTANCE_SCRATCH_BYTES", "1")  # below one pair: a pair per launch
    single = _run(gtn, case, True)
    for got in (whole, sliced, single):
        assert (got[0] == fp.expected(case)[0]).all() and (got[1] == fp.expected(case)[1]).all()
        assert got[2] == (1, case.B * case.N)


@pytest.mark.parametrize("name", ["B5-N3", "edges-a5", "clamped-lengths"])
def test_raw_addresses_equal_tensors(gtn, name, monkeypatch):
    monkeypatch.delenv("GTNX_EDIT_DISTANCE_SCRATCH_BYTES", raising=False)
    case = _case(name)
    a = _run(gtn, case, True, address=True)
    t = _run(gtn, case, True)
    assert (a[0] == t[0]).all() and (a[1] == t[1]).all() and a[2] == t[2] == (1, case.B * case.N)
    assert (a[0] == fp.expected(case)[0]).all() and (a[1] == fp.expected(case)[1]).all()
    assert (_run(gtn, case, False, address=True)[0] == a[0]).all()


def test_lengths_outside_the_widths_are_clamped(gtn, monkeypatch):
    """-3 counts as 0 and L + 5 as L (U + 5 as U): the same answers as the clamped lengths given outright"""
    monkeypatch.delenv("GTNX_EDIT_DISTANCE_SCRATCH_BYTES", raising=False)
    case = _case("clamped-lengths")
    hyp, hl, ref, rl = case.arrays()
    assert hl.min() == -3 and hl.max() == case.L + 5 and rl.min() == -3 and rl.max() == case.U + 5
    lied = _run(gtn, case, True)
    told = _run(gtn, case, True, arrays=(hyp, np.clip(hl, 0, case.L), ref, np.clip(rl, 0, case.U)))
    assert (lied[0] == told[0]).all() and (lied[1] == told[1]).all()
    assert (lied[0] == fp.expected(case)[0]).all()
    # an empty side scores the other side's length
    assert lied[0][0, 0] == case.U and tuple(lied[1][0, 0]) == (0, case.U, 0)
    assert lied[0][1, 0] == len(case.hyps[1][0]) and tuple(lied[1][1, 0]) == (0, 0, len(case.hyps[1][0]))


def test_two_dimensional_hyp_is_one_hypothesis_per_utterance(gtn, monkeypatch):
    import torch
    from gtn_amd import torch_loss
    monkeypatch.delenv("GTNX_EDIT_DISTANCE_SCRATCH_BYTES", raising=False)
    case = _case("B70-N1")
    hyp, hl, ref, rl = case.arrays()
    B, L, U = case.B, case.L, case.U
    want_dist, want_ops = fp.expected(case)
    hyp_d, hl_d, ref_d, rl_d = _dev(hyp), _dev(hl), _dev(ref), _dev(rl)
    d2, d3 = (torch.full((B, 1), SENTINEL, dtype=torch.int32, device="cuda:0") for _ in range(2))
    gtn.edit_distance(hyp_d[:, 0, :L], hl_d, ref_d[:, :U], rl_d, d2)
    gtn.edit_distance(hyp_d[:, :, :L], hl_d, ref_d[:, :U], rl_d, d3)
    gtn.synchronize()
    assert (d2.cpu().numpy() == want_dist).all() and (d3.cpu().numpy() == want_dist).all()
    # torch_loss: [B, L] with [B] lengths against [B, 1, L] with [B, 1]; int64 lengths are converted on the device
    flat, flat_ops = torch_loss.edit_distance(hyp_d[:, 0, :L], hl_d[:, 0], ref_d[:, :U], rl_d, return_ops=True)
    cube, cube_ops = torch_loss.edit_distance(hyp_d[:, :, :L], hl_d.long(), ref_d[:, :U], rl_d.long(), return_ops=True)
    only = torch_loss.edit_distance(hyp_d[:, 0, :L], hl_d[:, 0].long(), ref_d[:, :U], rl_d)
    assert flat.is_cuda and flat.dtype == torch.int32 and tuple(flat.shape) == (B,) and tuple(flat_ops.shape) == (B, 3)
    assert tuple(cube.shape) == (B, 1) and tuple(cube_ops.shape) == (B, 1, 3) and tuple(only.shape) == (B,)
    assert (flat.cpu().numpy() == want_dist[:, 0]).all() and (cube.cpu().numpy() == want_dist).all()
    assert (only.cpu().numpy() == want_dist[:, 0]).all()
    assert (flat_ops.cpu().numpy() == want_ops[:, 0]).all() and (cube_ops.cpu().numpy() == want_ops).all()


def test_torch_entry_on_an_nbest_shape(gtn, monkeypatch):
    from gtn_amd import torch_loss
    monkeypatch.delenv("GTNX_EDIT_DISTANCE_SCRATCH_BYTES", raising=False)
    case = _case("B70-N3")
    hyp, hl, ref, rl = case.arrays(pad_l=0, pad_u=0)
    c0 = gtn.debug_edit_distance_stats()
    dist, ops = torch_loss.edit_distance(_dev(hyp), _dev(hl), _dev(ref), _dev(rl), return_ops=True)
    best = dist.min(dim=1).values  # the oracle error count, still on the device
    c1 = gtn.debug_edit_distance_stats()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, case.B * case.N)
    assert (dist.cpu().numpy() == fp.expected(case)[0]).all() and (ops.cpu().numpy() == fp.expected(case)[1]).all()
    assert (best.cpu().numpy() == fp.expected(case)[0].min(axis=1)).all()


def test_refused_and_empty_calls_do_not_count(gtn):
    import torch
    hyp = torch.zeros(2, 3, 8, dtype=torch.int32, device="cuda:0")
    hl = torch.zeros(2, 3, dtype=torch.int32, device="cuda:0")
    ref = torch.zeros(2, 5, dtype=torch.int32, device="cuda:0")
    rl = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    dist = torch.full((2, 3), SENTINEL, dtype=torch.int32, device="cuda:0")
    before = gtn.debug_edit_distance_stats()
    kw = dict(B=2, N=3, L=8, U=5, hyp_stride=8, ref_stride=5)
    # (the refusal of an output on ANOTHER GPU of the process needs two devices: ptr_local_to admits every pointer where
    # there is one, host memory included, so it is not exercised here)
    with pytest.raises(ValueError, match="hyp_stride is shorter"):
        gtn.edit_distance(hyp.data_ptr(), hl.data_ptr(), ref.data_ptr(), rl.data_ptr(), dist.data_ptr(), None,
                          **{**kw, "hyp_stride": 7})
    with pytest.raises(ValueError, match="null dist pointer"):
        gtn.edit_distance(hyp, hl, ref, rl, None)
    gtn.edit_distance(hyp[:0], hl[:0], ref[:0], rl[:0], dist[:0])
    gtn.edit_distance(hyp[:, :0], hl[:, :0], ref, rl, dist[:, :0])
    gtn.edit_distance(hyp.data_ptr(), hl.data_ptr(), ref.data_ptr(), rl.data_ptr(), dist.data_ptr(), None,
                      **{**kw, "B": 0})
    gtn.synchronize()
    assert gtn.debug_edit_distance_stats() == before
    assert (dist.cpu().numpy() == SENTINEL).all()
    # widths of zero are a call like any other: every distance is the other side's length
    rl2 = _dev(np.array([4, 0], np.int32))
    gtn.edit_distance(hyp.data_ptr(), hl, ref, rl2, dist, B=2, N=3, L=0, hyp_stride=8)
    gtn.synchronize()
    assert dist.cpu().numpy().tolist() == [[4, 4, 4], [0, 0, 0]]
    after = gtn.debug_edit_distance_stats()
    assert (after[0] - before[0], after[1] - before[1]) == (1, 6)


def test_widths_of_4096(gtn, monkeypatch):
    """the largest reference the kernel takes (64 blocks: every lane of the wave owns one) against 4096 tokens"""
    monkeypatch.delenv("GTNX_EDIT_DISTANCE_SCRATCH_BYTES", raising=False)
    rng = np.random.RandomState(4096)
    ref = rng.randint(0, 4, size=4096).tolist()
    case = fp.Case("4096", [ref], [[fp.edited(ref, rng, 4096, 4)]])
    assert (case.L, case.U) == (4096, 4096)
    want_dist, (s, d, i), _ = fp.distance_ops(case.refs[0], case.hyps[0][0])
    plain = _run(gtn, case, False)
    dist, ops, _ = _run(gtn, case, True)
    assert plain[0][0, 0] == want_dist and dist[0, 0] == want_dist
    assert tuple(ops[0, 0]) == (s, d, i)


@pytest.mark.parametrize("nbest", [1, 3])
def test_end_to_end_from_the_decoders(gtn, nbest):
    """torch_loss.ctc_beam_decode and torch_loss.ctc_decode hand their tensors straight to torch_loss.edit_distance --
    no host access in between; then everything is downloaded and judged by the table on the downloaded hypotheses"""
    import torch
    from gtn_amd import torch_loss
    rng = np.random.RandomState(5 + nbest)
    B, T, C, U = 6, 40, 7, 12
    log_probs = torch.from_numpy(rng.randn(B, T, C).astype(np.float32)).to("cuda:0").log_softmax(-1)
    frames = torch.tensor([40, 33, 0, 1, 40, 17], dtype=torch.int64)
    ref_np = rng.randint(1, C, size=(B, U)).astype(np.int32)
    rl_np = np.array([12, 5, 3, 0, 9, 12], np.int32)
    ref, rl = _dev(ref_np), _dev(rl_np)
    tokens, lengths, scores = torch_loss.ctc_beam_decode(log_probs, blank=0, input_lengths=frames, beam_size=8,
                                                         cutoff_top_n=4, nbest=nbest)
    dist, ops = torch_loss.edit_distance(tokens, lengths, ref, rl, return_ops=True)
    labels, _, best_tokens, _, best_lengths = torch_loss.ctc_decode(log_probs, blank=0, input_lengths=frames)
    best = torch_loss.edit_distance(best_tokens, best_lengths, ref, rl)
    tokens, lengths, dist, ops = (t.cpu().numpy() for t in (tokens, lengths, dist, ops))
    best_tokens, best_lengths, best = (t.cpu().numpy() for t in (best_tokens, best_lengths, best))
    assert dist.shape == (B, nbest) and ops.shape == (B, nbest, 3) and best.shape == (B,)
    assert lengths[0].max() > 0
    for b in range(B):
        r = ref_np[b, :rl_np[b]]
        for k in range(nbest):
            want, want_ops, _ = fp.distance_ops(r, tokens[b, k, :lengths[b, k]])
            assert dist[b, k] == want and tuple(ops[b, k]) == want_ops, (b, k)
        assert best[b] == fp.distance_ops(r, best_tokens[b, :best_lengths[b]])[0], b
    # a slot without a hypothesis (no frames: length 0, tokens -1) scores the reference's length
    assert (lengths[2] == 0).all() and (dist[2] == rl_np[2]).all()
