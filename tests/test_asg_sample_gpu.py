"""Batched ASG posterior sampling with device-resident output (asg_sample.hip through gtnx_batch_asg_sample;
gtn_amd.Batch.asg_sample, gtn_amd.torch_loss.asg_sample, gtn_asg_sample_n).

The judge is the certificate of tests/asg_sample_fp.py (test_asg_sample_cpu.py shows that it has teeth): every returned
label has mass in float64, every returned alignment a finite score, the Philox uniform of every (b, k, t) is bracketed by
the float64 conditional CDF given the device's own y_{t+1} within tol(C) + 32 d (d: the drift of float32 planes from
float64 ones that the yardstick measures on the case), tokens and lengths == the merge of the returned labels, logq within
(T + 8) * 2^-24 * sum |term| + T * 32 d of the float64 s(y) / tau - logZ, logz within 1e-4 * max(1, |logz|); -1 fills
exact.  No sample is left out.  Every output is allocated with a guard row and guard columns of sentinels that must
survive.  Every certifying test prints its worst bracket miss as a multiple of the tolerance.
"""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import asg_sample_fp as fp

pytestmark = pytest.mark.gpu
SENTINEL = -7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tokens", "lengths", "logq", "labels", "logz")


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True, order="C")).to("cuda:0")


def _sample(gtn, em, table, frames=None, rows=None, N=4, seed=1, tau=1.0, logq=True, labels=True, logz=True, pad=1,
            address=False, batch=None):
    """Batch.asg_sample on Batch.linear (or on `batch`); outputs allocated with a guard row (one more utterance) and
    `pad` guard columns of sentinels that must survive (pad > 1: row_stride > T; address: raw device addresses with
    row_stride).  Returns ([tokens, lengths, logq, labels, logz] as numpy, None where not asked for, (calls, utterances)
    of this call); _sample.raw keeps the arrays with their guards, also when the call raised"""
    import torch
    B, T, C = em.shape
    em_dev, table_dev = _dev(em), _dev(table)
    ems = batch if batch is not None else gtn.Batch.linear(B, T, C, em_dev, False, True, rows)

    def rows_of(on):
        return torch.full((B + 1, N, T + pad), SENTINEL, dtype=torch.int32, device="cuda:0") if on else None
    tok, lab = rows_of(True), rows_of(labels)
    ln = torch.full((B + 1, N), SENTINEL, dtype=torch.int32, device="cuda:0")
    lq = torch.full((B + 1, N), float("nan"), dtype=torch.float32, device="cuda:0") if logq else None
    lz = torch.full((B + 1,), float("nan"), dtype=torch.float32, device="cuda:0") if logz else None
    torch.cuda.synchronize()

    def view(t):
        if t is None:
            return None
        return t.data_ptr() if address else t[:B, :, :T]
    c0, u0 = gtn.debug_asg_sample_stats()
    try:
        ems.asg_sample(view(tok), ln.data_ptr() if address else ln[:B], table_dev.data_ptr() if address else table_dev,
                       None if lq is None else lq[:B], view(lab), None if lz is None else lz[:B], frames, N, seed, tau,
                       row_stride=T + pad if address else None)
    finally:
        gtn.synchronize()
        c1, u1 = gtn.debug_asg_sample_stats()
        raw = [None if t is None else t.cpu().numpy() for t in (tok, ln, lq, lab, lz)]
        _sample.raw = raw
        for name, r in zip(NAMES, raw):
            if r is None:
                continue
            if r.ndim == 3:
                assert (r[B] == SENTINEL).all() and (r[:, :, T:] == SENTINEL).all(), name
            elif name in ("logq", "logz"):
                assert np.isnan(r[B]).all(), name
            else:
                assert (r[B] == SENTINEL).all(), name
    out = [None if r is None else (r[:B, :, :T] if r.ndim == 3 else r[:B]) for r in raw]
    return out, (c1 - c0, u1 - u0)


def _certify(tag, em, table, got, frames=None, N=4, seed=1, tau=1.0):
    tokens, lengths, logq, labels, logz = got
    worst = fp.certify(em, table, frames, N, seed, tau, tokens, lengths, logq, labels, logz, tag=tag)
    print(f"[asg_sample] {tag}: worst bracket miss {worst:.3e} of tol(C) + 32 d")
    return worst


def _same(tag, a, b):
    for name, x, y in zip(NAMES, a, b):
        if x is None or y is None:
            continue
        assert x.tobytes() == y.tobytes(), (tag, name, np.argwhere(x != y)[:5].tolist())


@functools.lru_cache(maxsize=None)
def _noise(seed, B, T, C):
    em, table = fp.continuous_case(seed, B, T, C)
    em.setflags(write=False)
    table.setflags(write=False)
    return em, table


@pytest.mark.parametrize("C,T,B,N", fp.SHAPES)
def test_sample_passes_the_certificate(gtn, C, T, B, N):
    em, table, seed = fp.shape_case(C, T, B, N)
    got, stats = _sample(gtn, em, table, N=N, seed=seed)
    assert stats == (1, B)
    _certify(f"C={C} T={T} B={B} N={N}", em, table, got, N=N, seed=seed)


@pytest.mark.parametrize("C", [2, 29, 65, 128, 129, 300])
def test_peaked_transitions(gtn, C):
    """after every label one successor holds mass 1 - 1e-6: nearly every step of a sample follows it (another label only
    where u falls into the 1e-6: the certificate decides)"""
    B, T, N = 3, 65, 8
    em, table, succ = fp.peaked_case(300 + C, B, T, C)
    got, _ = _sample(gtn, em, table, N=N, seed=C)
    _certify(f"peaked C={C}", em, table, got, N=N, seed=C)
    lab = got[3]
    hit = (lab[:, :, 1:] == succ[lab[:, :, :-1]]).mean()
    print(f"[asg_sample] peaked C={C}: {hit:.6f} of the steps follow the successor")
    assert hit >= 1.0 - 1e-3  # (B * N * (T - 1) = 1536 steps at 1e-6 each: more than one miss has probability 1e-6)


@pytest.mark.parametrize("C", [1, 3, 29, 64, 65, 129, 300])
def test_equal_masses(gtn, C):
    """all alignments alike: every step of every CDF is 1 / C, the label is floor(u C)"""
    B, T, N = 3, 9, 17
    em, table = fp.equal_case(B, T, C)
    got, _ = _sample(gtn, em, table, N=N, seed=5)
    _certify(f"equal C={C}", em, table, got, N=N, seed=5)
    u = fp.uniforms(5, B, N, T)
    want = np.minimum(np.floor(u * C), C - 1)
    assert (got[3] == want).mean() > 0.999
    assert np.allclose(got[4], T * np.log(C), atol=1e-4 * max(1.0, T * np.log(C)))


@pytest.mark.parametrize("C", [3, 29, 65, 129, 300])
def test_holes_are_never_on_a_path(gtn, C):
    """-inf, +inf and NaN in the emissions, the transitions and the start scores"""
    B, T, N = 3, 40, 9
    em, table = fp.holes_case(40 + C, B, T, C)
    got, _ = _sample(gtn, em, table, N=N, seed=3)
    _certify(f"holes C={C}", em, table, got, N=N, seed=3)
    lab = got[3].astype(np.int64)
    start, W = fp.split(table, C)
    assert np.isfinite(em[np.arange(B)[:, None, None], np.arange(T)[None, None, :], lab]).all()
    assert np.isfinite(W[lab[:, :, 1:], lab[:, :, :-1]]).all() and np.isfinite(start[lab[:, :, 0]]).all()
    assert np.isfinite(got[2]).all() and np.isfinite(got[4]).all()


@pytest.mark.parametrize("C", [4, 65, 300])
def test_dead_ends_are_drawn_at_the_last_frame_only(gtn, C):
    B, T, N = 3, 30, 16
    em, table, dead = fp.dead_end_case(9 + C, B, T, C)
    got, _ = _sample(gtn, em, table, N=N, seed=2)
    _certify(f"dead end C={C}", em, table, got, N=N, seed=2)
    assert not (got[3][:, :, :-1] == dead).any()


@pytest.mark.parametrize("C", [3, 65, 300])
def test_no_path_beside_ordinary_neighbours(gtn, C):
    """a frame of -inf, T_b = 0, and (a call of its own) every start forbidden: -1 rows, length 0, logq -inf, logz -inf;
    the neighbours are what they are without it"""
    B, T, N = 5, 70, 5
    em0, table = _noise(7 + C, B, T, C)
    em = np.array(em0)
    em[1, 33] = -np.inf
    em[3, 69] = np.nan
    em[3, 69, 0] = np.inf
    frames = [T, T, 0, T, T - 1]
    got, _ = _sample(gtn, em, table, frames=frames, N=N, seed=4)
    _certify(f"no path C={C}", em, table, got, frames=frames, N=N, seed=4)
    for b in (1, 2, 3):
        assert (got[0][b] == -1).all() and (got[3][b] == -1).all() and (got[1][b] == 0).all()
        assert np.isneginf(got[2][b]).all() and np.isneginf(got[4][b])
    clean, _ = _sample(gtn, em0, table, frames=[T, T, T, T, T - 1], N=N, seed=4)
    for b in (0, 4):
        for g, c in zip(got, clean):
            assert g[b].tobytes() == c[b].tobytes()
    closed = np.array(table)
    closed[:C] = [-np.inf, np.inf, np.nan][C % 3]
    got, _ = _sample(gtn, em0, closed, N=N, seed=4)
    _certify(f"no start C={C}", em0, closed, got, N=N, seed=4)
    assert (got[3] == -1).all() and (got[1] == 0).all() and np.isneginf(got[2]).all() and np.isneginf(got[4]).all()


@pytest.mark.parametrize("C,T", [(29, 65), (300, 130)])
def test_ragged_batches(gtn, C, T):
    """frame counts with 0, 1 and T among them; NaN in every pad row changes no byte; every utterance equals itself run
    alone at its own length (at its own place in the batch: the counter has the batch index)"""
    B, N = 6, 5
    em, table = _noise(11 + C, B, T, C)
    counts = [T, T - 1, 1, 0, T // 2, 64]
    by_frames, _ = _sample(gtn, em, table, frames=counts, N=N, seed=8)
    _certify(f"ragged C={C}", em, table, by_frames, frames=counts, N=N, seed=8)
    poisoned = np.array(em)
    for b, t in enumerate(counts):
        poisoned[b, t:] = np.nan
    _same("NaN pads", _sample(gtn, poisoned, table, frames=counts, N=N, seed=8)[0], by_frames)
    none, _ = _sample(gtn, em, table, N=N, seed=8)
    _same("full frames", _sample(gtn, em, table, frames=[T] * B, N=N, seed=8)[0], none)
    rows = [max(c, 1) for c in counts]  # (a chain carries at least one row)
    both, _ = _sample(gtn, em, table, frames=counts, rows=rows, N=N, seed=8)
    _same("frames and rows", both, by_frames)
    for b in (0, 2, 4):
        t = counts[b]
        alone = np.zeros((b + 1, t, C), np.float32)  # (utterance b alone at its own length, the ones before it empty)
        alone[b] = em[b, :t]
        one, _ = _sample(gtn, alone, table, frames=[0] * b + [t], N=N, seed=8)
        assert one[3][b].tobytes() == np.ascontiguousarray(by_frames[3][b, :, :t]).tobytes()
        assert one[0][b].tobytes() == np.ascontiguousarray(by_frames[0][b, :, :t]).tobytes()
        for i in (1, 2, 4):
            assert one[i][b].tobytes() == by_frames[i][b].tobytes()


def test_determinism_and_independence(gtn, monkeypatch):
    B, T, C, N = 5, 130, 65, 17
    em, table = _noise(77, B, T, C)
    a, _ = _sample(gtn, em, table, N=N, seed=31)
    _certify("determinism", em, table, a, N=N, seed=31)
    _same("same seed", _sample(gtn, em, table, N=N, seed=31)[0], a)
    other, _ = _sample(gtn, em, table, N=N, seed=32)
    assert (other[3] != a[3]).mean() > 0.5
    high, _ = _sample(gtn, em, table, N=N, seed=31 + (1 << 40))
    assert (high[3] != a[3]).mean() > 0.5
    _same("wide rows", _sample(gtn, em, table, N=N, seed=31, pad=7)[0], a)
    _same("addresses", _sample(gtn, em, table, N=N, seed=31, pad=3, address=True)[0], a)
    five, _ = _sample(gtn, em, table, N=5, seed=31)
    for x, y in zip(five, a):
        assert x.tobytes() == (y if y.ndim == 1 else np.ascontiguousarray(y[:, :5])).tobytes()
    # sliced scratch: one utterance per slice (planes plus 4 or 8 bytes per cell), and a cap below one utterance
    c0, u0 = gtn.debug_asg_sample_stats()
    monkeypatch.setenv("GTNX_ASG_SAMPLE_SCRATCH_BYTES", str(4 * T * C + 4 * N * T + 1))
    _same("sliced", _sample(gtn, em, table, N=N, seed=31)[0], a)
    monkeypatch.setenv("GTNX_ASG_SAMPLE_SCRATCH_BYTES", str(2 * (4 * T * C + 8 * N * T)))
    _same("sliced, no labels", _sample(gtn, em, table, N=N, seed=31, labels=False)[0], a)
    monkeypatch.setenv("GTNX_ASG_SAMPLE_SCRATCH_BYTES", "1")
    _same("a slice above the cap runs alone", _sample(gtn, em, table, N=N, seed=31, labels=False)[0], a)
    monkeypatch.delenv("GTNX_ASG_SAMPLE_SCRATCH_BYTES")
    assert gtn.debug_asg_sample_stats() == (c0 + 3, u0 + 3 * B)  # (a sliced call is one call)


def test_slicing_above_the_register_variant(gtn, monkeypatch):
    """the wide filter carries four utterances per workgroup: slices of one and of three give the bytes of the whole"""
    B, T, C, N = 6, 20, 140, 5
    em, table = _noise(78, B, T, C)
    counts = [T, 3, 0, T, 7, T - 1]
    a, _ = _sample(gtn, em, table, frames=counts, N=N, seed=9)
    _certify("wide slices", em, table, a, frames=counts, N=N, seed=9)
    per = 4 * T * C + 4 * N * T
    for k in (1, 3):
        monkeypatch.setenv("GTNX_ASG_SAMPLE_SCRATCH_BYTES", str(k * per + 1))
        _same(f"{k} per slice", _sample(gtn, em, table, frames=counts, N=N, seed=9)[0], a)


@pytest.mark.parametrize("tau", [0.5, 2.0])
def test_temperature(gtn, tau):
    B, T, C, N = 3, 65, 29, 8
    em, table = fp.continuous_case(55, B, T, C, scale=1.0)
    got, _ = _sample(gtn, em, table, N=N, seed=6, tau=tau)
    _certify(f"tau={tau}", em, table, got, N=N, seed=6, tau=tau)
    with pytest.raises(AssertionError):  # (the same result judged at temperature 1)
        fp.certify(em, table, None, N, 6, 1.0, *got)
    with pytest.raises(AssertionError):  # (and the labels alone)
        fp.certify(em, table, None, N, 6, 1.0, got[0], got[1], None, got[3], None)


def test_distribution_end_to_end(gtn):
    """256 copies of one slab (T = 4, C = 3, one bigram forbidden, one favoured), N = 16: the frequency of every
    alignment and of every label sequence over the 4096 samples is within 5 sqrt(p (1 - p) / 4096) of the enumerated
    probability"""
    from test_asg_sample_cpu import STAT_B, STAT_N, STAT_SEED, check_frequencies, stat_model
    slab, table = stat_model()
    em = np.broadcast_to(slab, (STAT_B,) + slab.shape).copy()
    got, _ = _sample(gtn, em, table, N=STAT_N, seed=STAT_SEED)
    _certify("distribution", em, table, got, N=STAT_N, seed=STAT_SEED)
    check_frequencies(got[3], got[0], got[1], slab, table)


def test_chain(gtn):
    """asg_score of the sampled tokens is finite and >= logq + logz - 1e-4 |.| (a sequence's mass contains its
    alignment's); logz is asg_loss's full-connect term; edit_distance and asg_token_align take the tensors as they
    are; the sampled-risk recipe runs backward"""
    import torch
    from gtn_amd import torch_loss
    B, T, C, N = 4, 50, 9, 6
    em, table = _noise(91, B, T, C)
    start, W = fp.split(table, C)
    x, tr, st = _dev(em), _dev(W), _dev(start)
    lens = [T, T - 3, 20, 1]
    tokens, lengths, logq, logz = torch_loss.asg_sample(x, tr, st, lens, N, seed=12, return_logz=True)
    score = torch_loss.asg_score(x, tr, tokens, lengths, st, lens)
    ref = torch.randint(1, C, (B, 7), dtype=torch.int32, device="cuda:0")
    ref_len = torch.tensor([7, 5, 3, 1], dtype=torch.int32, device="cuda:0")
    dist = torch_loss.edit_distance(tokens, lengths, ref, ref_len)
    al = torch_loss.asg_token_align(x, tr, tokens, lengths, st, lens)
    # the full-connect term of asg_loss: loss = full-connect - force-align, the latter is asg_score of the target
    targets = [[1], [2, 3], [4], [5]]
    tt = torch.full((B, 1, 2), -1, dtype=torch.int32, device="cuda:0")
    for b, y in enumerate(targets):
        tt[b, 0, :len(y)] = torch.tensor(y, dtype=torch.int32)
    tl = torch.tensor([[len(y)] for y in targets], dtype=torch.int32, device="cuda:0")
    loss = torch_loss.asg_loss(x, tr, targets, st, input_lengths=lens)
    fal = torch_loss.asg_score(x, tr, tt, tl, st, lens)[:, 0]
    torch.cuda.synchronize()
    fcc = loss.cpu().numpy().astype(np.float64) + fal.cpu().numpy().astype(np.float64)
    z = logz.cpu().numpy().astype(np.float64)
    print(f"[asg_sample] chain: logz - full-connect max {np.abs(z - fcc).max():.3e}")
    assert (np.abs(z - fcc) <= 1e-4 * np.maximum(1.0, np.abs(fcc))).all()
    s, q = score.cpu().numpy().astype(np.float64), logq.cpu().numpy().astype(np.float64)
    lower = q + z[:, None]
    print(f"[asg_sample] chain: score - (logq + logz) min {np.min(s - lower):.3e}")
    assert np.isfinite(s).all() and (s >= lower - 1e-4 * np.abs(lower)).all()
    assert dist.shape == (B, N) and (dist.cpu().numpy() >= 0).all()
    assert al[0].shape == (B, N) and np.isfinite(al[0].cpu().numpy()).all()
    # the sampled-risk recipe runs end to end on the device
    xg, tg = x.clone().requires_grad_(True), tr.clone().requires_grad_(True)
    sc = torch_loss.asg_score(xg, tg, tokens, lengths, st, lens)
    err = dist.float()
    risk = ((err - err.mean(1, keepdim=True)).detach() * (sc - logz[:, None])).mean()
    risk.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(xg.grad).all() and xg.grad.abs().sum() > 0
    assert torch.isfinite(tg.grad).all() and tg.grad.abs().sum() > 0


@pytest.mark.parametrize("logq", [True, False])
@pytest.mark.parametrize("labels", [True, False])
@pytest.mark.parametrize("logz", [True, False])
def test_optional_outputs(gtn, logq, labels, logz):
    B, T, C, N = 3, 70, 29, 5
    em, table = _noise(3, B, T, C)
    full, _ = _sample(gtn, em, table, frames=[T, 9, 64], N=N, seed=77)
    got, stats = _sample(gtn, em, table, frames=[T, 9, 64], N=N, seed=77, logq=logq, labels=labels, logz=logz)
    assert stats == (1, B)
    assert (got[2] is None) == (not logq) and (got[3] is None) == (not labels) and (got[4] is None) == (not logz)
    _same(f"optional logq={logq} labels={labels} logz={logz}", got, full)


def test_bad_arguments_raise_and_write_nothing(gtn):
    import torch
    B, T, C, N = 2, 6, 5, 4
    em, table = _noise(1, B, T, C)
    cases = [dict(frames=[T + 1, 1]), dict(frames=[-1, 1]), dict(rows=[3, 6], frames=[4, 6]), dict(N=0), dict(N=1025),
             dict(tau=0.0), dict(tau=float("inf")), dict(tau=float("nan")), dict(tau=-1.0), dict(seed=-1),
             dict(seed=1 << 64)]
    c0 = gtn.debug_asg_sample_stats()
    for kw in cases:
        with pytest.raises(ValueError, match="asg_sample"):
            _sample(gtn, em, table, **({"N": N} | kw))
        for name, r in zip(NAMES, _sample.raw):
            assert (np.isnan(r) if name in ("logq", "logz") else r == SENTINEL).all(), (kw, name)
    # more labels than the cap: refused with the range in the message
    wide, wtable = np.zeros((1, 2, 1025), np.float32), np.zeros(1025 + 1025 * 1025, np.float32)
    with pytest.raises(ValueError, match=r"gtnx_batch_asg_sample.*outside 1 \.\. 1024"):
        _sample(gtn, wide, wtable, N=N)
    for name, r in zip(NAMES, _sample.raw):
        assert (np.isnan(r) if name in ("logq", "logz") else r == SENTINEL).all(), ("C", name)
    # row_stride < M, as raw addresses; a table of the wrong size
    tok = torch.full((B, N, T), SENTINEL, dtype=torch.int32, device="cuda:0")
    ln = torch.full((B, N), SENTINEL, dtype=torch.int32, device="cuda:0")
    tab = _dev(table)
    ems = gtn.Batch.linear(B, T, C, _dev(em), False, True)
    with pytest.raises(ValueError, match="gtnx_batch_asg_sample.*row_stride is shorter"):
        ems.asg_sample(tok.data_ptr(), ln, tab, row_stride=T - 1)
    with pytest.raises(ValueError, match="asg_sample.*rows of"):
        ems.asg_sample(tok[:, :, :T - 1], ln, tab)
    with pytest.raises(ValueError, match="asg_sample: table has"):
        ems.asg_sample(tok, ln, tab[:-1])
    # not a native linear batch: there is no other route
    with pytest.raises(ValueError, match="gtnx_batch_asg_sample.*not a native linear batch"):
        gtn.Batch([gtn.linear_graph(T, C) for _ in range(B)]).asg_sample(tok.data_ptr(), ln.data_ptr(), tab.data_ptr(),
                                                                         row_stride=T)
    gtn.synchronize()
    assert (tok == SENTINEL).all() and (ln == SENTINEL).all()
    assert gtn.debug_asg_sample_stats() == c0


TORCH_CASES = [(1, 3, 70, 29, True), (2, 2, 64, 300, False), (3, 1, 5, 3, True)]


def _torch_frames(seed, B, T):
    rng = np.random.default_rng(seed)
    fr = rng.integers(0, T + 1, B)
    fr[0] = T
    return fr.tolist()


def _torch_entry(em, table, frames, N, seed, side_stream, extras=True, tau=1.0):
    import torch
    from gtn_amd import torch_loss
    B, T, C = em.shape
    start, W = fp.split(table, C)
    x, tr, st = _dev(em), _dev(W), _dev(start)
    before = x.clone()
    lens = None if frames is None else torch.tensor(frames)
    torch.cuda.synchronize()

    def call():
        return torch_loss.asg_sample(x, tr, st, lens, N, tau, seed, extras, extras)
    if side_stream:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            out = call()
        s.synchronize()
    else:
        out = call()
        torch.cuda.synchronize()
    kinds = [(torch.int32, (B, N, T)), (torch.int32, (B, N)), (torch.float32, (B, N)), (torch.int32, (B, N, T)),
             (torch.float32, (B,))]
    assert len(out) == (5 if extras else 3)
    for o, (dt, shape) in zip(out, kinds):
        assert o.dtype == dt and tuple(o.shape) == shape and o.device == x.device and not o.requires_grad
    assert torch.equal(x, before)
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("side_stream", [True, False])
@pytest.mark.parametrize("seed,B,T,C,ragged", TORCH_CASES)
def test_torch_entry(gtn, seed, B, T, C, ragged, side_stream):
    frames = _torch_frames(seed, B, T) if ragged else None
    em, table = _noise(seed, B, T, C)
    c0, u0 = gtn.debug_asg_sample_stats()
    out = _torch_entry(em, table, frames, 5, 900 + seed, side_stream)
    assert gtn.debug_asg_sample_stats() == (c0 + 1, u0 + B)
    _certify(f"torch seed={seed}", em, table, out, frames=frames, N=5, seed=900 + seed)
    three = _torch_entry(em, table, frames, 5, 900 + seed, side_stream, extras=False)
    _same("without labels and logz", three + [None, None], out)
    # start omitted is a start of zeros
    import torch
    from gtn_amd import torch_loss
    zero = np.array(table)
    zero[:C] = 0.0
    got = torch_loss.asg_sample(_dev(em), _dev(fp.split(table, C)[1]), None, frames, 5, 1.0, 900 + seed, True, True)
    torch.cuda.synchronize()
    _certify(f"torch seed={seed}, no start", em, zero, [o.cpu().numpy() for o in got], frames=frames, N=5, seed=900 + seed)


def test_torch_seed_none_repeats_under_manual_seed(gtn):
    import torch
    em, table = _noise(4, 2, 40, 9)
    torch.manual_seed(4321)
    a = _torch_entry(em, table, None, 4, None, False)
    b = _torch_entry(em, table, None, 4, None, False)
    torch.manual_seed(4321)
    c = _torch_entry(em, table, None, 4, None, False)
    _same("manual_seed", a, c)
    assert (a[3] != b[3]).mean() > 0.3
    torch.manual_seed(4321)
    want = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
    _same("the seed is the generator's draw", _torch_entry(em, table, None, 4, want, False), a)


_CHILD = "--python-criteria-child"


def test_torch_entry_python_route(tmp_path):
    """GTN_AMD_PYTHON_CRITERIA=1 in a fresh process: Batch.linear(borrow).asg_sample gives the native route's bytes"""
    out = str(tmp_path / "child.npz")
    env = dict(os.environ, GTN_AMD_PYTHON_CRITERIA="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), _CHILD, out], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    z = np.load(out)
    for i, (seed, B, T, C, ragged) in enumerate(TORCH_CASES):
        frames = _torch_frames(seed, B, T) if ragged else None
        em, table = _noise(seed, B, T, C)
        got = [z[f"o{i}_{k}"] for k in range(5)]
        _certify(f"python route {i}", em, table, got, frames=frames, N=5, seed=900 + seed)
        _same(f"python route {i} == native", got, _torch_entry(em, table, frames, 5, 900 + seed, False))
    assert int(z["calls"]) == len(TORCH_CASES) and int(z["native"]) == 0


def _python_route_child(out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gtn_amd as gtn
    from gtn_amd import torch_loss
    res = {"native": int(bool(torch_loss._native()))}
    for i, (seed, B, T, C, ragged) in enumerate(TORCH_CASES):
        frames = _torch_frames(seed, B, T) if ragged else None
        em, table = _noise(seed, B, T, C)
        for k, o in enumerate(_torch_entry(em, table, frames, 5, 900 + seed, bool(i % 2))):
            res[f"o{i}_{k}"] = o
    res["calls"] = gtn.debug_asg_sample_stats()[0]
    np.savez(out, **res)


def test_dense_rows_c_entry(gtn):
    """gtn_asg_sample_n of libgtn_criteria.so on dense [B][N][T] rows"""
    import torch
    B, T, C, N = 3, 66, 29, 5
    em, table = _noise(21, B, T, C)
    frames = np.array([T, 10, 0], np.int32)
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.gtn_asg_sample_n.argtypes = [P, I, I, I, P, P, I, ctypes.c_uint64, ctypes.c_float, P, P, P, P, P]
    lib.gtn_asg_sample_n.restype = I
    lib.gtn_criteria_last_error.restype = ctypes.c_char_p
    x, tab = _dev(em), _dev(table)
    tok = torch.full((B, N, T), SENTINEL, dtype=torch.int32, device="cuda:0")
    lab = torch.full((B, N, T), SENTINEL, dtype=torch.int32, device="cuda:0")
    ln = torch.full((B, N), SENTINEL, dtype=torch.int32, device="cuda:0")
    lq = torch.full((B, N), float("nan"), dtype=torch.float32, device="cuda:0")
    lz = torch.full((B,), float("nan"), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    gtn.set_stream(None)
    seed = (1 << 63) + 5
    rc = lib.gtn_asg_sample_n(x.data_ptr(), B, T, C, tab.data_ptr(), frames.ctypes.data, N, seed, 1.0, tok.data_ptr(),
                              ln.data_ptr(), lq.data_ptr(), lab.data_ptr(), lz.data_ptr())
    assert rc == 0, lib.gtn_criteria_last_error().decode()
    gtn.synchronize()
    got = [t.cpu().numpy() for t in (tok, ln, lq, lab, lz)]
    _certify("gtn_asg_sample_n", em, table, got, frames=frames.tolist(), N=N, seed=seed)
    _same("== Batch.asg_sample", got, _sample(gtn, em, table, frames=frames.tolist(), N=N, seed=seed)[0])
    rc = lib.gtn_asg_sample_n(x.data_ptr(), B, T, C, tab.data_ptr(), None, 0, seed, 1.0, tok.data_ptr(), ln.data_ptr(),
                              None, None, None)
    assert rc != 0 and "gtnx_batch_asg_sample" in lib.gtn_criteria_last_error().decode()


def test_stats_count_calls_and_utterances(gtn):
    em, table = _noise(2, 4, 10, 5)
    c0, u0 = gtn.debug_asg_sample_stats()
    _sample(gtn, em, table, N=1)
    _sample(gtn, em[:3], table, N=9)
    assert gtn.debug_asg_sample_stats() == (c0 + 2, u0 + 7)


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == _CHILD:
    _python_route_child(sys.argv[2])
