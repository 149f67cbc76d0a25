"""Batched CTC posterior sampling with device-resident output (ctc_sample.hip through gtnx_batch_ctc_sample;
gtn_amd.Batch.ctc_sample, gtn_amd.torch_loss.ctc_sample, gtn_ctc_sample_n).

The judge is the certificate of tests/ctc_sample_fp.py (test_ctc_sample_cpu.py shows that it has teeth): every returned
label carries mass and brackets the Philox uniform of its (b, k, t) within tol(C) = (4 C + 64) * 2^-24 of the float64
CDF; tokens and lengths == the collapse of the returned labels; logq within (T + 8) * 2^-24 * sum |term| of the float64
sum of the returned labels' terms; -1 fills exact.  No sample is left out.  Every output is allocated with a guard row
and guard columns of sentinels that must survive.
"""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import ctc_sample_fp as fp

pytestmark = pytest.mark.gpu
SENTINEL = -7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tokens", "lengths", "logq", "labels")


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True, order="C")).to("cuda:0")


def _sample(gtn, em, frames=None, rows=None, blank=0, N=4, seed=1, tau=1.0, logq=True, labels=True, pad=1,
            address=False, batch=None):
    """Batch.ctc_sample on Batch.linear (or on `batch`); outputs allocated with a guard row (one more utterance) and
    `pad` guard columns of sentinels that must survive (pad > 1: row_stride > T; address: raw device addresses with
    row_stride).  Returns ([tokens, lengths, logq, labels] as numpy, None where not asked for, (calls, utterances) of
    this call); _sample.raw keeps the arrays with their guards, also when the call raised"""
    import torch
    B, T, C = em.shape
    em_dev = _dev(em)
    ems = batch if batch is not None else gtn.Batch.linear(B, T, C, em_dev, False, True, rows)

    def rows_of(on):
        return torch.full((B + 1, N, T + pad), SENTINEL, dtype=torch.int32, device="cuda:0") if on else None
    tok, lab = rows_of(True), rows_of(labels)
    ln = torch.full((B + 1, N), SENTINEL, dtype=torch.int32, device="cuda:0")
    lq = torch.full((B + 1, N), float("nan"), dtype=torch.float32, device="cuda:0") if logq else None
    torch.cuda.synchronize()

    def view(t):
        if t is None:
            return None
        return t.data_ptr() if address else t[:B, :, :T]
    c0, u0 = gtn.debug_ctc_sample_stats()
    try:
        ems.ctc_sample(view(tok), ln.data_ptr() if address else ln[:B], None if lq is None else lq[:B], view(lab),
                       frames, blank, N, seed, tau, row_stride=T + pad if address else None)
    finally:
        gtn.synchronize()
        c1, u1 = gtn.debug_ctc_sample_stats()
        raw = [None if t is None else t.cpu().numpy() for t in (tok, ln, lq, lab)]
        _sample.raw = raw
        for name, r in zip(NAMES, raw):
            if r is None:
                continue
            if r.ndim == 3:
                assert (r[B] == SENTINEL).all() and (r[:, :, T:] == SENTINEL).all(), name
            elif name == "logq":
                assert np.isnan(r[B]).all(), name
            else:
                assert (r[B] == SENTINEL).all(), name
    out = [None if r is None else (r[:B, :, :T] if r.ndim == 3 else r[:B]) for r in raw]
    return out, (c1 - c0, u1 - u0)


def _certify(tag, em, got, frames=None, blank=0, N=4, seed=1, tau=1.0):
    tokens, lengths, logq, labels = got
    worst = fp.certify(em, frames, blank, N, seed, tau, tokens, lengths, logq, labels, tag=tag)
    print(f"[ctc_sample] {tag}: worst bracket miss {worst:.3e} of tol(C)")
    return worst


def _same(tag, a, b):
    for name, x, y in zip(NAMES, a, b):
        if x is None or y is None:
            continue
        assert x.tobytes() == y.tobytes(), (tag, name, np.argwhere(x != y)[:5].tolist())


@functools.lru_cache(maxsize=None)
def _noise(seed, B, T, C):
    em = fp.continuous_case(seed, B, T, C)
    em.setflags(write=False)
    return em


# C: each lanes-per-row variant (<= 32, <= 64, <= 128, above), rows that are not 16-byte aligned, with head and tail (3,
# 9, 29, 65, 300, 1025), rows of many tiles (1025, 5000).  T: the 64-frame collapse blocks and the rows per workgroup of
# every variant.  B: 1, 3, 70.  N: the four-sample Philox groups (1, 3, 4, 5, 17).  blank: first, last, none.
SHAPES = [(1, 1, 1, 1, 0), (1, 65, 3, 5, -1), (3, 1, 3, 4, 0), (3, 63, 70, 3, 2), (9, 64, 3, 17, 8), (9, 200, 1, 4, -1),
          (29, 65, 70, 1, 0), (29, 200, 3, 5, 28), (64, 129, 1, 17, 63), (64, 63, 3, 3, 0), (65, 129, 3, 4, 0),
          (65, 64, 1, 5, -1), (256, 200, 3, 4, 255), (256, 64, 70, 3, 0), (300, 65, 3, 17, -1), (300, 1, 1, 4, 299),
          (1025, 129, 3, 5, 0), (1025, 63, 1, 1, 1024), (5000, 63, 3, 4, 4999), (5000, 129, 1, 17, 0)]


@pytest.mark.parametrize("C,T,B,N,blank", SHAPES)
def test_sample_passes_the_certificate(gtn, C, T, B, N, blank):
    em = _noise(100 + C + T, B, T, C)
    got, stats = _sample(gtn, em, blank=blank, N=N, seed=1000 + C)
    assert stats == (1, B)
    _certify(f"C={C} T={T} B={B} N={N} blank={blank}", em, got, blank=blank, N=N, seed=1000 + C)
    if C > 3 and T >= 63 and blank >= 0:
        assert (got[1] > 0).all()


@pytest.mark.parametrize("C", [3, 29, 64, 65, 300, 1025])
def test_peaked_rows(gtn, C):
    """one label holds mass 1 - 1e-6: nearly every draw is it (a draw is another label only where u falls into the
    1e-6: the certificate decides), wherever the peak lies in the row"""
    B, T, N = 3, 65, 8
    em, peak = fp.peaked_case(300 + C, B, T, C)
    got, _ = _sample(gtn, em, blank=0, N=N, seed=C)
    _certify(f"peaked C={C}", em, got, blank=0, N=N, seed=C)
    hit = (got[3] == peak[:, None, :]).mean()
    print(f"[ctc_sample] peaked C={C}: {hit:.6f} of the draws are the peak")
    assert hit >= 1.0 - 1e-3  # (B * N * T = 1560 draws at 1e-6 each: more than one miss has probability 1e-6)


@pytest.mark.parametrize("C", [1, 3, 29, 64, 65, 300, 1025])
def test_equal_masses(gtn, C):
    """integer-valued rows: all-zero rows (every step of the CDF is 1 / C) and small integers"""
    B, T, N = 3, 9, 17
    rng = np.random.default_rng(C)
    for kind, em in (("zero", np.zeros((B, T, C), np.float32)),
                     ("int", rng.integers(-2, 3, (B, T, C)).astype(np.float32))):
        got, _ = _sample(gtn, em, blank=-1, N=N, seed=5)
        _certify(f"equal {kind} C={C}", em, got, blank=-1, N=N, seed=5)
        if kind == "zero" and C > 1:
            u = fp.uniforms(5, B, N, T)
            want = np.minimum(np.floor(u * C), C - 1)
            assert (np.abs(got[3] - want) <= 1).all() and (got[3] == want).mean() > 0.99


@pytest.mark.parametrize("C", [3, 9, 29, 65, 300, 1025])
def test_holes_are_never_chosen(gtn, C):
    """-inf, +inf and NaN entries carry no mass: never returned, left out of Z (the certificate's CDF skips them)"""
    B, T, N = 3, 40, 9
    em = fp.holes_case(40 + C, B, T, C, p=0.4)
    got, _ = _sample(gtn, em, blank=0, N=N, seed=9)
    _certify(f"holes C={C}", em, got, blank=0, N=N, seed=9)
    lab = got[3]
    assert np.isfinite(em[np.arange(B)[:, None, None], np.arange(T)[None, None, :], lab]).all()
    assert not np.isnan(got[2]).any() and np.isfinite(got[2]).all()


@pytest.mark.parametrize("C", [1, 3, 29, 64, 65, 300, 1025, 5000])
def test_a_single_finite_entry_at_the_last_label(gtn, C):
    B, T, N = 2, 5, 6
    em = np.full((B, T, C), np.nan, np.float32)
    em[0, :, :-1] = -np.inf
    em[1, 1::2, :-1] = np.inf
    em[:, :, -1] = 3.5
    got, _ = _sample(gtn, em, blank=-1, N=N, seed=2)
    _certify(f"single C={C}", em, got, blank=-1, N=N, seed=2)
    assert (got[3] == C - 1).all() and (got[1] == 1).all() and (got[2] == 0).all() and (got[0][:, :, 0] == C - 1).all()


@pytest.mark.parametrize("C", [3, 65, 300])
def test_no_path_beside_ordinary_neighbours(gtn, C):
    """a row without a finite entry, and T_b = 0: -1 rows, length 0, logq -inf for every sample of that utterance; the
    neighbours are what they are without it"""
    B, T, N = 5, 70, 5
    em = np.array(_noise(7 + C, B, T, C))
    em[1, 33] = -np.inf
    em[3, 69] = np.nan
    em[3, 69, 0] = np.inf
    frames = [T, T, 0, T, T - 1]
    got, _ = _sample(gtn, em, frames=frames, blank=0, N=N, seed=4)
    _certify(f"no path C={C}", em, got, frames=frames, blank=0, N=N, seed=4)
    for b in (1, 2, 3):
        assert (got[0][b] == -1).all() and (got[3][b] == -1).all() and (got[1][b] == 0).all()
        assert np.isneginf(got[2][b]).all()
    clean, _ = _sample(gtn, np.array(_noise(7 + C, B, T, C)), frames=[T, T, T, T, T - 1], blank=0, N=N, seed=4)
    for b in (0, 4):
        for g, c in zip(got, clean):
            assert g[b].tobytes() == c[b].tobytes()


@pytest.mark.parametrize("C,T", [(29, 65), (300, 130)])
def test_ragged_batches(gtn, C, T):
    """frame counts through `frames`, through `rows` and through both (T, T - 1, 1, 0 among them); NaN in every pad row
    changes no byte; full-length frames equals none"""
    B, N = 6, 5
    em = _noise(11 + C, B, T, C)
    counts = [T, T - 1, 1, 0, T // 2, 64]
    by_frames, _ = _sample(gtn, em, frames=counts, blank=0, N=N, seed=8)
    _certify(f"ragged C={C}", em, by_frames, frames=counts, blank=0, N=N, seed=8)
    rows = [T, T - 1, 1, 1, T // 2, 64]  # (a chain carries at least one row)
    counts_r = [T, T - 1, 1, 1, T // 2, 64]
    by_rows, _ = _sample(gtn, em, rows=rows, blank=0, N=N, seed=8)
    _certify(f"rows C={C}", em, by_rows, frames=counts_r, blank=0, N=N, seed=8)
    both, _ = _sample(gtn, em, frames=counts, rows=rows, blank=0, N=N, seed=8)
    _same("frames and rows", both, by_frames)
    for b in (0, 1, 2, 4, 5):
        for x, y in zip(by_rows, by_frames):
            assert x[b].tobytes() == y[b].tobytes()
    poisoned = np.array(em)
    for b, t in enumerate(counts):
        poisoned[b, t:] = np.nan
    _same("NaN pads", _sample(gtn, poisoned, frames=counts, blank=0, N=N, seed=8)[0], by_frames)
    none, _ = _sample(gtn, em, blank=0, N=N, seed=8)
    _same("full frames", _sample(gtn, em, frames=[T] * B, blank=0, N=N, seed=8)[0], none)
    # what the others' counts are changes nothing in the frames that count
    for b in range(B):
        t = counts[b]
        assert (by_frames[3][b, :, :t] == none[3][b, :, :t]).all()


def test_determinism_and_independence(gtn, monkeypatch):
    B, T, C, N = 5, 130, 65, 17
    em = _noise(77, B, T, C)
    a, _ = _sample(gtn, em, blank=0, N=N, seed=31)
    _certify("determinism", em, a, blank=0, N=N, seed=31)
    _same("same seed", _sample(gtn, em, blank=0, N=N, seed=31)[0], a)
    other, _ = _sample(gtn, em, blank=0, N=N, seed=32)
    assert (other[3] != a[3]).mean() > 0.5
    high, _ = _sample(gtn, em, blank=0, N=N, seed=31 + (1 << 40))
    assert (high[3] != a[3]).mean() > 0.5
    _same("wide rows", _sample(gtn, em, blank=0, N=N, seed=31, pad=7)[0], a)
    _same("addresses", _sample(gtn, em, blank=0, N=N, seed=31, pad=3, address=True)[0], a)
    five, _ = _sample(gtn, em, blank=0, N=5, seed=31)
    for x, y in zip(five, a):
        assert x.tobytes() == np.ascontiguousarray(y[:, :5]).tobytes()
    # sliced scratch: one utterance per slice with labels (4 bytes per cell), and without (8)
    c0, u0 = gtn.debug_ctc_sample_stats()
    monkeypatch.setenv("GTNX_CTC_SAMPLE_SCRATCH_BYTES", str(4 * N * T + 1))
    _same("sliced", _sample(gtn, em, blank=0, N=N, seed=31)[0], a)
    monkeypatch.setenv("GTNX_CTC_SAMPLE_SCRATCH_BYTES", str(2 * 8 * N * T))
    _same("sliced, no labels", _sample(gtn, em, blank=0, N=N, seed=31, labels=False)[0], a)
    monkeypatch.setenv("GTNX_CTC_SAMPLE_SCRATCH_BYTES", "1")
    _same("a slice above the cap runs alone", _sample(gtn, em, blank=0, N=N, seed=31, labels=False)[0], a)
    monkeypatch.delenv("GTNX_CTC_SAMPLE_SCRATCH_BYTES")
    assert gtn.debug_ctc_sample_stats() == (c0 + 3, u0 + 3 * B)  # (a sliced call is one call)


@pytest.mark.parametrize("tau", [0.5, 2.0])
def test_temperature(gtn, tau):
    B, T, C, N = 3, 65, 29, 8
    em = _noise(55, B, T, C)
    got, _ = _sample(gtn, em, blank=0, N=N, seed=6, tau=tau)
    _certify(f"tau={tau}", em, got, blank=0, N=N, seed=6, tau=tau)
    with pytest.raises(AssertionError):  # (the same labels judged at temperature 1)
        fp.certify(em, None, 0, N, 6, 1.0, got[0], got[1], None, got[3])


def test_distribution_end_to_end(gtn):
    """256 copies of one slab (T = 3, C = 3, blank 0), N = 16: the frequency of every label sequence over the 4096
    samples is within 5 sqrt(p (1 - p) / 4096) of exp(ctc_score - sum log Z) from float64"""
    from test_ctc_sample_cpu import STAT_B, STAT_N, STAT_SEED, check_frequencies, stat_slab
    slab = stat_slab()
    em = np.broadcast_to(slab, (STAT_B,) + slab.shape).copy()
    got, _ = _sample(gtn, em, blank=0, N=STAT_N, seed=STAT_SEED)
    _certify("distribution", em, got, blank=0, N=STAT_N, seed=STAT_SEED)
    check_frequencies(got[0], got[1], slab)


def test_chain(gtn):
    """ctc_score of the sampled tokens is finite and >= logq + sum log Z - 1e-4 |.| (a sequence's mass contains its
    alignment's); edit_distance and ctc_token_align take the tensors as they are"""
    import torch
    from gtn_amd import torch_loss
    B, T, C, N = 4, 50, 9, 6
    em = _noise(91, B, T, C)
    x = _dev(em)
    lens = [T, T - 3, 20, 1]
    tokens, lengths, logq = torch_loss.ctc_sample(x, 0, lens, N, seed=12)
    score = torch_loss.ctc_score(x, tokens, lengths, 0, lens)
    ref = torch.randint(1, C, (B, 7), dtype=torch.int32, device="cuda:0")
    ref_len = torch.tensor([7, 5, 3, 1], dtype=torch.int32, device="cuda:0")
    dist = torch_loss.edit_distance(tokens, lengths, ref, ref_len)
    al = torch_loss.ctc_token_align(x, tokens, lengths, 0, lens)
    torch.cuda.synchronize()
    logz = np.array([fp.log_normaliser(em[b, :lens[b]]).sum() for b in range(B)])
    s, q = score.cpu().numpy().astype(np.float64), logq.cpu().numpy().astype(np.float64)
    lower = q + logz[:, None]
    print(f"[ctc_sample] chain: score - (logq + log Z) min {np.min(s - lower):.3e}")
    assert np.isfinite(s).all() and (s >= lower - 1e-4 * np.abs(lower)).all()
    assert dist.shape == (B, N) and (dist.cpu().numpy() >= 0).all()
    assert al[0].shape == (B, N) and np.isfinite(al[0].cpu().numpy()).all()
    ln = lengths.cpu().numpy()
    st = al[1].cpu().numpy()
    for b in range(B):
        for k in range(N):
            assert (st[b, k, :ln[b, k]] >= 0).all() and (st[b, k, ln[b, k]:] == -1).all()
    # the sampled-risk recipe runs end to end on the device
    xg = x.clone().requires_grad_(True)
    sc = torch_loss.ctc_score(xg, tokens, lengths, 0, lens)
    err = dist.float()
    loss = ((err - err.mean(1, keepdim=True)).detach() * (sc - torch.from_numpy(logz).float().cuda()[:, None])).mean()
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(xg.grad).all() and xg.grad.abs().sum() > 0


@pytest.mark.parametrize("logq", [True, False])
@pytest.mark.parametrize("labels", [True, False])
def test_optional_outputs(gtn, logq, labels):
    B, T, C, N = 3, 70, 29, 5
    em = _noise(3, B, T, C)
    full, _ = _sample(gtn, em, frames=[T, 9, 64], blank=28, N=N, seed=77)
    got, stats = _sample(gtn, em, frames=[T, 9, 64], blank=28, N=N, seed=77, logq=logq, labels=labels)
    assert stats == (1, B) and (got[2] is None) == (not logq) and (got[3] is None) == (not labels)
    _same(f"optional logq={logq} labels={labels}", got, full)


def test_bad_arguments_raise_and_write_nothing(gtn):
    import torch
    B, T, C, N = 2, 6, 5, 4
    em = _noise(1, B, T, C)
    cases = [dict(frames=[T + 1, 1]), dict(frames=[-1, 1]), dict(blank=C), dict(rows=[3, 6], frames=[4, 6]),
             dict(N=0), dict(N=1025), dict(tau=0.0), dict(tau=float("inf")), dict(tau=float("nan")), dict(tau=-1.0)]
    c0 = gtn.debug_ctc_sample_stats()
    for kw in cases:
        with pytest.raises(ValueError):
            _sample(gtn, em, **({"N": N} | kw))
        for name, r in zip(NAMES, _sample.raw):
            assert (np.isnan(r) if name == "logq" else r == SENTINEL).all(), (kw, name)
    # row_stride < M, as raw addresses
    tok = torch.full((B, N, T), SENTINEL, dtype=torch.int32, device="cuda:0")
    ln = torch.full((B, N), SENTINEL, dtype=torch.int32, device="cuda:0")
    ems = gtn.Batch.linear(B, T, C, _dev(em), False, True)
    with pytest.raises(ValueError, match="row_stride is shorter"):
        ems.ctc_sample(tok.data_ptr(), ln, row_stride=T - 1)
    with pytest.raises(ValueError, match="rows of"):
        ems.ctc_sample(tok[:, :, :T - 1], ln)
    # not a native linear batch: there is no other route
    with pytest.raises(ValueError, match="not a native linear batch"):
        gtn.Batch([gtn.linear_graph(T, C) for _ in range(B)]).ctc_sample(tok, ln)
    # (an output on another GPU of the process is refused by check_outputs_local, shared with every device-output entry;
    #  it needs two devices and is not exercised here)
    gtn.synchronize()
    assert (tok == SENTINEL).all() and (ln == SENTINEL).all()
    assert gtn.debug_ctc_sample_stats() == c0


TORCH_CASES = [(1, 3, 70, 29, 0, True), (2, 2, 64, 300, 299, False), (3, 1, 5, 3, -1, True)]


def _torch_frames(seed, B, T):
    rng = np.random.default_rng(seed)
    fr = rng.integers(0, T + 1, B)
    fr[0] = T
    return fr.tolist()


def _torch_entry(em, blank, frames, N, seed, side_stream, return_labels=True, tau=1.0):
    import torch
    from gtn_amd import torch_loss
    x = _dev(em)
    before = x.clone()
    lens = None if frames is None else torch.tensor(frames)
    torch.cuda.synchronize()
    if side_stream:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            out = torch_loss.ctc_sample(x, blank, lens, N, tau, seed, return_labels)
        s.synchronize()
    else:
        out = torch_loss.ctc_sample(x, blank, lens, N, tau, seed, return_labels)
        torch.cuda.synchronize()
    B, T, _ = em.shape
    kinds = [(torch.int32, (B, N, T)), (torch.int32, (B, N)), (torch.float32, (B, N)), (torch.int32, (B, N, T))]
    assert len(out) == (4 if return_labels else 3)
    for o, (dt, shape) in zip(out, kinds):
        assert o.dtype == dt and tuple(o.shape) == shape and o.device == x.device and not o.requires_grad
    assert torch.equal(x, before)
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("side_stream", [True, False])
@pytest.mark.parametrize("seed,B,T,C,blank,ragged", TORCH_CASES)
def test_torch_entry(gtn, seed, B, T, C, blank, ragged, side_stream):
    frames = _torch_frames(seed, B, T) if ragged else None
    em = _noise(seed, B, T, C)
    c0, u0 = gtn.debug_ctc_sample_stats()
    out = _torch_entry(em, blank, frames, 5, 900 + seed, side_stream)
    assert gtn.debug_ctc_sample_stats() == (c0 + 1, u0 + B)
    _certify(f"torch seed={seed}", em, out, frames=frames, blank=blank, N=5, seed=900 + seed)
    three = _torch_entry(em, blank, frames, 5, 900 + seed, side_stream, return_labels=False)
    _same("without labels", three + [None], out)


def test_torch_seed_none_repeats_under_manual_seed(gtn):
    import torch
    em = _noise(4, 2, 40, 9)
    torch.manual_seed(4321)
    a = _torch_entry(em, 0, None, 4, None, False)
    b = _torch_entry(em, 0, None, 4, None, False)
    torch.manual_seed(4321)
    c = _torch_entry(em, 0, None, 4, None, False)
    _same("manual_seed", a, c)
    assert (a[3] != b[3]).mean() > 0.3
    torch.manual_seed(4321)
    want = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
    _same("the seed is the generator's draw", _torch_entry(em, 0, None, 4, want, False), a)


_CHILD = "--python-criteria-child"


def test_torch_entry_python_route(tmp_path):
    """GTN_AMD_PYTHON_CRITERIA=1 in a fresh process: Batch.linear(borrow).ctc_sample gives the native route's bytes"""
    out = str(tmp_path / "child.npz")
    env = dict(os.environ, GTN_AMD_PYTHON_CRITERIA="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), _CHILD, out], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    z = np.load(out)
    for i, (seed, B, T, C, blank, ragged) in enumerate(TORCH_CASES):
        frames = _torch_frames(seed, B, T) if ragged else None
        em = _noise(seed, B, T, C)
        got = [z[f"o{i}_{k}"] for k in range(4)]
        _certify(f"python route {i}", em, got, frames=frames, blank=blank, N=5, seed=900 + seed)
        _same(f"python route {i} == native", got, _torch_entry(em, blank, frames, 5, 900 + seed, False))
    assert int(z["calls"]) == len(TORCH_CASES) and int(z["native"]) == 0


def _python_route_child(out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gtn_amd as gtn
    from gtn_amd import torch_loss
    res = {"native": int(bool(torch_loss._native()))}
    for i, (seed, B, T, C, blank, ragged) in enumerate(TORCH_CASES):
        frames = _torch_frames(seed, B, T) if ragged else None
        for k, o in enumerate(_torch_entry(_noise(seed, B, T, C), blank, frames, 5, 900 + seed, bool(i % 2))):
            res[f"o{i}_{k}"] = o
    res["calls"] = gtn.debug_ctc_sample_stats()[0]
    np.savez(out, **res)


def test_dense_rows_c_entry(gtn):
    """gtn_ctc_sample_n of libgtn_criteria.so on dense [B][N][T] rows"""
    import torch
    B, T, C, N = 3, 66, 29, 5
    em = _noise(21, B, T, C)
    frames = np.array([T, 10, 0], np.int32)
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.gtn_ctc_sample_n.argtypes = [P, I, I, I, I, P, I, ctypes.c_uint64, ctypes.c_float, P, P, P, P]
    lib.gtn_ctc_sample_n.restype = I
    lib.gtn_criteria_last_error.restype = ctypes.c_char_p
    x = _dev(em)
    tok = torch.full((B, N, T), SENTINEL, dtype=torch.int32, device="cuda:0")
    lab = torch.full((B, N, T), SENTINEL, dtype=torch.int32, device="cuda:0")
    ln = torch.full((B, N), SENTINEL, dtype=torch.int32, device="cuda:0")
    lq = torch.full((B, N), float("nan"), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    gtn.set_stream(None)
    seed = (1 << 63) + 5
    rc = lib.gtn_ctc_sample_n(x.data_ptr(), B, T, C, 0, frames.ctypes.data, N, seed, 1.0, tok.data_ptr(), ln.data_ptr(),
                              lq.data_ptr(), lab.data_ptr())
    assert rc == 0, lib.gtn_criteria_last_error().decode()
    gtn.synchronize()
    got = [t.cpu().numpy() for t in (tok, ln, lq, lab)]
    _certify("gtn_ctc_sample_n", em, got, frames=frames.tolist(), blank=0, N=N, seed=seed)
    _same("== Batch.ctc_sample", got, _sample(gtn, em, frames=frames.tolist(), blank=0, N=N, seed=seed)[0])
    rc = lib.gtn_ctc_sample_n(x.data_ptr(), B, T, C, C, None, N, seed, 1.0, tok.data_ptr(), ln.data_ptr(), None, None)
    assert rc != 0 and "blank" in lib.gtn_criteria_last_error().decode()


def test_stats_count_calls_and_utterances(gtn):
    em = _noise(2, 4, 10, 5)
    c0, u0 = gtn.debug_ctc_sample_stats()
    _sample(gtn, em, N=1)
    _sample(gtn, em[:3], N=9)
    assert gtn.debug_ctc_sample_stats() == (c0 + 2, u0 + 7)


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == _CHILD:
    _python_route_child(sys.argv[2])
