"""Batched CTC prefix beam search with device-resident N-best output (ctc_beam.hip through gtnx_batch_ctc_beam_decode;
gtn_amd.Batch.ctc_beam_decode, gtn_amd.torch_loss.ctc_beam_decode, gtn_ctc_beam_decode_n).

The judge is the float64 yardstick of tests/ctc_beam_fp.py, which tests/test_ctc_beam_cpu.py pins to a brute-force
enumeration and to the oracle's forwardScore.  Tokens and lengths are compared with ==; that is sound because every
case here vets on the host (test_ctc_beam_cpu.py::test_every_gpu_case_vets): the three host forms agree on the compared
hypotheses and neighbouring float64 totals are at least 64 err apart.  Scores must be within 8 err of float64, err being
the case's host-side distance of the float32 forms from float64 -- computed from the host forms, never from the device.
The largest |device - float64| / err seen on an MI355X is in DESIGN section 20.

Every output has guards of sentinels that must survive: a row before and after the token rows and columns behind each
of them; the lengths and scores are dense [n][nbest] arrays (the call has no stride for them), so their guards are an
element before and after.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import ctc_beam_fp as fp

pytestmark = pytest.mark.gpu
SENTINEL = -7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tokens", "lengths", "scores")


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True, order="C")).to("cuda:0")  # (the cached cases are read-only)


def _decode(gtn, em, blank, W, K, nbest, frames=None, rows=None, pad=1, address=False, batch=None):
    """Batch.ctc_beam_decode on Batch.linear (or on `batch`) with guarded outputs (pad: guard columns, so row_stride =
    T + pad; address: raw device addresses with row_stride).  Returns ([tokens, lengths, scores] as numpy, (calls,
    utterances) counted by this call); _decode.raw keeps the arrays with their guards, also when the call raised"""
    import torch
    B, T, C = em.shape
    em_dev = _dev(em)  # (borrowed by the batch: it must outlive the call)
    ems = batch if batch is not None else gtn.Batch.linear(B, T, C, em_dev, False, True, rows)
    tok = torch.full((B + 2, nbest, T + pad), SENTINEL, dtype=torch.int32, device="cuda:0")
    ln = torch.full((B * nbest + 2,), SENTINEL, dtype=torch.int32, device="cuda:0")
    sc = torch.full((B * nbest + 2,), float("nan"), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    tv, lv, sv = tok[1:B + 1, :, :T], ln[1:B * nbest + 1].view(B, nbest), sc[1:B * nbest + 1].view(B, nbest)
    c0 = gtn.debug_ctc_beam_stats()
    try:
        if address:
            ems.ctc_beam_decode(tv.data_ptr(), lv.data_ptr(), sv.data_ptr(), frames, blank, W, K, nbest,
                                row_stride=T + pad)
        else:
            ems.ctc_beam_decode(tv, lv, sv, frames, blank, W, K, nbest)
    finally:
        gtn.synchronize()
        c1 = gtn.debug_ctc_beam_stats()
        raw = [t.cpu().numpy() for t in (tok, ln, sc)]
        _decode.raw = raw
        assert (raw[0][0] == SENTINEL).all() and (raw[0][B + 1] == SENTINEL).all(), "tokens: guard rows"
        assert (raw[0][:, :, T:] == SENTINEL).all(), "tokens: guard columns"
        assert raw[1][0] == SENTINEL and raw[1][-1] == SENTINEL, "lengths: guards"
        assert np.isnan(raw[2][0]) and np.isnan(raw[2][-1]), "scores: guards"
    out = [raw[0][1:B + 1, :, :T], raw[1][1:-1].reshape(B, nbest), raw[2][1:-1].reshape(B, nbest)]
    return out, (c1[0] - c0[0], c1[1] - c0[1])


def _untouched():
    tok, ln, sc = _decode.raw
    return (tok == SENTINEL).all() and (ln == SENTINEL).all() and np.isnan(sc).all()


def _want(case):
    """(em, the float64 outputs, err) of an entry of ctc_beam_fp's case lists"""
    kind, seed, B, T, C, blank, W, K, nbest, frames = case
    em, res = fp.results_of(case)
    tokens = np.full((B, nbest, T), -1, np.int32)
    lengths = np.zeros((B, nbest), np.int32)
    scores = np.full((B, nbest), -np.inf, np.float64)
    for b in range(B):
        for r, (toks, s) in enumerate(res["f64"][b][:nbest]):
            tokens[b, r, :len(toks)] = toks
            lengths[b, r] = len(toks)
            scores[b, r] = s
    return em, (tokens, lengths, scores), fp.case_err(res, nbest)


def _check(tag, got, want, err):
    """tokens and lengths == the float64 yardstick; scores within 8 err of it (-inf where it is -inf)"""
    for name, g, w in zip(NAMES[:2], got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (tag, name, bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
    g, w = got[2], want[2]
    assert g.dtype == np.float32 and g.shape == w.shape and not np.isnan(g).any(), tag
    dead = np.isneginf(w)
    assert (np.isneginf(g) == dead).all(), (tag, g, w)
    dist = float(np.abs(g[~dead].astype(np.float64) - w[~dead]).max()) if (~dead).any() else 0.0
    print(f"[ctc_beam] {tag}: |device - float64| {dist:.3g}, err {err:.3g}, ratio {dist / err if err else 0:.3g}")
    assert dist <= fp.SCORE_FACTOR * err, (tag, dist, err)


def _run_case(gtn, case, **kw):
    kind, seed, B, T, C, blank, W, K, nbest, frames = case
    em, want, err = _want(case)
    got, stats = _decode(gtn, em, blank, W, K, nbest, frames=None if frames is None else list(frames), **kw)
    assert stats == (1, B)
    _check(str(case[:9]), got, want, err)
    return got


@pytest.mark.parametrize("case", fp.SHAPE_CASES + [fp.REPEAT_CASE],
                         ids=lambda c: "B{2}-T{3}-C{4}-blank{5}-W{6}-K{7}-n{8}".format(*c))
def test_search_matches_the_yardstick(gtn, case):
    """every C of the row kernel's head, tail and lanes-per-row variants, C <= K, T around the 64s, B = 1, 2, 65,
    W = 1 .. 64, K = 1 .. 32, nbest = 1, 2, 4 and nbest = W at T <= 3"""
    _run_case(gtn, case)


@pytest.mark.parametrize("case", fp.RECREATED_CASES, ids=lambda c: "B{2}-T{3}-C{4}-W{6}-K{7}-seed{1}".format(*c))
def test_a_prefix_that_comes_back_is_still_its_childs_parent(gtn, case):
    """a prefix leaves the list while its child stays and is created again from its own parent: the child's extension
    is still merged, the list holds no tokens twice (test_ctc_beam_cpu.py shows that identity by node number gets these
    cases wrong)"""
    got = _run_case(gtn, case)
    for b in range(case[2]):
        rows = [tuple(got[0][b, r, :got[1][b, r]]) for r in range(case[8]) if np.isfinite(got[2][b, r])]
        assert len(set(rows)) == len(rows), b


def test_exact_ties(gtn):
    """integer-valued rows at T = 1, where every score is an entry of its row and so exact: the top-K ties go to the
    smaller label, and equal totals are ordered stay first, then by label -- tokens, lengths AND scores with =="""
    for C, K, W, blank in ((29, 3, 8, 0), (65, 32, 64, 64), (300, 16, 16, 7), (3, 3, 4, 1)):
        em = fp.integer_case(C, 65, 1, C)
        nbest = min(W, 4)
        want = fp.decode_batch(em, None, blank, W, K, nbest, "f32")
        got, _ = _decode(gtn, em, blank, W, K, nbest)
        for name, g, w in zip(NAMES, got, want):
            assert g.tobytes() == w.tobytes(), (C, name)


@pytest.mark.parametrize("mode", ["frames", "rows", "both"])
def test_mixed_frame_counts(gtn, mode):
    """per-utterance lengths (T, T - 1, 1 and 0 among them) through `frames`, through Batch.linear(rows=) and through
    both: the yardstick at each length; NaN in every pad row changes no bit of any output; each utterance equals the
    call on em[b, :T_b] alone, bit for bit"""
    case = fp.RAGGED_ROWS_CASE if mode == "rows" else fp.RAGGED_CASE
    kind, seed, B, T, C, blank, W, K, nbest, fr = case
    em, want, err = _want(case)
    rows = None if mode == "frames" else [max(f, 1) for f in fr] if mode == "both" else list(fr)
    frames = None if mode == "rows" else list(fr)
    got, stats = _decode(gtn, em, blank, W, K, nbest, frames, rows)
    assert stats == (1, B)
    _check(f"ragged {mode}", got, want, err)
    raw = _decode.raw
    poisoned = em.copy()
    for b in range(B):
        poisoned[b, fr[b]:] = np.nan
    _decode(gtn, poisoned, blank, W, K, nbest, frames, rows)
    for name, r0, r1 in zip(NAMES, raw, _decode.raw):
        assert r0.tobytes() == r1.tobytes(), name
    if mode == "frames":
        for b in range(B):
            if fr[b] == 0:
                assert (got[0][b] == -1).all() and (got[1][b] == 0).all() and np.isneginf(got[2][b]).all()
                continue
            alone, _ = _decode(gtn, em[b:b + 1, :fr[b]], blank, W, K, nbest)
            assert (got[0][b, :, :fr[b]] == alone[0][0]).all() and (got[0][b, :, fr[b]:] == -1).all(), b
            assert got[1][b].tobytes() == alone[1][0].tobytes() and got[2][b].tobytes() == alone[2][0].tobytes(), b


def test_full_length_frames_equal_no_frames(gtn):
    kind, seed, B, T, C, blank, W, K, nbest, _ = fp.REPEAT_CASE
    em = _want(fp.REPEAT_CASE)[0]
    _decode(gtn, em, blank, W, K, nbest)
    raw = _decode.raw
    _decode(gtn, em, blank, W, K, nbest, frames=[T] * B)
    for name, r0, r1 in zip(NAMES, raw, _decode.raw):
        assert r0.tobytes() == r1.tobytes(), name


def test_holes_and_a_dead_utterance(gtn):
    """-inf and NaN entries inside the rows that count are never chosen; utterance 1 has an all--inf row inside T_b:
    rows of -1, length 0, score -inf, and its neighbours are what they are without it"""
    kind, seed, B, T, C, blank, W, K, nbest, _ = fp.HOLES_CASE
    em, want, err = _want(fp.HOLES_CASE)
    assert np.isneginf(em[1, T // 2]).all() and np.isnan(em).any() and np.isneginf(want[2][1]).all()
    assert np.isfinite(want[2][[0, 2, 3]]).all()
    got = _run_case(gtn, fp.HOLES_CASE)
    assert (got[0][1] == -1).all() and (got[1][1] == 0).all() and np.isneginf(got[2][1]).all()
    healed = em.copy()
    healed[1, T // 2] = 0.0
    other, _ = _decode(gtn, healed, blank, W, K, nbest)
    for g, o in zip(got, other):
        assert g[[0, 2, 3]].tobytes() == o[[0, 2, 3]].tobytes()
    assert np.isfinite(other[2][1]).all()


def test_fewer_hypotheses_than_nbest(gtn):
    """one frame over two labels has two prefixes: the other slots are -1, 0, -inf"""
    em = fp.continuous_case(7, 3, 1, 2)
    want = fp.decode_batch(em, None, 0, 8, 2, 4, "f32")
    got, _ = _decode(gtn, em, 0, 8, 2, 4)
    for name, g, w in zip(NAMES, got, want):
        assert g.tobytes() == w.tobytes(), name  # (one frame: the scores are entries of the row)
    assert np.isneginf(got[2][:, 2:]).all() and (got[1][:, 2:] == 0).all() and (got[0][:, 2:] == -1).all()


def test_repeatable(gtn):
    """two calls on the same input: every output bit for bit"""
    for case in (fp.SHAPE_CASES[9], fp.SHAPE_CASES[10], fp.RAGGED_CASE):
        kind, seed, B, T, C, blank, W, K, nbest, fr = case
        em = _want(case)[0]
        frames = None if fr is None else list(fr)
        _decode(gtn, em, blank, W, K, nbest, frames)
        raw = _decode.raw
        _decode(gtn, em, blank, W, K, nbest, frames)
        for name, r0, r1 in zip(NAMES, raw, _decode.raw):
            assert r0.tobytes() == r1.tobytes(), (case, name)


@pytest.mark.parametrize("address", [False, True])
def test_row_stride_above_T(gtn, address):
    """rows 5 entries wider than T, as tensor views and as raw device addresses with row_stride"""
    _run_case(gtn, fp.REPEAT_CASE, pad=5, address=address)


@pytest.mark.parametrize("case", fp.UNPRUNED_CASES, ids=lambda c: "T{3}-C{4}-blank{5}".format(*c))
def test_unpruned_scores_are_the_loss_on_the_device(gtn, case):
    """T <= 3, C <= 4, W = 64, K = C, log-softmax input: nothing is pruned, so every returned hypothesis has
    score = -ctc_loss(log_probs, [y]), within the 1e-4 max(1, |score|) the suite uses for losses"""
    import torch
    from gtn_amd import torch_loss
    kind, seed, B, T, C, blank, W, K, nbest, _ = case
    assert T <= 3 and C <= 4 and W == 64 and K == C
    got = _run_case(gtn, case)
    x = _dev(_want(case)[0])
    try:
        for r in range(nbest):
            keep = [b for b in range(B) if np.isfinite(got[2][b, r])]
            assert keep, r
            targets = [got[0][b, r, :got[1][b, r]].tolist() for b in keep]
            loss = torch_loss.ctc_loss(x[keep], targets, blank=blank)
            torch.cuda.synchronize()
            for b, l in zip(keep, loss.cpu().numpy()):
                s = float(got[2][b, r])
                print(f"[ctc_beam] unpruned b={b} r={r} y={targets[keep.index(b)]} score {s!r} -loss {-float(l)!r}")
                assert abs(s + float(l)) <= 1e-4 * max(1.0, abs(s)), (b, r, s, float(l))
    finally:
        gtn.set_stream(None)


def test_bad_arguments_raise_before_anything_is_written(gtn):
    """a count outside 0 .. M or above the rows the batch carries, a stride below M, a blank that is no label, a batch
    that is not a native linear one: ValueError, outputs untouched"""
    B, T, C = 3, 9, 8
    em = fp.continuous_case(83, B, T, C)
    for kw, msg in ((dict(frames=[9, 10, 1]), "outside 0 .. M"), (dict(frames=[-1, 2, 3]), "outside 0 .. M"),
                    (dict(frames=[9, 5, 1], rows=[9, 4, 9]), "beyond the rows"), (dict(blank=8), "blank"),
                    (dict(address=True, pad=-1), "row_stride is shorter")):
        with pytest.raises(ValueError, match=msg):
            _decode(gtn, em, kw.pop("blank", 0), 4, 4, 2, **kw)
        if kw.get("pad") != -1:  # (those arrays have no guard column to look at)
            assert _untouched()
    import torch
    em_dev = _dev(em)
    ems = gtn.Batch.linear(B, T, C, em_dev, False, True)
    wide = torch.full((B, 2, T + 3), SENTINEL, dtype=torch.int32, device="cuda:0")
    ln = torch.full((B, 2), SENTINEL, dtype=torch.int32, device="cuda:0")
    sc = torch.full((B, 2), float("nan"), dtype=torch.float32, device="cuda:0")
    with pytest.raises(ValueError, match="rows of 8 entries, the batch has 9"):  # (a view narrower than M, stride >= M)
        ems.ctc_beam_decode(wide[:, :, :T - 1], ln, sc, None, 0, 4, 4, 2)
    with pytest.raises(ValueError, match="tokens_out must be an int32"):
        ems.ctc_beam_decode(wide.float(), ln, sc, None, 0, 4, 4, 2)
    with pytest.raises(ValueError, match="scores_out must be a float32"):
        ems.ctc_beam_decode(wide[:, :, :T], ln, ln.clone(), None, 0, 4, 4, 2)
    gtn.synchronize()
    assert (wide == SENTINEL).all() and (ln == SENTINEL).all() and sc.isnan().all()
    graphs = gtn.linear_graph_n(B, T, C, _dev(em), False)
    with pytest.raises(ValueError, match="not a native linear batch"):
        _decode(gtn, em, 0, 4, 4, 2, batch=gtn.Batch(graphs))
    assert _untouched()
    assert gtn.debug_ctc_beam_stats() == gtn.debug_ctc_beam_stats()


def _torch_entry(gtn, case, side_stream):
    import torch
    from gtn_amd import torch_loss
    kind, seed, B, T, C, blank, W, K, nbest, frames = case
    x = _dev(_want(case)[0]).requires_grad_(True)
    before = x.detach().clone()
    torch.cuda.synchronize()
    kw = dict(blank=blank, input_lengths=None if frames is None else list(frames), beam_size=W, cutoff_top_n=K,
              nbest=nbest)
    try:
        if side_stream:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                out = torch_loss.ctc_beam_decode(x, **kw)
            torch.cuda.current_stream().wait_stream(s)
        else:
            out = torch_loss.ctc_beam_decode(x, **kw)
        torch.cuda.synchronize()
    finally:
        gtn.set_stream(None)
    assert len(out) == 3
    kinds = ((torch.int32, (B, nbest, T)), (torch.int32, (B, nbest)), (torch.float32, (B, nbest)))
    for o, (dt, shape) in zip(out, kinds):
        assert o.dtype == dt and o.shape == shape and o.device == x.device and not o.requires_grad
    assert torch.equal(x.detach(), before)
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("side_stream", [True, False])
@pytest.mark.parametrize("case", fp.TORCH_CASES, ids=lambda c: "B{2}-T{3}-C{4}".format(*c))
def test_torch_entry(gtn, case, side_stream):
    """torch_loss.ctc_beam_decode (native route) on a non-default stream and on the default one, with and without
    input_lengths: dtypes, device, shapes; the yardstick; log_probs untouched, nothing requires grad; counted"""
    _, want, err = _want(case)
    c0 = gtn.debug_ctc_beam_stats()
    out = _torch_entry(gtn, case, side_stream)
    c1 = gtn.debug_ctc_beam_stats()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, case[2])
    _check(f"torch {case[:9]}", out, want, err)


_CHILD = "--python-criteria-child"


def test_torch_entry_python_route(tmp_path):
    """GTN_AMD_PYTHON_CRITERIA=1 in a fresh process: Batch.linear(borrow).ctc_beam_decode"""
    out = str(tmp_path / "child.npz")
    env = dict(os.environ, GTN_AMD_PYTHON_CRITERIA="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), _CHILD, out], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    z = np.load(out)
    i = 0
    for case in fp.TORCH_CASES:
        _, want, err = _want(case)
        for side_stream in (True, False):
            _check(f"python route {i}", [z[f"o{i}_{k}"] for k in range(3)], want, err)
            i += 1
    assert int(z["calls"]) == 2 * len(fp.TORCH_CASES) and int(z["utterances"]) == sum(2 * c[2] for c in fp.TORCH_CASES)


def _python_route_child(out):
    sys.path.insert(0, ROOT)
    import gtn_amd as gtn
    from gtn_amd import torch_loss
    assert not torch_loss._native()
    res, i = {}, 0
    for case in fp.TORCH_CASES:
        for side_stream in (True, False):
            for k, o in enumerate(_torch_entry(gtn, case, side_stream)):
                res[f"o{i}_{k}"] = o
            i += 1
    res["calls"], res["utterances"] = gtn.debug_ctc_beam_stats()
    np.savez(out, **res)


def test_criteria_abi(gtn):
    """gtn_ctc_beam_decode_n gives the three tensors the Batch API gives"""
    import torch
    case = fp.TORCH_CASES[1]
    kind, seed, B, T, C, blank, W, K, nbest, frames = case
    em, want, err = _want(case)
    em_dev = _dev(em)
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    lib.gtn_ctc_beam_decode_n.argtypes = ([ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] + [ctypes.c_int] * 3
                                          + [ctypes.c_void_p] * 3)
    lib.gtn_ctc_beam_decode_n.restype = ctypes.c_int
    lib.gtn_criteria_last_error.restype = ctypes.c_char_p
    fr = np.ascontiguousarray(frames, dtype=np.int32)
    tok = torch.full((B, nbest, T), SENTINEL, dtype=torch.int32, device="cuda:0")
    le = torch.full((B, nbest), SENTINEL, dtype=torch.int32, device="cuda:0")
    sc = torch.full((B, nbest), float("nan"), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rc = lib.gtn_ctc_beam_decode_n(em_dev.data_ptr(), B, T, C, blank, fr.ctypes.data, W, K, nbest, tok.data_ptr(),
                                   le.data_ptr(), sc.data_ptr())
    assert rc == 0, lib.gtn_criteria_last_error().decode()
    gtn.synchronize()
    _check("abi", [t.cpu().numpy() for t in (tok, le, sc)], want, err)
    rc = lib.gtn_ctc_beam_decode_n(em_dev.data_ptr(), B, T, C, C, fr.ctypes.data, W, K, nbest, tok.data_ptr(),
                                   le.data_ptr(), sc.data_ptr())
    assert rc == -1 and "blank" in lib.gtn_criteria_last_error().decode()


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == _CHILD:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _python_route_child(sys.argv[2])
