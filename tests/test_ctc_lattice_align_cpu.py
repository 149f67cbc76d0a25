"""CTC Viterbi alignment of token lattices, the parts that need no GPU.  The float32 transcription of
tests/ctc_lattice_align_fp.py (which test_ctc_lattice_align_gpu.py compares the kernel with bit for bit) is pinned to an
enumeration of the lattice's paths, to the oracle's viterbi score of the alignment graph built arc by arc, and to
ctc_token_align_fp on chains; the path and the spans it returns are scored on their own in float64 and measured against
the float64 optimum; the no-path and truncation rules are those of the contract; and the entry points
exist in every layer, refuse bad arguments before they ask for a device, and fail loudly without one."""
import ctypes
import os

import numpy as np
import pytest

import ctc_beam_fp as bfp
import ctc_lattice_align_fp as fp
import ctc_lattice_fp as lfp
import ctc_token_align_fp as tfp
from conftest import ROOT, has_gpu
from oracle_lib import OGraph, lib as oracle

NEG = -np.inf
GATE = fp.SCORE_GATE

# small continuous cases: the lattices of the tie cases under emissions without ties
CONT = [(li, kind, seed, T) for li in range(len(fp.TIE_LATTICES))
        for kind, seed, T in (("continuous", 1, 3), ("continuous", 2, 7), ("holes", 3, 6))]


def cont_case(li, kind, seed, T):
    name, arcs, K, weights = fp.TIE_LATTICES[li]
    make = {"continuous": bfp.continuous_case, "holes": bfp.holes_case}[kind]
    em = make(300 + 17 * li + seed, 1, T, fp.TIE_C)[0]
    rng = np.random.default_rng(li + seed)
    w = None if weights is None else np.where(np.isfinite(weights), rng.normal(0, 1, len(arcs)), NEG).astype(np.float32)
    a, w = fp.sort_by_dst(arcs, w)
    return name, em, T, a, K, w


def lattice(arcs, K, w, C=fp.TIE_C):
    return fp.lattice_of(arcs, len(arcs), K, w, C, 4096)


def chain_best64(em, y, blank):
    """the best alignment score of the chain y in float64: the 2 U + 1 states of ctcGraph, written out on its own"""
    x = np.asarray(em, dtype=np.float64)
    T, U = x.shape[0], len(y)
    labs = [blank] * (2 * U + 1)
    labs[1::2] = list(y)
    v = np.full(2 * U + 1, NEG)
    v[0] = 0.0
    for t in range(T):
        nv = np.full(2 * U + 1, NEG)
        for s in range(2 * U + 1):
            c = [v[s]] + ([v[s - 1]] if s >= 1 else []) + ([v[s - 2]] if s % 2 and s >= 3 and labs[s] != labs[s - 2] else [])
            m = max(c)
            nv[s] = m + x[t, labs[s]] if m > NEG else NEG
        v = np.where(np.isnan(nv), NEG, nv)
    return float(max(v[-1], v[-2])) if U else float(v[0])


def by_enumeration(em, lat, blank):
    src, dst, lab, w, K = lat
    best = NEG
    for p in fp.paths_of(src, dst, K):
        z = chain_best64(em, lab[p], blank)
        wp = float(np.sum(w[p]))
        if np.isfinite(z) and wp > NEG:
            best = max(best, wp + z)
    return best


def oracle_viterbi(em, lat, blank):
    """viterbiScore of the lattice's CTC alignment graph, built arc by arc, intersected with
    linearGraph(T, C) (float32); an arc of weight -inf is left out"""
    src, dst, lab, w, K = lat
    L = oracle()
    g = OGraph()
    A = len(src)
    for n in range(K):
        L.og_add_node(g.h, int(n == 0), int(n == K - 1))
    for a in range(A):
        L.og_add_node(g.h, 0, int(dst[a] == K - 1))
    for n in range(K):
        L.og_add_arc(g.h, n, n, blank, blank, 0.0)
    for a in range(A):
        if not np.isfinite(w[a]):
            continue
        s, l, wa = K + a, int(lab[a]), float(w[a])
        L.og_add_arc(g.h, s, s, l, l, 0.0)
        L.og_add_arc(g.h, int(src[a]), s, l, l, wa)
        L.og_add_arc(g.h, s, int(dst[a]), blank, blank, 0.0)
        for a2 in range(A):
            if dst[a2] == src[a] and lab[a2] != lab[a] and np.isfinite(w[a2]):
                L.og_add_arc(g.h, K + a2, s, l, l, wa)
    T, C = em.shape
    return g.compose(OGraph.linear(T, C, em), "intersect").shortest_distance(tropical=True)


def check_returned(em, lat, blank, r, opt64):
    """the path and the spans of Out r, scored on their own, against the float64 optimum and r's own score"""
    n = int(r.path_len)
    assert n <= len(r.path_arcs)
    z = fp.rescore64(em, lat, r.path_arcs[:n], r.starts[:n], r.ends[:n], blank)
    tol = GATE * max(1.0, abs(opt64))
    assert abs(z - opt64) <= tol and abs(z - float(r.score)) <= tol, (z, opt64, float(r.score))
    assert (r.path_tokens[:n] == lat[2][r.path_arcs[:n]]).all()
    T = em.shape[0]
    want = np.full(T, -1)
    for i in range(n):
        want[r.starts[i]:r.ends[i]] = r.path_arcs[i]
    assert (r.frame_arcs[:T] == want).all() and (r.frame_arcs[T:] == -1).all()
    return z


# ---- the transcription against enumeration, the oracle and its own returned path ----
def test_tie_cases_cover_what_they_name():
    cases = fp.tie_cases()
    Ks = {c[4] for c in cases}
    Ts = {c[2] for c in cases}
    assert Ks == {1, 2, 3, 4, 5, 6} and min(Ts) == 1 and max(Ts) == 9
    names = " ".join(l[0] for l in fp.TIE_LATTICES)
    for what in ("parallel arcs of equal", "parallel arcs of different", "consecutive equal", "equal to blank", "dead end",
                 "-inf weight"):
        assert what in names
    assert any(c[5] is not None and np.isneginf(c[5]).any() for c in cases)
    # ties are real: under the all-zero emissions every alignment of every path without weights scores 0
    r = fp.tie_result()
    zero = [b for b, c in enumerate(cases) if "zero" in c[0] and "no weights" in c[0] and np.isfinite(r.scores[b])]
    assert len(zero) >= 20 and (r.scores[zero] == 0).all()


def test_the_transcription_is_the_enumeration_and_the_oracle_on_ties():
    cases, r = fp.tie_cases(), fp.tie_result()
    finite = 0
    for b, (name, em, T, arcs, K, w) in enumerate(cases):
        lat = lattice(arcs, K, w)
        x = em[:T]
        want = by_enumeration(x, lat, fp.TIE_BLANK)
        got = float(r.scores[b])
        assert got == want, (name, got, want)  # (every sum is exact)
        orc = oracle_viterbi(x, lat, fp.TIE_BLANK)
        if np.isfinite(want):
            finite += 1
            assert orc is not None and np.float32(orc) == np.float32(got), (name, got, orc)
            out = fp.Out(*(f[b] for f in r))
            assert check_returned(x, lat, fp.TIE_BLANK, out, want) == want, name
        else:
            assert orc is None or not np.isfinite(orc) or orc < -1e29, (name, orc)
            assert r.path_len[b] == 0 and (r.path_arcs[b] == -1).all() and (r.frame_arcs[b] == -1).all()
    assert finite >= len(cases) // 2


@pytest.mark.parametrize("li,kind,seed,T", CONT)
def test_the_transcription_is_the_enumeration_and_the_oracle_on_continuous_inputs(li, kind, seed, T):
    name, em, T, arcs, K, w = cont_case(li, kind, seed, T)
    lat = lattice(arcs, K, w)
    want = by_enumeration(em, lat, fp.TIE_BLANK)
    r64 = fp.align_lattice(em, lat, fp.TIE_BLANK, T, 8, np.float64)
    r32 = fp.align_lattice(em, lat, fp.TIE_BLANK, T, 8)
    orc = oracle_viterbi(em, lat, fp.TIE_BLANK)
    if np.isfinite(want):
        assert abs(float(r64.score) - want) <= 1e-9, (name, r64.score, want)
        tol = GATE * max(1.0, abs(want))
        assert abs(float(r32.score) - want) <= tol and abs(orc - want) <= tol, (name, r32.score, orc, want)
        check_returned(em, lat, fp.TIE_BLANK, r64, want)
        check_returned(em, lat, fp.TIE_BLANK, r32, want)
        assert r32.score.dtype == np.float32 and r32.token_scores.dtype == np.float32
    else:
        assert np.isneginf(r64.score) and np.isneginf(r32.score) and r32.path_len == 0


@pytest.mark.parametrize("name", fp.ALL_GPU_CASES)
def test_returned_paths_of_the_named_cases_and_the_order_of_max_and_sum(name):
    """rescore64 of what the float32 transcription returns against the float64 optimum, on every utterance of every case
    the GPU file runs; and the max is below the log-sum"""
    c, r, r64 = fp.case(name), fp.result(name), fp.result64(name)
    sums = lfp.result(name, False).scores
    B, M, C = c.em.shape
    assert np.isfinite(r.scores).any()
    assert (np.isfinite(r.scores) == np.isfinite(sums)).all()  # a path exactly where ctc_lattice_score is above -inf
    worst = 0.0
    for b in range(B):
        out, opt = fp.Out(*(f[b] for f in r)), float(r64.scores[b])
        if not np.isfinite(opt):
            assert np.isneginf(out.score) and out.path_len == 0
            continue
        assert opt <= sums[b] + 1e-9 * max(1.0, abs(sums[b])), (name, b, opt, sums[b])
        T = M if c.frames is None else int(c.frames[b])
        lat = fp.lattice_of(c.arcs[b], c.num_arcs[b], c.num_nodes[b], None if c.weights is None else c.weights[b], C,
                            c.max_states)
        assert out.path_len <= len(out.path_arcs)  # (the default width holds every path)
        z = check_returned(c.em[b, :T], lat, c.blank, out, opt)
        worst = max(worst, abs(z - opt) / max(1.0, abs(opt)))
    print(name, "rescored path against the float64 optimum, relative:", worst)


# ---- chains ----
@pytest.mark.parametrize("kind", ["continuous", "integer"])
def test_a_chain_lattice_has_the_bits_of_ctc_token_align(kind):
    rng = np.random.default_rng(5)
    C, blank, T = 6, 0, 14
    for trial in range(24):
        n = int(rng.integers(0, 9))
        y = rng.integers(0 if trial % 3 == 0 else 1, C, n)  # (every third with tokens equal to blank)
        em = (tfp.continuous(trial, 1, T, C) if kind == "continuous" else tfp.integer(trial, 1, T, C, -2, 1))[0]
        arcs, K = fp.chain_lattice(y)
        lat = fp.lattice_of(arcs.reshape(-1, 3), n, K, None, C, 4096)
        got = fp.align_lattice(em, lat, blank, T, max(n, 1))
        want = tfp.align_pair(em, y.astype(np.int32) if n else np.zeros(1, np.int32), n, blank, T, max(n, 1))
        assert np.float32(got.score).tobytes() == np.float32(want.score).tobytes(), (kind, trial, got.score, want.score)
        if np.isfinite(want.score):
            assert got.path_len == n and (got.path_arcs[:n] == np.arange(n)).all() and (got.path_tokens[:n] == y).all()
            if kind == "continuous" and (y != blank).all():  # (a token equal to blank ties with the blank beside it)
                assert (got.starts[:n] == want.starts[:n]).all() and (got.ends[:n] == want.ends[:n]).all()
                assert got.token_scores[:n].tobytes() == want.token_scores[:n].tobytes()
                assert (got.frame_arcs == want.frame_tokens).all()
        else:
            assert got.path_len == 0


# ---- no path, the empty path, truncation ----
def test_no_path_exactly_where_the_contract_says():
    c, r = fp.case("edges"), fp.result("edges")
    fin = np.isfinite(r.scores)
    want = [n.startswith("valid") or n in ("num_arcs above the width", "negative num_arcs") for n in fp.EDGES]
    assert fin.tolist() == want, list(zip(fp.EDGES, r.scores))
    for b in np.nonzero(~fin)[0]:
        assert np.isneginf(r.scores[b]) and r.path_len[b] == 0
        for rows in (r.path_arcs, r.path_tokens, r.starts, r.ends, r.frame_arcs):
            assert (rows[b] == -1).all()
        assert np.isneginf(r.token_scores[b]).all()
    # a one-node lattice (a negative count is no arc): the empty path, the blank emissions summed in frame order
    s = c.em[14, 0, c.blank]
    for t in range(1, c.em.shape[1]):
        s = np.float32(s + c.em[14, t, c.blank])
    assert r.scores[14] == s and r.path_len[14] == 0 and (r.path_arcs[14] == -1).all() and (r.frame_arcs[14] == -1).all()
    # the forbidden arc and the dead end are on no path
    n = r.path_len[10]
    assert n > 0 and not set(r.path_arcs[10, :n].tolist()) & {0, 2, 3, 5}
    g, rg = fp.case("ragged"), fp.result("ragged")
    assert fp.RAGGED_FRAMES[2] == 0 and np.isneginf(rg.scores[2]) and rg.path_len[2] == 0  # T_b == 0
    lat = fp.lattice_of(g.arcs[6], g.num_arcs[6], g.num_nodes[6], None, 5, g.max_states)
    assert fp.min_frames(*lat[:3], lat[4]) == fp.RAGGED_FRAMES[6] + 1  # one frame fewer than the shortest path
    assert np.isneginf(rg.scores[6]) and rg.path_len[6] == 0 and (rg.starts[6] == -1).all()
    for b, f in enumerate(fp.RAGGED_FRAMES):
        assert (rg.frame_arcs[b, f:] == -1).all()
    assert np.isfinite(rg.scores[[0, 1, 3, 4, 5]]).all() and (rg.path_len[[0, 1, 3, 4, 5]] > 0).all()


def test_a_path_longer_than_the_rows_keeps_its_length_and_writes_its_head():
    c = fp.case("indeg8-c37")
    full = fp.evaluate(c)
    n = int(full.path_len.max())
    assert n >= 3
    for P in (1, 2, n - 1):
        cut = fp.evaluate(c, P=P)
        assert (cut.path_len == full.path_len).all() and cut.scores.tobytes() == full.scores.tobytes()
        for a, b in zip(cut[2:7], full[2:7]):
            assert a.shape[1] == P and a.tobytes() == np.ascontiguousarray(b[:, :P]).tobytes()
        assert (cut.frame_arcs == full.frame_arcs).all()


# ---- the entry points ----
def test_entry_points_exist(gtn):
    from gtn_amd import torch_loss
    assert callable(torch_loss.ctc_lattice_align)
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    assert hasattr(lib, "gtn_ctc_lattice_align_n")
    eng = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_amd.so"))
    for name in ("gtnx_batch_ctc_lattice_align", "gtnx_batch_ctc_lattice_align_stats"):
        assert hasattr(eng, name), name
    assert callable(gtn.Batch.ctc_lattice_align)
    calls, utts = gtn.debug_ctc_lattice_align_stats()
    assert calls >= 0 and utts >= 0
    for header, name in (("include/gtn_amd.h", "gtnx_batch_ctc_lattice_align_stats"),
                         ("include/gtn_amd.h", "gtnx_batch_ctc_lattice_align("),
                         ("include/gtn/batch.h", "ctcLatticeAlign"),
                         ("gtn_amd/criteria/ctc_criterion.h", "ctcLatticeAlignBatch"),
                         ("gtn_amd/criteria/criteria_capi.cpp", "gtn_ctc_lattice_align_n"),
                         ("gtn_amd/csrc/kernels.h", "CtcLatticeAlignArgs"), ("gtn_amd/csrc/kernels.h", "launch_ctc_lattice_align"),
                         ("gtn_amd/csrc/batch.h", "batch_ctc_lattice_align_stats"),
                         ("gtn_amd/csrc/ctc_lattice_align.hip", "ctc_lattice_align_kernel")):
        with open(os.path.join(ROOT, header)) as f:
            assert name in f.read(), header


def test_argument_errors_come_before_the_device(gtn):
    """what the arguments alone decide is GTNX_INVALID_ARGUMENT (1) with or without a device"""
    import gtn_amd
    lib = gtn_amd._lib
    batch = gtn.Batch([gtn.linear_graph(2, 8)])
    p = ctypes.c_void_p
    call = lib.gtnx_batch_ctc_lattice_align
    #        0 ems    1 frames 2 blank 3 arcs 4 stride 5 num_arcs 6 num_nodes 7 weights 8 A 9 max_states
    good = [batch._h, None, 0, p(64), 12, p(64), p(64), None, 4, 8,
            # 10 scores 11 path_len 12 path_arcs 13 path_tokens 14 starts 15 ends 16 token_scores 17 P 18 out_stride
            p(64), p(64), p(64), p(64), p(64), p(64), None, 4, 4,
            # 19 frame_arcs 20 frame_stride
            None, 0]
    before = gtn.debug_ctc_lattice_align_stats()

    def bad(i, v):
        a = list(good)
        a[i] = v
        return a
    # the refusals of gtnx_batch_ctc_lattice_score ...
    refused = [bad(0, None), bad(3, None), bad(5, None), bad(6, None), bad(8, -1), bad(4, 11), bad(4, -1), bad(2, -1),
               bad(9, 0), bad(9, 4097), bad(9, -5)]
    # ... a null output, P < 1, out_stride < P
    refused += [bad(i, None) for i in range(10, 16)] + [bad(17, 0), bad(17, -3), bad(18, 3), bad(18, -1)]
    for a in refused:
        assert call(*a) == 1, a
    assert gtn.debug_ctc_lattice_align_stats() == before  # (nothing launched)
    with pytest.raises(ValueError, match="max_states outside"):
        batch.ctc_lattice_align(64, 64, 64, 64, 64, 64, 64, 64, 64, A=4, row_stride=12, max_states=0, P=4)
    with pytest.raises(ValueError, match="needs A and row_stride"):
        batch.ctc_lattice_align(64, 64, 64, 64, 64, 64, 64, 64, 64, P=4)
    with pytest.raises(ValueError, match="need P"):
        batch.ctc_lattice_align(64, 64, 64, 64, 64, 64, 64, 64, 64, A=4, row_stride=12)
    with pytest.raises(ValueError, match="P below 1"):
        batch.ctc_lattice_align(64, 64, 64, 64, 64, 64, 64, 64, 64, A=4, row_stride=12, max_states=8, P=0)
    with pytest.raises(ValueError, match="shorter than the rows' width P"):
        batch.ctc_lattice_align(64, 64, 64, 64, 64, 64, 64, 64, 64, A=4, row_stride=12, max_states=8, P=4, out_stride=3)
    with pytest.raises(ValueError, match="null output pointer"):
        batch.ctc_lattice_align(64, 64, 64, 64, 0, 64, 64, 64, 64, A=4, row_stride=12, max_states=8, P=4)


def test_a_batch_without_an_utterance_needs_no_device(gtn):
    import gtn_amd
    lib = gtn_amd._lib
    p = ctypes.c_void_p
    empty = gtn.Batch([])
    if empty._h:  # (a batch without elements may have no handle to give: then there is nothing to call with)
        before = gtn.debug_ctc_lattice_align_stats()
        assert lib.gtnx_batch_ctc_lattice_align(empty._h, None, 0, p(64), 12, p(64), p(64), None, 4, 8, p(64), p(64),
                                                p(64), p(64), p(64), p(64), None, 4, 4, None, 0) == 0
        assert gtn.debug_ctc_lattice_align_stats() == before


def test_torch_argument_checks():
    import torch
    from gtn_amd import torch_loss
    em = torch.zeros(2, 3, 8)
    arcs = torch.zeros(2, 4, 3, dtype=torch.int32)
    na = torch.zeros(2, dtype=torch.int32)
    nn_ = torch.ones(2, dtype=torch.int32)
    w = torch.zeros(2, 4)
    for args, kw, msg in (((em.double(), arcs, na, nn_), {}, "float32 tensor"), ((em[0], arcs, na, nn_), {}, "float32 tensor"),
                          ((em, arcs.long(), na, nn_), {}, "arcs must be an int32"),
                          ((em, arcs[:1], na, nn_), {}, "arcs must be an int32"),
                          ((em, arcs[:, :, :2], na, nn_), {}, "arcs must be an int32"),
                          ((em, arcs, na.float(), nn_), {}, "num_arcs must be an int32 or int64"),
                          ((em, arcs, na, nn_[:1]), {}, "num_nodes must be an int32 or int64"),
                          ((em, arcs, na, nn_, w[:, :3]), {}, "arc_weights must be a floating-point"),
                          ((em, arcs, na, nn_, w.long()), {}, "arc_weights must be a floating-point"),
                          ((em, arcs, na, nn_), dict(blank=8), "blank must be one of"),
                          ((em, arcs, na, nn_), dict(blank=-1), "blank must be one of"),
                          ((em, arcs, na, nn_), dict(max_states=0), "max_states outside 1 .. 4096"),
                          ((em, arcs, na, nn_), dict(max_states=4097), "max_states outside 1 .. 4096"),
                          ((em, arcs, na, nn_), dict(input_lengths=[4, 1]), "input length outside 0 .. 3"),
                          ((em, arcs, na, nn_), dict(input_lengths=[1]), "input lengths for a batch of 2"),
                          ((em, arcs, na, nn_), dict(max_path=0), "max_path must be at least 1")):
        with pytest.raises(ValueError, match=msg):
            torch_loss.ctc_lattice_align(*args, **kw)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        torch_loss.ctc_lattice_align(em, arcs, na, nn_)
    doc = torch_loss.ctc_lattice_align.__doc__
    assert "path_tokens" in doc and "frame_arcs" in doc and "No autograd" in doc


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU behaviour")
def test_ctc_lattice_align_fails_loudly_without_gpu(gtn):
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.gtn_ctc_lattice_align_n.argtypes = [P, I, I, I, I, P, P, P, P, P, I, I, I, P, P, P, P, P, P, P, P]
    lib.gtn_ctc_lattice_align_n.restype = I
    lib.gtn_criteria_last_error.restype = ctypes.c_char_p
    rc = lib.gtn_ctc_lattice_align_n(None, 1, 2, 8, 0, None, P(64), P(64), P(64), None, 2, 4, 2, P(64), P(64), P(64),
                                     P(64), P(64), P(64), None, None)
    assert rc == -1 and "no HIP device" in lib.gtn_criteria_last_error().decode()
    batch = gtn.Batch([gtn.linear_graph(2, 8)])
    with pytest.raises(RuntimeError, match="no HIP device"):
        batch.ctc_lattice_align(64, 64, 64, 64, 64, 64, 64, 64, 64, A=2, row_stride=6, max_states=4, P=2)
