"""CTC prefix beam search with a compiled LM graph fused in, the parts that need no GPU.
gtn_amd.LmGraph compiles and walks on the host: every (state, label) of hand-made and generated back-off graphs is
compared with the numpy walk of tests/ctc_beam_graph_fp.py, weights with == as float32.  Every refusal of the compile
raises with its message.  The float64 yardstick (which test_ctc_beam_graph_gpu.py judges the kernel by) is pinned to a
brute-force enumeration and to the search without a language model; every case the GPU file runs vets; the entry points
exist in every layer with matching argument lists and refuse bad arguments before they ask for a device."""
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest

import ctc_beam_fp as fp
import ctc_beam_graph_fp as gfp
from conftest import ROOT


def hand_graph():
    """0 (start): ONE labelled arc (5) and an epsilon arc to 2; 2: label 3 with weight -inf and an epsilon arc to 3;
    3: 69 arcs, labels 0 .. 69 without 7 (not contiguous), no epsilon arc; 4: labels 10 .. 20 (contiguous: the
    one-load layout) and an epsilon arc to 3; 5: nothing at all; 10 .. 18: an epsilon chain of exactly 8 arcs that ends
    in a state whose only arc is label 1"""
    rng = np.random.default_rng(5)
    arcs = [(0, 1, 5, 1.5), (0, 2, -1, -0.25), (2, 0, 3, -np.inf), (2, 3, -1, -0.5)]
    arcs += [(3, int(rng.integers(0, 6)), c, np.float32(rng.normal())) for c in range(70) if c != 7]
    arcs += [(4, 3, -1, 0.125)] + [(4, c % 6, c, np.float32(rng.normal())) for c in range(10, 21)]
    arcs += [(10 + k, 11 + k, -1, np.float32(0.1 * (k + 1))) for k in range(8)] + [(18, 0, 1, 2.0)]
    return gfp.Arcs(19, 0, arcs)


def _same_walks(gtn, G, lm, labels):
    for s in range(G.n):
        for c in labels:
            want_w, want_to = G.walk(s, c)
            got_w, got_to = lm.walk(s, c)
            assert got_to == want_to, (s, c, got_to, want_to)
            if want_to < 0:
                assert got_w == -np.inf
            else:
                assert got_w == float(want_w), (s, c, got_w, want_w)  # (both float32 values; none is NaN)


def test_hand_graph_compiles_and_walks(gtn):
    G = hand_graph()
    lm = gtn.LmGraph(G.to_api(gtn, shuffle_seed=1))  # (arcs given unsorted)
    assert lm.info() == dict(num_states=19, num_arcs=len(G.arcs), start_state=0, longest_epsilon_chain=8)
    _same_walks(gtn, G, lm, range(0, 72))
    # what the graph was made to show
    assert lm.walk(0, 5) == (1.5, 1)                                   # the node with one arc
    w4 = float(np.float32(np.float32(-0.25) + np.float32(-0.5)) + G.out[3][4][1])
    assert lm.walk(0, 4) == (w4, G.out[3][4][0])                       # found only after two back-offs
    assert lm.walk(0, 7) == (-np.inf, -1) and lm.walk(5, 0) == (-np.inf, -1)   # found nowhere: forbidden
    assert lm.walk(2, 3) == (-np.inf, 0) and lm.walk(0, 3) == (-np.inf, 0)     # a -inf arc weight: found, not finite
    w8 = np.float32(0)
    for k in range(8):
        w8 = np.float32(0.1 * (k + 1)) if k == 0 else np.float32(w8 + np.float32(0.1 * (k + 1)))
    assert lm.walk(10, 1) == (float(np.float32(w8 + np.float32(2.0))), 0)       # eight back-offs
    assert lm.walk(4, 15) == (float(G.out[4][15][1]), 15 % 6)              # contiguous labels: the one-load layout
    assert lm.walk(4, 21) == (float(np.float32(np.float32(0.125) + G.out[3][21][1])), G.out[3][21][0])
    assert lm.walk(0, -1) == (-np.inf, -1)  # epsilon is no label to ask for
    with pytest.raises(IndexError):
        lm.walk(19, 0)
    with pytest.raises(IndexError):
        lm.walk(-1, 0)


@pytest.mark.parametrize("kind,C", [("tri", 6), ("wide", 40), ("chain", 6), ("bigram", 9), ("lexicon", 7)])
def test_generated_graphs_walk_like_numpy(gtn, kind, C):
    if kind == "bigram":
        G = gfp.backoff_bigram_graph(4, C)
    elif kind == "lexicon":
        G = gfp.lexicon_graph(4, C)
    else:
        G = gfp.graph_of(3, C, kind)
    lm = gtn.LmGraph(G.to_api(gtn, shuffle_seed=C))
    info = lm.info()
    assert info["num_states"] == G.n and info["num_arcs"] == len(G.arcs) and info["start_state"] == G.start
    assert info["longest_epsilon_chain"] == {"tri": 2, "wide": 2, "chain": 8, "bigram": 1, "lexicon": 0}[kind]
    if kind == "wide":
        assert len(G.out[0]) > 64
    _same_walks(gtn, G, lm, range(0, max(l for _, _, l, _ in G.arcs) + 2))


def test_the_compile_is_a_snapshot(gtn):
    G = gfp.backoff_bigram_graph(1, 5)
    g = G.to_api(gtn)
    lm = gtn.LmGraph(g)
    before = [lm.walk(s, c) for s in range(G.n) for c in range(5)]
    g.set_weights(np.zeros(len(G.arcs), np.float32))
    assert [lm.walk(s, c) for s in range(G.n) for c in range(5)] == before
    del g
    assert [lm.walk(s, c) for s in range(G.n) for c in range(5)] == before


def _graph(gtn, n, starts, arcs):
    g = gtn.Graph(False)
    for s in range(n):
        g.add_node(s in starts, True)
    for a in arcs:
        g.add_arc(a[0], a[1], a[2], a[2], a[3] if len(a) > 3 else 0.0)
    return g


def test_every_refusal_of_the_compile(gtn):
    chain = lambda k: [(s, s + 1, -1) for s in range(k)]
    for n, starts, arcs, msg in (
            (2, (), [(0, 1, 0)], "no start node"),
            (2, (0, 1), [(0, 1, 0)], "more than one start node"),
            (2, (0,), [(0, 1, 3), (0, 0, 1), (0, 0, 3)], "two arcs with the same input label 3 out of node 0"),
            (3, (0,), [(1, 0, -1), (1, 2, 0), (1, 2, -1)], "more than one epsilon arc out of node 1"),
            (3, (0,), [(0, 1, -1), (1, 2, -1), (2, 0, -1)], "epsilon cycle"),
            (2, (0,), [(1, 1, -1)], "epsilon cycle"),
            (10, (0,), chain(9), "epsilon chain longer than 8 arcs")):
        with pytest.raises(ValueError, match=msg):
            gtn.LmGraph(_graph(gtn, n, starts, arcs))
    # a label below -1 never reaches the compile: a Graph refuses the arc itself, in add_arc and in add_arcs alike (the
    # compile checks all the same, for a graph that did not come through them)
    with pytest.raises(ValueError, match="labels must be >= epsilon"):
        _graph(gtn, 2, (0,), [(0, 1, 0), (1, 0, -2)])
    with pytest.raises(ValueError, match="labels must be >= epsilon"):
        _graph(gtn, 2, (0,), []).add_arcs([0], [1], [-2])
    gtn.LmGraph(_graph(gtn, 9, (0,), chain(8)))  # (eight is allowed)
    with pytest.raises(ValueError, match="linear graph"):
        gtn.LmGraph(gtn.linear_graph(2, 3))
    big = gtn.Graph(False)
    n = (1 << 24) + 1
    flags = np.zeros(n, np.uint8)
    flags[0] = 1
    big.add_nodes(flags, np.zeros(n, np.uint8))
    with pytest.raises(ValueError, match=r"more than 2\^24 nodes"):
        gtn.LmGraph(big)


def brute_force_graph(em, blank, G, alpha, beta):
    """{label sequence: (acoustic log score over all C^T alignments, L)} in float64; sequences the graph forbids (or
    whose L is not finite) are left out"""
    T, C = em.shape
    x = em.astype(np.float64)
    am = {}
    for path in itertools.product(range(C), repeat=T):
        y = tuple(c for t, c in enumerate(path) if c != blank and (t == 0 or c != path[t - 1]))
        s = float(sum(x[t, c] for t, c in enumerate(path)))
        am[y] = s if y not in am else max(am[y], s) + math.log1p(math.exp(-abs(am[y] - s)))
    alpha, beta = float(np.float32(alpha)), float(np.float32(beta))
    out = {}
    for y, s in am.items():
        L, state = 0.0, G.start
        for c in y:
            w, state = G.walk(state, c)
            if state < 0:
                L = -math.inf
                break
            L += alpha * float(w) + beta
        if math.isfinite(L):
            out[y] = (s, L)
    return out


@pytest.mark.parametrize("T,C,blank", [(1, 2, 0), (2, 3, 0), (3, 3, 2), (3, 4, 1), (4, 3, 0), (5, 3, 1), (5, 4, 0)])
@pytest.mark.parametrize("kind", ["tri", "chain", "lexicon"])
def test_unpruned_search_is_the_enumeration(T, C, blank, kind):
    em = fp.continuous_case(10 * T + C, 1, T, C)[0]
    G = gfp.lexicon_graph(T, C, 5, 0.6, blank) if kind == "lexicon" else gfp.trigram_graph(T + C, C, 0.5, **gfp.GRAPHS[kind])
    want = brute_force_graph(em, blank, G, 0.7, -0.3)
    assert len(want) > 1
    got = gfp.beam_search_graph(em, blank, 10 ** 6, C, G, 0.7, -0.3, "f64")
    assert [y for y, _, _ in got] == sorted(want, key=lambda y: -(want[y][0] + want[y][1]))
    for y, total, am in got:
        assert abs(am - want[y][0]) <= 1e-9 and abs(total - (want[y][0] + want[y][1])) <= 1e-9, (y, total, am, want[y])


@pytest.mark.parametrize("form", fp.FORMS)
def test_zero_weight_and_bonus_is_the_search_without_a_language_model(form):
    for seed, (T, C, blank, W, K) in enumerate([(40, 6, 0, 8, 4), (65, 5, 4, 4, 3), (3, 3, 1, 64, 3)]):
        em = fp.continuous_case(seed + 30, 2, T, C)
        G = gfp.trigram_graph(seed, C)  # (its unigram state has every label: nothing is forbidden)
        for b, frames in ((0, None), (1, T - 1)):
            plain = fp.beam_search(em[b], blank, W, K, form, frames)
            got = gfp.beam_search_graph(em[b], blank, W, K, G, 0.0, 0.0, form, frames)
            assert [(y, s) for y, s, _ in got] == plain and [(y, a) for y, _, a in got] == plain


def test_a_bigram_graph_is_its_table():
    """the yardstick with a table spelled as a graph, and with a back-off bigram expanded into its table, is
    ctc_beam_lm_fp's: the same lists, the same bits"""
    import ctc_beam_lm_fp as lfp
    T, C, blank, W, K = 30, 7, 0, 8, 5
    em = fp.continuous_case(77, 1, T, C)[0]
    for w, G in ((lfp.table_case(5, C, 0.3), None), (None, gfp.backoff_bigram_graph(5, C))):
        if G is None:
            G = gfp.bigram_graph(w, C)
        else:
            w = gfp.expand_bigram(G, C)
        for form in fp.FORMS:
            a = lfp.beam_search_lm(em, blank, W, K, w, 0.8, 0.5, form)
            b = gfp.beam_search_graph(em, blank, W, K, G, 0.8, 0.5, form)
            assert [y for y, _, _ in a] == [y for y, _, _ in b]
            assert all(x[1].tobytes() == y[1].tobytes() and x[2].tobytes() == y[2].tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("case", gfp.ALL_GPU_CASES, ids=lambda c: "-".join(str(v) for v in c[:8]) + "-" + c[9])
def test_every_gpu_case_vets(case):
    seed, B, T, C, blank, W, K, nbest, frames, gkind = case
    assert nbest <= 4 and nbest <= W
    em, G, res, again = gfp.results_of(case)
    ok, err, gap = gfp.vet_lm(res, nbest)
    print(f"[ctc_beam_graph] {case}: err {err:.3g} smallest gap {gap:.3g} re-created {again}")
    assert ok and err > 0, (err, gap)
    if case in gfp.RECREATED_CASES:
        assert again > 0


def test_the_unpruned_case_prunes_no_ancestor_of_what_it_returns():
    """C = 4 and T = 5 have more label sequences than the 64 a beam can hold, but the returned hypotheses keep their
    exact scores: each equals the enumeration's, so the GPU test may compare am_scores with ctc_score"""
    case = gfp.UNPRUNED_CASE
    seed, B, T, C, blank, W, K, nbest, frames, gkind = case
    assert (T, C, W, K) == (5, 4, 64, 4)
    em, G, res, _ = gfp.results_of(case)
    for b in range(B):
        want = brute_force_graph(em[b], blank, G, gfp.ALPHA, gfp.BETA)
        best = sorted(want, key=lambda y: -(want[y][0] + want[y][1]))[:nbest]
        assert [y for y, _, _ in res["f64"][b][:nbest]] == best
        for y, total, am in res["f64"][b][:nbest]:
            assert abs(am - want[y][0]) <= 1e-9 and abs(total - sum(want[y])) <= 1e-9


def test_the_issues_cases_are_covered():
    cases = gfp.TRIGRAM_CASES
    assert {c[1] for c in cases} == {1, 3} and {c[2] for c in cases} == {7, 66} and {c[3] for c in cases} == {6, 40}
    assert {c[5] for c in cases} == {2, 16, 64} and {c[6] for c in cases} == {3, 32}
    assert any(len(gfp.graph_of(c[0], c[3], c[9]).out[0]) > 64 for c in cases)
    assert any(c[9] == "chain" for c in cases) and gfp.RAGGED_CASE[8] == (40, 1, 0, 39, 33, 2, 40)
    assert len(gfp.RECREATED_CASES) >= 1


def _params(text, name):
    """how many parameters the declaration or definition of `name` has in a C source text"""
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
    assert m, name
    return 0 if m.group(1).strip() in ("", "void") else m.group(1).count(",") + 1


def test_symbols_and_argument_lists(gtn):
    import inspect
    import gtn_amd
    from gtn_amd import _capi, torch_loss
    assert "lm_graph" in inspect.signature(torch_loss.ctc_beam_decode).parameters
    assert hasattr(gtn_amd, "LmGraph") and hasattr(gtn_amd.LmGraph, "walk") and hasattr(gtn_amd.LmGraph, "info")
    eng = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_amd.so"))
    header = open(os.path.join(ROOT, "include", "gtn_amd.h")).read()
    for name in ("gtnx_lm_graph_create", "gtnx_lm_graph_destroy", "gtnx_lm_graph_walk", "gtnx_lm_graph_info",
                 "gtnx_batch_ctc_beam_decode_graph"):
        assert hasattr(eng, name), name
        assert len(_capi._SIGS[name]) == _params(header, name), name
    crit = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    assert hasattr(crit, "gtn_ctc_beam_decode_graph_n")
    capi = open(os.path.join(ROOT, "gtn_amd", "criteria", "criteria_capi.cpp")).read()
    # (x, B, T, C are handed over by _route / _call in front of the listed ones: the list has them all)
    assert len(torch_loss._ARGTYPES["gtn_ctc_beam_decode_graph_n"]) == _params(capi, "gtn_ctc_beam_decode_graph_n")
    assert (_capi._SIGS["gtnx_batch_ctc_beam_decode_graph"][:6] + _capi._SIGS["gtnx_batch_ctc_beam_decode_graph"][7:]
            == _capi._SIGS["gtnx_batch_ctc_beam_decode_lm"][:6] + _capi._SIGS["gtnx_batch_ctc_beam_decode_lm"][7:])
    for path, name in (("include/gtn/batch.h", "class LmGraph"), ("include/gtn/batch.h", "gtnx_batch_ctc_beam_decode_graph"),
                       ("gtn_amd/criteria/ctc_criterion.h", "gtnx_lm_graph_t lmGraph")):
        assert name in open(os.path.join(ROOT, path)).read(), (path, name)


def test_argument_errors_come_before_the_device(gtn):
    """a weight or bonus that is not finite, a destroyed or foreign handle, nbest above beam_size, a table and a graph
    together: refused as invalid arguments, with or without a device"""
    import torch
    import gtn_amd
    from gtn_amd import torch_loss
    batch = gtn.Batch([gtn.linear_graph(2, 8)])
    lm = gtn.LmGraph(gfp.backoff_bigram_graph(1, 8).to_api(gtn))
    inf, nan = float("inf"), float("nan")
    for kw, msg in ((dict(lm_weight=nan), "must be finite"), (dict(insertion_bonus=-inf), "must be finite"),
                    (dict(nbest=17), "nbest above beam_size"), (dict(beam_size=65), "beam_size outside")):
        with pytest.raises(ValueError, match=msg):
            batch.ctc_beam_decode(64, 64, 64, row_stride=2, lm=lm, **kw)
    p = ctypes.c_void_p
    call = gtn_amd._lib.gtnx_batch_ctc_beam_decode_graph
    err = lambda: gtn_amd._lib.gtnx_last_error().decode()
    assert call(batch._h, None, 0, 16, 16, 1, p(lm._h), nan, 0.0, p(64), 2, p(64), p(64), None) == 1
    assert call(batch._h, None, 0, 16, 16, 1, None, 1.0, 0.0, p(64), 2, p(64), p(64), None) == 1 and "null LM graph" in err()
    stack = ctypes.create_string_buffer(256)  # (memory that is no handle)
    assert call(batch._h, None, 0, 16, 16, 1, ctypes.addressof(stack), 1.0, 0.0, p(64), 2, p(64), p(64), None) == 1
    assert "not a live LM graph handle" in err()
    gone = lm._h
    lm.destroy()
    assert call(batch._h, None, 0, 16, 16, 1, p(gone), 1.0, 0.0, p(64), 2, p(64), p(64), None) == 1
    assert "not a live LM graph handle" in err()
    with pytest.raises(ValueError, match="null LM graph handle"):
        batch.ctc_beam_decode(64, 64, 64, row_stride=2, lm=lm)
    with pytest.raises(ValueError, match="not a live LM graph handle"):
        lm._h = gone
        try:
            lm.walk(0, 0)
        finally:
            lm._h = None
    assert gtn_amd._lib.gtnx_lm_graph_destroy(p(gone)) == 1 and gtn_amd._lib.gtnx_lm_graph_destroy(None) == 0
    lm2 = gtn.LmGraph(gfp.backoff_bigram_graph(1, 8).to_api(gtn))
    em = torch.zeros(2, 3, 8)
    for kw, msg in ((dict(lm_graph=lm2, transitions=torch.zeros(8, 8)), "not both"),
                    (dict(lm_graph=lm2, start=torch.zeros(8)), "not both"),
                    (dict(lm_graph=object()), "must be a gtn_amd.LmGraph"),
                    (dict(lm_graph=lm2, lm_weight=nan), "must be finite"),
                    (dict(lm_graph=lm2, beam_size=4, nbest=5), "nbest outside")):
        with pytest.raises(ValueError, match=msg):
            torch_loss.ctc_beam_decode(em, **kw)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        torch_loss.ctc_beam_decode(em, lm_graph=lm2)
