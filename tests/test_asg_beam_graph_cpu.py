"""ASG prefix beam search with a compiled LM graph fused in, the parts that need no GPU.  The
float64 yardstick of tests/asg_beam_graph_fp.py (which test_asg_beam_graph_gpu.py judges the kernel by) is pinned to a
brute-force enumeration and to the search without a language model; every case the GPU file runs vets, so its tokens may
be compared with ==; the conditions the GPU tests rely on (a prefix is created again, the lexicon's constraint bites, no
score of the identity cases is a zero) are checked here; the entry points exist in every layer with matching argument
lists and refuse bad arguments before they ask for a device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import asg_beam_fp as af
import asg_beam_graph_fp as gfp
import ctc_beam_fp as cf
from conftest import ROOT


def _graph(kind, seed, C):
    if kind == "lexicon":
        return gfp.lexicon_graph(seed, C, 5, 0.6, blank=-1)
    return gfp.trigram_graph(seed, C, 0.5, **gfp.GRAPHS[kind])


@pytest.mark.parametrize("T,C", [(1, 2), (2, 3), (3, 3), (3, 4), (4, 3), (5, 3), (5, 4)])
@pytest.mark.parametrize("kind", ["tri", "chain", "lexicon"])
def test_unpruned_search_is_the_enumeration(T, C, kind):
    """all label sequences without equal neighbours: am = the log-sum over the labellings that collapse to the
    sequence, L = the walked sum; a sequence the graph does not accept is absent; unpruned, the list is exactly the
    accepted sequences with a finite score, ordered by am + L"""
    em = af.continuous_case(10 * T + C, 1, T, C)[0]
    table = af.table_case(T + C, C, 0.2 if kind == "chain" else 0.0)
    G = _graph(kind, T + C, C)
    want = gfp.brute_force_graph(em, table, G, 0.7, -0.3)
    assert len(want) > 1
    every = af.brute_force(em, table)
    assert all(gfp.accepts(G, y) for y in want) and all(not gfp.accepts(G, y) for y in every if y not in want)
    if kind == "lexicon" and T >= 3:  # (the start state keeps two labels by construction: at T = 1, C = 2 that is all)
        assert len(want) < len(every)
    got = gfp.beam_search_graph(em, table, 10 ** 6, C, G, 0.7, -0.3, "f64")
    assert [y for y, _, _ in got] == sorted(want, key=lambda y: -want[y][0])
    for y, total, am in got:
        assert all(a != c for a, c in zip(y, y[1:]))
        assert abs(am - want[y][1]) <= 1e-9 and abs(total - want[y][0]) <= 1e-9, (y, total, am, want[y])


@pytest.mark.parametrize("form", cf.FORMS)
def test_zero_weight_and_bonus_is_the_search_without_a_language_model(form):
    for seed, (T, C, W, K) in enumerate([(40, 6, 8, 4), (65, 5, 4, 3), (3, 3, 64, 3)]):
        em = af.continuous_case(seed + 30, 2, T, C)
        table = af.table_case(seed + 30, C)
        G = gfp.trigram_graph(seed, C)  # (its unigram state has every label: nothing is forbidden)
        for b, frames in ((0, None), (1, T - 1)):
            plain = af.beam_search(em[b], table, W, K, form, frames)
            got = gfp.beam_search_graph(em[b], table, W, K, G, 0.0, 0.0, form, frames)
            assert [(y, s) for y, s, _ in got] == plain and [(y, a) for y, _, a in got] == plain


@pytest.mark.parametrize("holes", [0.0, 0.3])
@pytest.mark.parametrize("shape", gfp.IDENTITY_SHAPES, ids=lambda s: "B{}-T{}-C{}-W{}-K{}".format(*s))
def test_a_zero_weight_bigram_acceptor_is_the_struck_out_table(shape, holes):
    """the float32 form with the 0 / -inf acceptor gives the lists and the bits of the plain search on the struck-out
    table, whatever the weight; and no score there is +0 or -0, so that s + 0 has s's bits on the device as well"""
    B, T, C, W, K = shape
    em, table, G, struck = gfp.identity_case(shape, holes)
    if holes:
        assert np.isneginf(struck).any() and np.isfinite(struck[C::C + 1]).all()
        assert any(not np.isfinite(struck[C + i * C + j]) for j in range(C) for i in range(C) if i != j)
    else:
        assert struck.tobytes() == table.tobytes()
    for b in range(B):
        plain = af.beam_search(em[b], struck, W, K, "f32")
        got = gfp.beam_search_graph(em[b], table, W, K, G, 0.7, 0.0, "f32")
        assert [y for y, _ in plain] == [y for y, _, _ in got] and len(plain) > 0
        for (_, s), (_, total, am) in zip(plain, got):
            assert s != 0 and s.tobytes() == total.tobytes() == am.tobytes()


def _id(case):
    return "-".join(str(v) for v in case[:7]) + "-" + case[8]


@pytest.mark.parametrize("case", gfp.ALL_GPU_CASES, ids=_id)
def test_every_gpu_case_vets(case):
    seed, B, T, C, W, K, nbest, frames, gkind = case
    assert nbest <= 4 and nbest <= W
    em, table, G, res, again = gfp.results_of(case)
    ok, err, gap = gfp.vet_lm(res, nbest)
    print(f"[asg_beam_graph] {case}: err {err:.3g} smallest gap {gap:.3g} re-created {again}")
    assert ok and err > 0, (err, gap)
    if case in gfp.RECREATED_CASES:
        assert again > 0
    for h in res["f64"]:
        assert all(gfp.accepts(G, y) for y, _, _ in h)


def test_the_lexicon_constraint_bites():
    """at least one hypothesis of the plain float64 decode is not accepted by the graph, and the constrained best of
    every utterance is finite"""
    assert gfp.LEXICON_CASE[8] == "lex" and gfp.constraint_bites(gfp.LEXICON_CASE)
    G = gfp.results_of(gfp.LEXICON_CASE)[2]
    assert all(-1 not in out for out in G.out)  # (no epsilon arcs: what a state lacks is forbidden from it)


def test_the_unpruned_case_prunes_no_ancestor_of_what_it_returns():
    """C = 4 and T = 5 have more label sequences than the 64 a beam can hold, but the returned hypotheses keep their
    exact scores: each equals the enumeration's, so the GPU test may compare am_scores with asg_score"""
    case = gfp.UNPRUNED_CASE
    seed, B, T, C, W, K, nbest, frames, gkind = case
    assert (B, T, C, W, K, nbest) == (2, 5, 4, 64, 4, 4)
    em, table, G, res, _ = gfp.results_of(case)
    for b in range(B):
        want = gfp.brute_force_graph(em[b], table, G, gfp.ALPHA, gfp.BETA)
        best = sorted(want, key=lambda y: -want[y][0])[:nbest]
        assert [y for y, _, _ in res["f64"][b][:nbest]] == best
        for y, total, am in res["f64"][b][:nbest]:
            assert abs(am - want[y][1]) <= 1e-9 and abs(total - want[y][0]) <= 1e-9


def test_the_issues_cases_are_covered():
    shapes = [c[1:7] for c in gfp.TRIGRAM_CASES]
    assert shapes == [(1, 7, 6, 2, 3, 2), (3, 66, 40, 16, 32, 4), (1, 66, 6, 64, 5, 4), (3, 7, 40, 64, 32, 4)]
    assert [c[8] for c in gfp.TRIGRAM_CASES] == ["tri", "wide", "chain", "tri"]
    wide = gfp.TRIGRAM_CASES[1]
    out0 = gfp.graph_of(wide[0], wide[3], wide[8]).out[0]
    labels = sorted(l for l in out0 if l >= 0)
    assert len(labels) > 64 and labels != list(range(labels[0], labels[0] + len(labels)))
    assert [c[1:7] + (c[8],) for c in gfp.RECREATED_CASES] == [(2, 40, 4, 4, 3, 2, "tri")]
    assert gfp.RAGGED_CASE[7] == (40, 1, 0, 39, 33, 2, 40) and gfp.UNPRUNED_CASE[1:7] == (2, 5, 4, 64, 4, 4)
    # the list of the chain case grows above 32 prefixes: the second pass of the walks runs
    chain = gfp.TRIGRAM_CASES[2]
    assert max(len(h) for h in gfp.results_of(chain)[3]["f64"]) > 32


def _params(text, name):
    """how many parameters the declaration or definition of `name` has in a C source text"""
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return 0 if body.strip() in ("", "void") else body.count(",") + 1


def test_symbols_and_argument_lists(gtn):
    from gtn_amd import _capi, torch_loss
    sig = inspect.signature(torch_loss.asg_beam_decode).parameters
    keys = ("lm_graph", "lm_weight", "insertion_bonus", "return_am_scores")
    assert [sig[k].default for k in keys] == [None, 1.0, 0.0, False]
    sig = inspect.signature(gtn.Batch.asg_beam_decode).parameters
    assert [sig[k].default for k in ("lm", "lm_weight", "insertion_bonus", "am_scores_out")] == [None, 1.0, 0.0, None]
    eng = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_amd.so"))
    header = open(os.path.join(ROOT, "include", "gtn_amd.h")).read()
    name = "gtnx_batch_asg_beam_decode_graph"
    assert hasattr(eng, name)
    assert len(_capi._SIGS[name]) == _params(header, name) == 14
    # the plain call's arguments with (lm_graph, lm_weight, insertion_bonus) after nbest and am_scores at the end
    plain = _capi._SIGS["gtnx_batch_asg_beam_decode"]
    assert _capi._SIGS[name][:6] == plain[:6] and _capi._SIGS[name][9:13] == plain[6:]
    assert _capi._SIGS[name][6:9] == [ctypes.c_void_p, ctypes.c_float, ctypes.c_float]
    crit = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    assert hasattr(crit, "gtn_asg_beam_decode_graph_n")
    capi = open(os.path.join(ROOT, "gtn_amd", "criteria", "criteria_capi.cpp")).read()
    name = "gtn_asg_beam_decode_graph_n"
    assert len(torch_loss._ARGTYPES[name]) == _params(capi, name) == 16
    for path, text in (("include/gtn/batch.h", "gtnx_batch_asg_beam_decode_graph"),
                       ("include/gtn/batch.h", "const LmGraph& lm, float lmWeight"),
                       ("gtn_amd/criteria/asg_criterion.h", "gtnx_lm_graph_t lmGraph")):
        assert text in open(os.path.join(ROOT, path)).read(), (path, text)


def test_argument_errors_come_before_the_device(gtn):
    """an lm that is no LmGraph, weights or am_scores_out without lm, a weight or bonus that is not finite, a
    destroyed or foreign handle: refused as invalid arguments, with or without a device, under the graph call's name"""
    import torch
    import gtn_amd
    from gtn_amd import torch_loss
    C = 8
    batch = gtn.Batch([gtn.linear_graph(2, C)])
    lm = gtn.LmGraph(gfp.trigram_graph(1, C).to_api(gtn))
    inf, nan = float("inf"), float("nan")
    call = lambda **kw: batch.asg_beam_decode(64, 64, 64, None, 64, row_stride=2, **kw)
    for kw, msg in ((dict(lm=object()), "lm must be an LmGraph"),
                    (dict(lm=np.zeros(C + C * C, np.float32)), "lm must be an LmGraph"),
                    (dict(lm_weight=0.5), "need lm"), (dict(insertion_bonus=0.5), "need lm"),
                    (dict(am_scores_out=64), "need lm"),
                    (dict(lm=lm, lm_weight=nan), "must be finite"),
                    (dict(lm=lm, insertion_bonus=-inf), "must be finite"),
                    (dict(lm=lm, lm_weight=inf), "must be finite"),
                    (dict(lm=lm, nbest=17), "nbest outside 1 .. beam_size"),
                    (dict(lm=lm, beam_size=65), "beam_size outside")):
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    with pytest.raises(ValueError, match=r"\[gtnx_batch_asg_beam_decode_graph\] nbest outside"):
        call(lm=lm, nbest=17)
    with pytest.raises(ValueError, match=r"\[gtnx_batch_asg_beam_decode\] nbest outside"):
        call(nbest=17)
    p = ctypes.c_void_p
    fn = gtn_amd._lib.gtnx_batch_asg_beam_decode_graph
    err = lambda: gtn_amd._lib.gtnx_last_error().decode()
    prefix = "[gtnx_batch_asg_beam_decode_graph] "
    assert fn(batch._h, None, p(64), 16, 16, 1, p(lm._h), nan, 0.0, p(64), 2, p(64), p(64), None) == 1
    assert err().startswith(prefix + "lm_weight and insertion_bonus must be finite")
    assert fn(batch._h, None, p(64), 16, 16, 1, p(lm._h), 1.0, inf, p(64), 2, p(64), p(64), None) == 1
    assert err().startswith(prefix + "lm_weight and insertion_bonus must be finite")
    assert fn(batch._h, None, p(64), 16, 16, 1, None, 1.0, 0.0, p(64), 2, p(64), p(64), None) == 1
    assert err().startswith(prefix + "null LM graph handle")
    assert fn(batch._h, None, None, 16, 16, 1, p(lm._h), 1.0, 0.0, p(64), 2, p(64), p(64), None) == 1
    assert err().startswith(prefix + "null table pointer")
    stack = ctypes.create_string_buffer(256)  # (memory that is no handle)
    assert fn(batch._h, None, p(64), 16, 16, 1, ctypes.addressof(stack), 1.0, 0.0, p(64), 2, p(64), p(64), None) == 1
    assert err().startswith(prefix + "not a live LM graph handle")
    gone = lm._h
    lm.destroy()
    assert fn(batch._h, None, p(64), 16, 16, 1, p(gone), 1.0, 0.0, p(64), 2, p(64), p(64), None) == 1
    assert err().startswith(prefix + "not a live LM graph handle")
    with pytest.raises(ValueError, match="null LM graph handle"):
        call(lm=lm)
    lm2 = gtn.LmGraph(gfp.trigram_graph(1, C).to_api(gtn))
    em, tr = torch.zeros(2, 3, C), torch.zeros(C, C)
    for kw, msg in ((dict(lm_graph=object()), "must be a gtn_amd.LmGraph"),
                    (dict(lm_graph=lm2, lm_weight=nan), "must be finite"),
                    (dict(lm_graph=lm2, insertion_bonus=inf), "must be finite"),
                    (dict(lm_weight=0.5), "need lm_graph"), (dict(insertion_bonus=1.0), "need lm_graph"),
                    (dict(return_am_scores=True), "need lm_graph"),
                    (dict(lm_graph=lm2, beam_size=4, nbest=5), "nbest outside")):
        with pytest.raises(ValueError, match=msg):
            torch_loss.asg_beam_decode(em, tr, **kw)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        torch_loss.asg_beam_decode(em, tr, lm_graph=lm2, return_am_scores=True)
