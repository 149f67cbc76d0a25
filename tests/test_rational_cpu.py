"""Pins the yardstick of tests/rational_fp.py -- numpy versions of clone / project / concat / closure / union / remove,
their adjacency and start / accept lists, the gradient slices and the float64 forward / backward -- to the UNMODIFIED
reference (oracle/_ref through tests/refbackend/gtn_ref.py) on exactly the case list tests/test_rational_gpu.py runs
(tests/rational_cases.py), and to the reference's recorded results in tests/golden/rational.json, which keep the small
cases pinned where oracle/_ref is not built."""
import json
import os
import sys

import numpy as np
import pytest

import rational_cases as rc
import rational_fp as fp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_rational as mk  # noqa: E402

HAVE_REF = os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libgtn_ref.so"))
NEEDS_REF = "needs oracle/_ref (built from the reference's sources by __graft_entry__.build())"
with open(os.path.join(ROOT, "tests", "golden", "rational.json")) as _f:
    FIXTURE = json.load(_f)


def ref():
    sys.path.insert(0, os.path.join(ROOT, "tests", "refbackend"))
    import gtn_ref
    return gtn_ref


@pytest.mark.parametrize("name", list(rc.CASES))
def test_yardstick_builds_what_the_reference_recorded(name):
    """the fixture: every small graph of the case, in full (needs nothing but the committed files)"""
    want = rc.CASES[name](rc.FpOps())
    for key in want.get("nonempty", ()):
        assert fp.A(want["probes"][key]) > 0, (name, key, "an empty probe proves nothing")
    recorded = {k for k in FIXTURE["graphs"] if k.startswith(name + "/")}
    seen = set()
    for kind in ("results", "probes"):
        for key, g in want[kind].items():
            if mk.is_small(g):
                k = "%s/%s/%s" % (name, kind, key)
                assert k in recorded, k + " is small but not in tests/golden/rational.json (run make_rational.py)"
                diff = rc.same(g, mk.unpack(FIXTURE["graphs"][k]))
                assert diff is None, (k, diff)
                seen.add(k)
    assert seen == recorded, recorded - seen
    if name.startswith("rm_") and name != "rm_second_batch":  # remove's walk semantics: all small, all recorded
        assert len(seen) == len(want["results"]) + len(want["probes"]), (name, "a graph of this case is not recorded")


@pytest.mark.skipif(not HAVE_REF, reason=NEEDS_REF)
@pytest.mark.parametrize("name", list(rc.CASES))
def test_yardstick_builds_what_the_reference_builds(name, tmp_path):
    want = rc.CASES[name](rc.FpOps())
    api = ref()
    ops = rc.ApiOps(api, tmp_path)
    got = rc.CASES[name](ops)
    assert set(got["results"]) == set(want["results"]) and set(got["probes"]) == set(want["probes"])
    for kind in ("results", "probes"):
        for key, h in got[kind].items():
            g = want[kind][key]
            diff = rc.same(ops.pull(h), g)
            assert diff is None, (name, kind, key, diff)
            assert (h.num_nodes(), h.num_arcs(), h.num_start(), h.num_accept()) == (
                fp.N(g), fp.A(g), fp.start_list(g).size, fp.accept_list(g).size)
            if fp.N(g) <= 300:  # the adjacency lists, node by node
                outs, ins = fp.out_lists(g), fp.in_lists(g)
                for n in range(fp.N(g)):
                    assert h.out(n) == outs[n] and h.in_(n) == ins[n], (name, kind, key, n)
    for h, g in ops.leaves:
        assert rc.same(ops.pull(h), g) is None


@pytest.mark.skipif(not HAVE_REF, reason=NEEDS_REF)
@pytest.mark.parametrize("name", list(rc.TIE_CASES))
def test_recorded_tie_paths_are_the_references(name, tmp_path):
    rec = mk.unpack(FIXTURE["ties"][name])
    assert fp.A(rec) > 0 and (rec["w"] == np.round(rec["w"])).all()
    ops = rc.ApiOps(ref(), tmp_path)
    assert rc.same(ops.pull(rc.TIE_CASES[name](ops)), rec) is None


@pytest.mark.skipif(not HAVE_REF, reason=NEEDS_REF)
@pytest.mark.parametrize("tropical", [False, True])
@pytest.mark.parametrize("name", list(rc.SCORE_CASES))
def test_float64_recursion_and_slices_against_the_reference(name, tropical):
    """the gates of the GPU test: scores rel = abs = 1e-5, gradients rtol 1e-4, atol 1e-5"""
    want_score, want_grads = rc.score_yardstick(name, tropical)
    assert np.isfinite(want_score)
    api = ref()
    score, grads, _ = rc.score_api(api, name, tropical)
    assert score == pytest.approx(want_score, rel=1e-5, abs=1e-5)
    for g, w, c in zip(grads, want_grads, rc.SCORE_CASES[name][2]):
        if c:
            np.testing.assert_allclose(g, w, rtol=1e-4, atol=1e-5)
    # a retained tape run twice (rational_cases.TWICE)
    _, twice, _ = rc.score_api(api, name, tropical, twice=True)
    for g2, g1, c, k in zip(twice, grads, rc.SCORE_CASES[name][2], rc.TWICE[rc.SCORE_CASES[name][0]]):
        if c:
            np.testing.assert_allclose(g2, k * g1, rtol=1e-6, atol=1e-7)
