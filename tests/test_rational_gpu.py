"""The device-built rational operations, remove and the binary loader (gtn_amd/csrc/rational.hip, ops_rational.cpp)
against the yardstick of tests/rational_fp.py, at the sizes where their loops, scans and sorts take a second trip:
start / accept lists across the 1024-node chunks of the list scan, connectors beyond one block, implicit chains as
inputs, the radix sort's bit count just above a power of two and its stability on a hub, arcs beyond one pass of the
grid, hundreds of inputs and more inputs than the grid's y dimension holds, the loader on both sides of its 4096-arc
threshold, remove's walk semantics and its second batch of walks over shared scratch rows.

Every case (tests/rational_cases.py; tests/test_rational_cpu.py pins the same list to the unmodified reference) checks:
the probes -- what a SECOND device operation made of a result before anything pulled that result to the host, the only
view of the result's adjacency lists, start / accept lists, counts and epsilon flag as they are on the device -- then
the results pulled to the host, then that the inputs are unchanged, then gtn.equal against the same graph built on the
host.  Every structural comparison is ==."""
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

pytestmark = pytest.mark.gpu

with open(os.path.join(ROOT, "tests", "golden", "rational.json")) as _f:
    FIXTURE = json.load(_f)


@pytest.mark.parametrize("name", list(rc.CASES))
def test_device_built_graph(gtn, name, tmp_path):
    want = rc.CASES[name](rc.FpOps())
    ops = rc.ApiOps(gtn, tmp_path)
    got = rc.CASES[name](ops)  # (results and probes are built; nothing has been pulled yet)
    assert set(got["results"]) == set(want["results"]) and set(got["probes"]) == set(want["probes"])
    for key in want.get("nonempty", ()):
        assert fp.A(want["probes"][key]) > 0 and got["probes"][key].num_arcs() > 0, (name, key, "an empty probe")
    for kind in ("probes", "results"):
        for key, h in got[kind].items():
            g = want[kind][key]
            counts = (h.num_nodes(), h.num_arcs(), h.num_start(), h.num_accept())
            assert counts == (fp.N(g), fp.A(g), fp.start_list(g).size, fp.accept_list(g).size), (name, kind, key, counts)
            diff = rc.same(ops.pull(h), g)
            assert diff is None, (name, kind, key, diff)
            rec = FIXTURE["graphs"].get("%s/%s/%s" % (name, kind, key))
            if rec is not None:  # (small: the reference's recorded graph, in full)
                diff = rc.same(ops.pull(h), mk.unpack(rec))
                assert diff is None, (name, kind, key, "recorded", diff)
    for h, g in ops.leaves:
        assert rc.same(ops.pull(h), g) is None, (name, "an input changed")
    for key, h in got["results"].items():
        assert gtn.equal(h, rc.to_api(gtn, want["results"][key])), (name, key)


@pytest.mark.parametrize("name", list(rc.TIE_CASES))
def test_tied_best_path_follows_the_device_in_lists(gtn, name, tmp_path):
    """every path ties exactly, so viterbi_path takes what the in-lists offer first: the arcs of the path are the
    reference's recorded ones only if the device-built in-lists are in the reference's order"""
    ops = rc.ApiOps(gtn, tmp_path)
    path = rc.TIE_CASES[name](ops)
    diff = rc.same(ops.pull(path), mk.unpack(FIXTURE["ties"][name]))
    assert diff is None, (name, diff)


@pytest.mark.parametrize("tropical", [False, True])
@pytest.mark.parametrize("name", list(rc.SCORE_CASES))
def test_scores_and_gradient_slices(gtn, name, tropical):
    """forward_score / viterbi_score through concat, union and compose(closure(g), chain), one input without calc_grad,
    against the float64 recursion on the yardstick's graph sliced by the yardstick's offsets; the gates are those of
    test_parity_gpu.py::test_non_layered_product_is_levelized_on_the_device.  Then the retained tape once more."""
    want_score, want_grads = rc.score_yardstick(name, tropical)
    kind, gs, cg = rc.SCORE_CASES[name]
    score, grads, hs = rc.score_api(gtn, name, tropical)
    assert score == pytest.approx(want_score, rel=1e-5, abs=1e-5)
    for h, g, w, c in zip(hs, grads, want_grads, cg):
        if c:
            np.testing.assert_allclose(g, w, rtol=1e-4, atol=1e-5)
        else:
            assert not h.is_grad_available()
    _, twice, _ = rc.score_api(gtn, name, tropical, twice=True)
    for g2, w, c, k in zip(twice, want_grads, cg, rc.TWICE[kind]):
        if c:
            np.testing.assert_allclose(g2, k * w, rtol=1e-4, atol=k * 1e-5)
    for h, g in zip(hs, gs):
        assert rc.same(rc.from_api(h), g) is None
