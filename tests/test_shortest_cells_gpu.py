"""forwardScore / viterbiScore / viterbiPath and their gradients on BUILT graphs (gtn_amd/csrc/shortest.hip) in every
cell of the host's dispatch: family (generic / narrow LDS ring / deep one-wave) x lanes per node (1, 8, 64, 256) x
semiring or mode x direction.  Every test first proves, by the route counters (gtn.debug_shortest_routes), that the
launch took the cell the case names, then judges the values against tests/shortest_fp.py:

  log semiring   |device - float64 form| <= FACTOR * err, score and every gradient entry, with
                 err = max(|float32 form - float64 form|, 2^-23 * max(1, |float64|)) from the two host forms alone -- and
                 never looser than what the parity suite grants against the oracle (score rel 1e-4; gradient rtol 2e-3,
                 atol 1e-6): both bounds are asserted;
  tropical       vetted cases (runner-up >= 64 err away at every node of the best path): score == the float32 form,
                 gradient == the 0/1 vector, path labels == the path's arc ids, path weights == those arcs' weights;
  ties           integer weights: everything == the oracle, which carries the reference's tie rules.

FACTOR / FACTOR_DEEP are the power of two at or above twice the largest ratio measured on an MI355X (DESIGN.md section
29 has the figures per family); every test prints its ratios before it asserts."""
import numpy as np
import pytest

import graphgen as gg
import shortest_fp as sf
from oracle_lib import OGraph

pytestmark = pytest.mark.gpu

FACTOR = 8.0        # generic and narrow cells
FACTOR_DEEP = 8.0   # deep cells (hardware exp / log on the staged path)
WORST = {}


def routed(gtn, fn):
    """(fn(), {cell: launches it took}) -- cells without a launch left out"""
    before = gtn.debug_shortest_routes()
    out = fn()
    after = gtn.debug_shortest_routes()
    return out, {k: after[k] - before[k] for k in after if after[k] != before[k]}


def judge_log(tag, family, factor, y, score, grad):
    """prints the ratios, then asserts both bounds"""
    rs = abs(float(score) - y["score"]) / y["score_err"]
    rg = 0.0
    if grad is not None:
        rg = float((np.abs(grad.astype(np.float64) - y["grad"]) / y["grad_err"]).max())
    WORST[family] = max(WORST.get(family, 0.0), rs, rg)
    print(f"[shortest_cells] {tag}: score ratio {rs:.3g} (err {y['score_err']:.3g}), gradient ratio {rg:.3g}; "
          f"largest so far in {family}: {WORST[family]:.3g}")
    assert rs <= factor and abs(float(score) - y["score"]) <= 1e-4 * abs(y["score"]), (tag, rs)
    if grad is not None:
        d = np.abs(grad.astype(np.float64) - y["grad"])
        assert rg <= factor, (tag, rg)
        assert (d <= 1e-6 + 2e-3 * np.abs(y["grad"])).all(), (tag, float(d.max()))


def run_log(gtn, g, cells, want_grad=True):
    api = gg.to_api(gtn, g)
    fs, r = routed(gtn, lambda: gtn.forward_score(api))
    score = fs.item()
    assert r == {cells["fwd_log"]: 1}, r
    if not want_grad:
        return score, None
    _, r = routed(gtn, lambda: gtn.backward(fs))
    assert r == {cells["bwd_log"]: 1}, r
    return score, api.grad().weights_to_numpy()


def run_tropical(gtn, g, cells):
    """(viterbi score, its gradient, path labels, path weights, the path's gradient), every launch in its cell"""
    api = gg.to_api(gtn, g)
    vs, r = routed(gtn, lambda: gtn.viterbi_score(api))
    score = np.float32(vs.item())
    assert r == {cells["fwd_trop"]: 1}, r
    _, r = routed(gtn, lambda: gtn.backward(vs))
    assert r == {cells["bwd_trop"]: 1}, r
    grad = api.grad().weights_to_numpy()
    api2 = gg.to_api(gtn, g)
    path, r = routed(gtn, lambda: gtn.viterbi_path(api2))
    assert r == {cells["path"]: 1}, r
    gtn.backward(path)
    return score, grad, path.labels_to_list(), path.weights_to_numpy(), api2.grad().weights_to_numpy()


def judge_tropical(tag, g, y, got):
    score, grad, labels, pw, pgrad = got
    assert y["vet"] is None, (tag, y["vet"])
    assert score == y["trop_score32"], (tag, score, y["trop_score32"])
    np.testing.assert_array_equal(grad, y["trop_grad"], err_msg=tag)
    assert labels == y["trop_path"], tag
    assert pw.tobytes() == g["w"][y["trop_path"]].tobytes(), tag
    np.testing.assert_array_equal(pgrad, y["trop_grad"], err_msg=tag)


@pytest.mark.parametrize("name", list(sf.GENERIC))
def test_generic_cells(gtn, name):
    """every shape of the generic family: forward log, forward tropical, viterbi_path and both gradients.  (The
    300-accepts cases carry accept nodes with score -inf: the reference's log gradient is NaN there -- exp(-inf + inf)
    -- so those are judged on both scores, the tropical gradient and the path; their 300-live-accepts twins, the same
    shape with every accept node reachable, carry the log gradient over more than 256 accept nodes.)"""
    g = sf.build(name)
    cells = sf.expected_cells(name)
    y = sf.case_yardstick(name)
    score, grad = run_log(gtn, g, cells, want_grad="dead_accepts" not in g)
    got = run_tropical(gtn, g, cells)
    judge_log(name, "generic", FACTOR, y, score, grad)
    judge_tropical(name, g, y, got)


@pytest.mark.parametrize("name", list(sf.TIES))
def test_ties_as_the_reference_breaks_them(gtn, name):
    """integer weights in {-2..1} on multi-node levels with several equal accept nodes.  "unsorted": in- and out-lists
    in arc-id order.  "sorted": the same structure and weights with the labels a permutation of the arc ids, arc-sorted,
    so every list is reordered and a row's slot order is not its arc-id order -- a kernel that ranked tropical ties by
    arc id instead of by slot differs there (tests/test_shortest_cells_cpu.py checks that it would).  (A host-built
    schedule never sets SCHED_TIE_BY_ARC: the by-arc-id rank belongs to device-built schedules, which
    tests/test_parity_gpu.py and test_lazy_gpu.py cover.)"""
    g = sf.build(name)
    og = OGraph.from_dict(sf.as_lists(g))
    score, grad, labels, pw, pgrad = run_tropical(gtn, g, sf.expected_cells(name))
    assert score == np.float32(og.shortest_distance(True))
    np.testing.assert_array_equal(grad, og.shortest_distance_grad(True))
    arcs, _ = og.shortest_path()
    assert labels == g["il"][arcs].tolist()
    assert pw.tobytes() == g["w"][arcs].tobytes()
    want = np.zeros(g["src"].size, np.float32)
    want[arcs] = 1
    np.testing.assert_array_equal(pgrad, want)


@pytest.mark.parametrize("name", list(sf.DEEP))
def test_deep_cells(gtn, name, monkeypatch):
    """the one-wave kernels at their edges, then the same graph on the generic kernels (GTNX_NO_DEEP=1, read per call)"""
    g = sf.build(name)
    y = sf.case_yardstick(name)
    deep = sf.DEEP[name][1]
    score, grad = run_log(gtn, g, sf.expected_cells(name))
    monkeypatch.setenv("GTNX_NO_DEEP", "1")
    score2, grad2 = run_log(gtn, g, sf.expected_cells(name, no_deep=True))
    monkeypatch.delenv("GTNX_NO_DEEP")
    judge_log(name, "deep" if deep else "generic", FACTOR_DEEP if deep else FACTOR, y, score, grad)
    judge_log(name + " (GTNX_NO_DEEP)", "generic", FACTOR, y, score2, grad2)


@pytest.mark.parametrize("name", list(sf.NARROW))
def test_narrow_eligibility_edges(gtn, name):
    """host-built graphs on either side of every rule that admits the LDS-ring kernel"""
    g = sf.build(name)
    cells = sf.expected_cells(name)
    score, grad = run_log(gtn, g, cells)
    judge_log(name, "narrow" if cells["fwd_log"].startswith("fwd/narrow") else "generic", FACTOR, sf.case_yardstick(name), score, grad)


@pytest.mark.parametrize("name", list(sf.BATCHES))
def test_batch_level_selection(gtn, name):
    """the cell is chosen from the batch totals: every element judged against its own yardstick, tropical results
    bit for bit what the element gives alone (where it takes another cell)"""
    gs = sf.build(name)
    cells = sf.expected_cells(name)
    solo_cells = [{w: sf.predict([g], w) for w in ("fwd_log", "bwd_log", "fwd_trop", "bwd_trop", "path")} for g in gs]
    assert any(s["fwd_log"] != cells["fwd_log"] for s in solo_cells), "no element would take another cell alone"
    apis = [gg.to_api(gtn, g) for g in gs]
    fs, r = routed(gtn, lambda: gtn.forward_score(apis))
    scores = gtn.items(fs)
    assert r == {cells["fwd_log"]: 1}, r
    _, r = routed(gtn, lambda: gtn.backward(fs))
    assert r == {cells["bwd_log"]: 1}, r
    for i, (g, api) in enumerate(zip(gs, apis)):
        judge_log("%s[%d]" % (name, i), "generic", FACTOR, sf.case_yardstick(name, i), scores[i], api.grad().weights_to_numpy())
    apis = [gg.to_api(gtn, g) for g in gs]
    vs, r = routed(gtn, lambda: gtn.viterbi_score(apis))
    vscores = gtn.items(vs)
    assert r == {cells["fwd_trop"]: 1}, r
    _, r = routed(gtn, lambda: gtn.backward(vs))
    assert r == {cells["bwd_trop"]: 1}, r
    apis2 = [gg.to_api(gtn, g) for g in gs]
    paths, r = routed(gtn, lambda: gtn.viterbi_path(apis2))
    assert r == {cells["path"]: 1}, r
    gtn.backward(paths)
    for i, g in enumerate(gs):
        got = (np.float32(vscores[i]), apis[i].grad().weights_to_numpy(), paths[i].labels_to_list(),
               paths[i].weights_to_numpy(), apis2[i].grad().weights_to_numpy())
        judge_tropical("%s[%d]" % (name, i), g, sf.case_yardstick(name, i), got)
        solo = run_tropical(gtn, g, solo_cells[i])  # alone, in the cell the element would take by itself
        assert solo[0].tobytes() == got[0].tobytes() and solo[1].tobytes() == got[1].tobytes()
        assert solo[2] == got[2] and solo[3].tobytes() == got[3].tobytes() and solo[4].tobytes() == got[4].tobytes()
