"""compose / intersect (gtn_amd/csrc/compose.hip, compose_wide.hip, ops_compose.cpp) in every cell of the dispatch, one
case per cell and one on either side of every threshold (tests/compose_cells.py has the table and the model of the
dispatch, tests/test_compose_cells_cpu.py pins both to the oracle).  Every test first proves, by the route counters
(gtn.debug_compose_routes), that the product went the way the case names; then

  structure   num_nodes, num_arcs, start, accept, src, dst, ilabel, olabel == the oracle's, weights equal as bytes: node
              ids, arc ids, arc order and float32 weights are the reference's by contract (header of compose.hip);
  gradient    gtn.backward(product, seed) with integer seeds in [-3, 3]: every sum is exact in float32 whatever order
              the atomics land in, so both input gradients == OGraph.compose_grad;
  scores      on non-empty acyclic products forward_score, viterbi_score and their gradients against the oracle run on
              its own product, with what the parity suite grants those calls: score RTOL of tests/test_parity_gpu.py,
              gradients rtol 1e-3 / atol 1e-4 (test_wide_chain_products_vs_oracle).  The largest error seen per route,
              as a fraction of what is granted, is printed (DESIGN.md section 36 has the figures of an MI355X);
  switches    a case run under an env switch or in a batch == the same pair composed alone without it, bit for bit."""
import numpy as np
import pytest

import compose_cells as cc
from test_parity_gpu import RTOL

pytestmark = pytest.mark.gpu

GRAD_RTOL, GRAD_ATOL = 1e-3, 1e-4
WORST = {}


def routed(gtn, fn):
    before = gtn.debug_compose_routes()
    out = fn()
    after = gtn.debug_compose_routes()
    return out, {k: after[k] - before[k] for k in after if after[k] != before[k]}


def compose_calls(gtn, name, pairs=None, calls=None, env=True):
    """the case's operands and products: ([(a, b)], [product]); device-built operands are composed on the way"""
    c = cc.CASES[name]
    pairs = cc.build(name) if pairs is None else pairs
    fn = gtn.intersect if c["mode"] == "intersect" else gtn.compose
    ops = [(cc.to_api(gtn, a), cc.to_api(gtn, b)) for a, b in pairs]
    comps = []
    for lo, hi in (calls or cc.calls_of(name)):
        if hi - lo == 1:
            comps.append(fn(ops[lo][0], ops[lo][1]))
        else:
            comps += fn([o[0] for o in ops[lo:hi]], [o[1] for o in ops[lo:hi]])
    return ops, comps


def arrays_of(comp):
    s, d, il, ol, w = comp.arcs()
    return (np.asarray(comp.start(), np.int64), np.asarray(comp.accept(), np.int64), s, d, il, ol, w)


def same_arrays(tag, got, want):
    for k, (g, w) in enumerate(zip(got[:6], want[:6])):
        np.testing.assert_array_equal(g, w, err_msg="%s: %s" % (tag, ("start", "accept", "src", "dst", "il", "ol")[k]))
    assert got[6].tobytes() == want[6].tobytes(), tag + ": weights"


def seed_graph(gtn, deltas):
    g = gtn.Graph(False)
    g.add_nodes([1, 0], [0, 1])
    A = len(deltas)
    if A:
        z = np.zeros(A, np.int32)
        g.add_arcs(z, z + 1, z, z, np.asarray(deltas, np.float32))
    return g


def grads_of(op):
    return op.grad().weights_to_numpy()


def note(family, what, got, want, rtol, atol):
    d = np.atleast_1d(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)))
    granted = np.atleast_1d(atol + rtol * np.abs(np.asarray(want, np.float64)))
    r = float(np.where(d > 0, d / np.maximum(granted, 1e-300), 0.0).max()) if d.size else 0.0
    WORST[family] = max(WORST.get(family, 0.0), r)
    print("[compose_cells] %s %s: %.3g of the granted error; largest so far on this route: %.3g" % (family, what, r, WORST[family]))
    return r


def family_of(routes):
    first = [c for c in cc.CELLS[:6] if c in routes]
    redo = [c for c in cc.CELLS[6:10] if c in routes]
    return (redo or first or ["symbolic"])[0]


def check_scores(gtn, name, family, oracles):
    """forward_score / viterbi_score of fresh products and the gradients they send through compose"""
    pairs = cc.build(name)
    for tropical in (False, True):
        want = [oc.shortest_distance(tropical) if oc.N else None for oc in oracles]
        if all(w is None for w in want):
            return      # empty or cyclic: the reference has no score either
        ops, comps = compose_calls(gtn, name)
        live = [k for k, w in enumerate(want) if w is not None]
        sel = [comps[k] for k in live]
        scores = gtn.viterbi_score(sel) if tropical else gtn.forward_score(sel)
        got = gtn.items(scores)
        for k, s in zip(live, got):
            note(family, "viterbi_score" if tropical else "forward_score", s, want[k], RTOL, 0.0)
            assert s == pytest.approx(want[k], rel=RTOL), (name, k, tropical)
        gtn.backward(scores)
        for k in live:
            oc, (a, b) = oracles[k], pairs[k]
            g1, g2 = oc.compose_grad(oc.shortest_distance_grad(tropical), cc.num_arcs(a), cc.num_arcs(b))
            for side, (op, g) in enumerate(zip(ops[k], (g1, g2))):
                if g.size == 0:
                    continue
                got_g = grads_of(op)
                note(family, "%s gradient of g%d" % ("viterbi" if tropical else "forward", side + 1), got_g, g, GRAD_RTOL, GRAD_ATOL)
                np.testing.assert_allclose(got_g, g, rtol=GRAD_RTOL, atol=GRAD_ATOL, err_msg="%s[%d] g%d" % (name, k, side + 1))


@pytest.mark.parametrize("name", list(cc.CASES))
def test_cells(gtn, name, monkeypatch):
    c = cc.CASES[name]
    pairs = cc.build(name)
    oracles = cc.oracle_products(name)
    for e in c["env"]:
        monkeypatch.setenv(e, "1")
    if c.get("compose_mode") is not None:
        gtn.compose_mode(c["compose_mode"])
    try:
        (ops, comps), routes = routed(gtn, lambda: compose_calls(gtn, name))
    finally:
        gtn.compose_mode(0)
    print("[compose_cells] %s: %s" % (name, routes))
    assert routes == cc.expected_routes(name), (name, routes, cc.expected_routes(name))
    family = family_of(routes)
    # ---- the product
    got = []
    for k, (comp, oc) in enumerate(zip(comps, oracles)):
        assert (comp.num_nodes(), comp.num_arcs()) == (oc.N, oc.A), (name, k)
        got.append(arrays_of(comp))
        same_arrays("%s[%d]" % (name, k), got[-1], cc.oracle_arrays(oc))
    if c.get("compose_mode") is not None:
        check_scores_symbolic(gtn, name, oracles)
        return
    # ---- its gradient, exactly
    rng = cc.rng_of(name + "/seed")
    for k, (comp, oc) in enumerate(zip(comps, oracles)):
        deltas = rng.integers(-3, 4, oc.A).astype(np.float32)
        gtn.backward(comp, seed_graph(gtn, deltas))
        (a, b) = pairs[k]
        g1, g2 = oc.compose_grad(deltas, cc.num_arcs(a), cc.num_arcs(b))
        np.testing.assert_array_equal(grads_of(ops[k][0]), g1, err_msg="%s[%d] g1" % (name, k))
        np.testing.assert_array_equal(grads_of(ops[k][1]), g2, err_msg="%s[%d] g2" % (name, k))
    # ---- scores and their gradients through the in-rows and the level schedule compose left behind
    check_scores(gtn, name, family, oracles)
    # ---- under a switch or in a batch == alone and plain
    if c["env"] or len(pairs) > 1:
        for e in c["env"]:
            monkeypatch.delenv(e)
        for k in range(len(pairs)):
            _, solo = compose_calls(gtn, name, pairs[k:k + 1], [(0, 1)])
            same_arrays("%s[%d] against the pair alone" % (name, k), arrays_of(solo[0]), got[k])


def check_scores_symbolic(gtn, name, oracles):
    gtn.compose_mode(cc.CASES[name]["compose_mode"])
    try:
        ops, comps = compose_calls(gtn, name)
        fs = gtn.forward_score(comps[0])
        assert fs.item() == pytest.approx(oracles[0].shortest_distance(), rel=RTOL)
    finally:
        gtn.compose_mode(0)


def test_batches_in_one_call_and_in_two_are_identical(gtn):
    """replicate/inline against replicate/grid: the same 130 pairs"""
    assert cc.expected_routes("batch/130-inline")["replicate/inline"] == 130
    assert cc.expected_routes("batch/130-in-two-calls")["replicate/grid"] == 130
    _, one = compose_calls(gtn, "batch/130-inline")
    _, two = compose_calls(gtn, "batch/130-in-two-calls")
    for k, (x, y) in enumerate(zip(one, two)):
        same_arrays("pair %d" % k, arrays_of(x), arrays_of(y))


def test_mixed_batch_elements_equal_their_solo_results(gtn):
    """the big pair sends the batch to the general variant; the small ones keep their bitmaps in LDS there"""
    name = "batch/mixed-big-and-small"
    (_, comps), routes = routed(gtn, lambda: compose_calls(gtn, name))
    assert routes.get("general/hbm") == 1 and routes.get("general/lds") == 2, routes
    pairs = cc.build(name)
    for k in (1, 2):
        (_, solo), r = routed(gtn, lambda: compose_calls(gtn, name, pairs[k:k + 1], [(0, 1)]))
        assert "fast256" in r, r      # alone it takes another kernel
        same_arrays("element %d" % k, arrays_of(solo[0]), arrays_of(comps[k]))


@pytest.mark.parametrize("off", [(True, False), (False, True), (True, True)])
def test_gradient_chunks_with_calc_grad_off(gtn, off):
    """compose_grad_kernel with a null gradient pointer on either side, over a chunk that takes the LDS window and one
    that takes direct atomics"""
    a, b = cc.build("explicit/grad-chunks")[0]
    oc = cc.oracle_products("explicit/grad-chunks")[0]
    g1, g2 = cc.to_api(gtn, a, not off[0]), cc.to_api(gtn, b, not off[1])
    comp = gtn.compose(g1, g2)
    assert comp.num_arcs() == oc.A and comp.calc_grad == (not all(off))
    deltas = cc.rng_of("grad-off").integers(-3, 4, oc.A).astype(np.float32)
    gtn.backward(comp, seed_graph(gtn, deltas))
    w1, w2 = oc.compose_grad(deltas, len(a["src"]), len(b["src"]))
    for g, w, is_off in ((g1, w1, off[0]), (g2, w2, off[1])):
        if is_off:
            assert not g.is_grad_available()
        else:
            np.testing.assert_array_equal(grads_of(g), w)


def test_fused_backward_does_not_scatter_twice(gtn):
    """forward_score of a deep FAST chain product: the narrow backward kernel scatters compose's gradient itself
    (bwd/narrow/fused) and marks the product grad_propagated; ComposeOp::backward must then add nothing.  A second
    consumer of the same product (viterbi_score) keeps the scatter in compose_grad_kernel: both ways, and their sum
    on a product with two consumers, against the oracle."""
    name = "ctc/U3-T40/cs/intersect"
    oc = cc.oracle_products(name)[0]
    a, b = cc.build(name)[0]
    A1, A2 = cc.num_arcs(a), cc.num_arcs(b)
    f1, f2 = oc.compose_grad(oc.shortest_distance_grad(False), A1, A2)
    v1, v2 = oc.compose_grad(oc.shortest_distance_grad(True), A1, A2)
    # one consumer: fused
    ops, comps = compose_calls(gtn, name)
    fs = gtn.forward_score(comps[0])
    before = gtn.debug_shortest_routes()
    gtn.backward(fs)
    after = gtn.debug_shortest_routes()
    assert after["bwd/narrow/fused"] == before["bwd/narrow/fused"] + 1
    np.testing.assert_allclose(grads_of(ops[0][0]), f1, rtol=GRAD_RTOL, atol=GRAD_ATOL)
    np.testing.assert_allclose(grads_of(ops[0][1]), f2, rtol=GRAD_RTOL, atol=GRAD_ATOL)
    # two consumers: the product's gradient is the sum, scattered once
    ops, comps = compose_calls(gtn, name)
    fs, vs = gtn.forward_score(comps[0]), gtn.viterbi_score(comps[0])
    gtn.backward(gtn.add(fs, vs))
    np.testing.assert_allclose(grads_of(ops[0][0]), f1 + v1, rtol=GRAD_RTOL, atol=2 * GRAD_ATOL)
    np.testing.assert_allclose(grads_of(ops[0][1]), f2 + v2, rtol=GRAD_RTOL, atol=2 * GRAD_ATOL)


def test_every_cell_was_counted(gtn):
    """runs last in this module: since the process started every cell a case can reach has seen a product"""
    r = gtn.debug_compose_routes()
    missing = [c for c in cc.CELLS if c not in cc.UNREACHABLE and r[c] == 0]
    if sum(r.values()) and not missing:
        print("[compose_cells] largest error per route, as a fraction of what is granted: %s" % {k: float("%.3g" % v) for k, v in WORST.items()})
    # (with -k selecting a few cases the others are legitimately missing: only judged when the whole table ran)
    if test_every_cell_was_counted.ran_all:
        assert not missing, missing
        assert r["redo/wide_chain->general"] == 0


test_every_cell_was_counted.ran_all = False


@pytest.fixture(autouse=True, scope="module")
def _note_whole_module(request):
    names = {i.name for i in request.session.items if i.fspath == request.fspath}
    test_every_cell_was_counted.ran_all = all("test_cells[%s]" % n in names for n in cc.CASES)
    yield
