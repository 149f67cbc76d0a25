"""CPU half of the built-graph shortest-distance cell tests (tests/shortest_fp.py, tests/test_shortest_cells_gpu.py):
the float64 host form is pinned to the oracle (and thereby to the reference), every GPU case vets, is trim and lands --
by the replica of the host's dispatch -- in the cell it names, every tie case really ties, the case lists together name
every cell the GPU suite has to reach, and the route counters answer without a GPU."""
import time

import numpy as np
import pytest

import rational_fp
import shortest_fp as sf
from conftest import has_gpu
from oracle_lib import OGraph

ALL_TABLES = (sf.GENERIC, sf.TIES, sf.DEEP, sf.NARROW, sf.BATCHES)
ALL_CASES = [n for t in ALL_TABLES for n in t]


def graphs_of(name):
    g = sf.build(name)
    return g if isinstance(g, list) else [g]


@pytest.mark.parametrize("name", ["g8/5x37/x16=64", "g256/9x2", "g8/starts-with-in-arcs", "deep/P=130", "deep/P=65",
                                  "narrow/levels=32"])
def test_float64_form_against_the_oracle(name):
    """the gates tests/test_rational_cpu.py uses for the same yardstick: scores rel = abs = 1e-5, gradients rtol 1e-4,
    atol 1e-5; the best path of a vetted case arc for arc"""
    g = sf.build(name)
    og = OGraph.from_dict(sf.as_lists(g))
    log = sf.sweep(g, np.float64)
    assert float(log["score"]) == pytest.approx(og.shortest_distance(), rel=1e-5, abs=1e-5)
    np.testing.assert_allclose(log["grad"], og.shortest_distance_grad(), rtol=1e-4, atol=1e-5)
    trop = sf.sweep(g, np.float64, True)
    assert float(trop["score"]) == pytest.approx(og.shortest_distance(True), rel=1e-5, abs=1e-5)
    # ... and in step with the suite's other float64 recursion (tests/rational_fp.py: score_and_grad)
    rg = rational_fp.graph(g["start"], g["accept"], g["src"], g["dst"], g["il"], g["ol"], g["w"])
    s2, g2 = rational_fp.score_and_grad(rg)
    assert float(log["score"]) == pytest.approx(s2, rel=1e-12)
    np.testing.assert_allclose(log["grad"], g2, rtol=1e-9, atol=1e-300)
    s3, g3 = rational_fp.score_and_grad(rg, tropical=True)
    assert float(trop["score"]) == s3 and (trop["grad"] == g3).all()
    if name in sf.GENERIC:
        np.testing.assert_array_equal(trop["grad"], og.shortest_distance_grad(True))
        assert trop["path"] == og.shortest_path()[0]


@pytest.mark.parametrize("name", list(sf.GENERIC) + list(sf.BATCHES))
def test_every_tropical_case_vets(name):
    for i, g in enumerate(graphs_of(name)):
        y = sf.case_yardstick(name, i if name in sf.BATCHES else None)
        assert y["vet"] is None, (name, i, y["vet"])
        assert len(y["trop_path"]) > 0 and np.isfinite(y["score"])


@pytest.mark.parametrize("name", list(sf.TIES))
def test_tie_cases_tie(name):
    g = sf.build(name)
    assert (g["w"] == np.round(g["w"])).all() and g["w"].min() == -2 and g["w"].max() == 1
    node_ties, on_best_path, accept_ties, slot_is_not_arc_order = sf.tie_census(g)
    assert node_ties >= 1 and on_best_path >= 1 and accept_ties >= 2, (node_ties, on_best_path, accept_ties)
    if g["sort"] == "i":
        # arc_sort really reorders the lists: labels are a permutation of the arc ids, no in-list of two or more arcs
        # that is in arc-id order by chance is relied on, and at some tied node the first best candidate of the row
        # is not the one with the smallest arc id -- ranking by slot and ranking by arc id give different answers
        assert sorted(g["il"].tolist()) == list(range(g["src"].size)) and (g["il"] != np.arange(g["src"].size)).any()
        rows = [r for r in sf.in_lists_as_built(g) if r.size >= 2]
        assert sum(1 for r in rows if (np.diff(r) < 0).any()) > len(rows) // 2
        assert slot_is_not_arc_order >= 1
        twin = sf.build(name.replace("sorted", "unsorted"))
        assert (twin["src"] == g["src"]).all() and (twin["w"] == g["w"]).all() and (twin["il"] != g["il"]).any()
    else:
        assert slot_is_not_arc_order == 0 and (g["il"] == np.arange(g["src"].size)).all()
    assert int(g["accept"].sum()) >= 3 and np.diff(g["level_off"]).min() >= 3  # multi-node levels, several accept nodes


@pytest.mark.parametrize("name", ALL_CASES)
def test_case_is_trim_and_lands_in_the_cell_it_names(name):
    gs = graphs_of(name)
    for g in gs:
        assert sf.is_trim(g)
    for no_deep in ((False, True) if name in sf.DEEP else (False,)):
        want = sf.expected_cells(name, no_deep)
        for what, cell in want.items():
            assert sf.predict(gs, what, no_deep) == cell, (name, what, no_deep)


def test_threshold_pairs_and_coverage():
    """every threshold pair lands on two different cells, and the lists name every generic cell, both deep cells and
    the host-built narrow forward cell"""
    pairs = [("g8/5x37/x16=64", "g8/5x37/x16=63"), ("g64/5x37/x16=384", "g64/5x37/x16=383"),
             ("g256/4x5/x16=3072", "g256/4x5/x16=3071"), ("deep/P=64", "deep/P=63"), ("deep/P=24576", "deep/P=24577"),
             ("narrow/levels=32", "narrow/levels=31"), ("narrow/width=1024", "narrow/width=1025"),
             ("narrow/level-arcs=2048", "narrow/level-arcs=2049"), ("narrow/reach=4096", "narrow/reach=4097"),
             ("narrow/A=16N", "narrow/A=16N+1")]
    for a, b in pairs:
        assert sf.expected_cells(a)["fwd_log"] != sf.expected_cells(b)["fwd_log"], (a, b)
    x16 = lambda n: (sf.sched_stats(sf.build(n)).n_in * 16) // sf.sched_stats(sf.build(n)).P
    assert [x16(n) for n in ("g8/5x37/x16=64", "g8/5x37/x16=63", "g64/5x37/x16=384", "g64/5x37/x16=383",
                             "g256/4x5/x16=3072", "g256/4x5/x16=3071")] == [64, 63, 384, 383, 3072, 3071]
    named = set()
    for n in ALL_CASES:
        named |= set(sf.expected_cells(n).values())
        if n in sf.DEEP:
            named |= set(sf.expected_cells(n, True).values())
    need = {"fwd/deep", "bwd/deep", "fwd/narrow/log"}
    for G in (1, 8, 64, 256):
        need |= set(sf.generic_cells(G).values())
    assert need <= named, need - named


def test_shapes_reach_the_edges_they_name():
    deg = lambda g: np.bincount(g["dst"], minlength=g["start"].size)
    odeg = lambda g: np.bincount(g["src"], minlength=g["start"].size)
    for d in (64, 65, 2048, 2049):
        assert deg(sf.build("deep/in-hub-%d" % d))[2150] == d
        assert odeg(sf.build("deep/out-hub-%d" % d))[2150] == d
    assert deg(sf.build("deep/in-hubs-2x1100"))[2150:2152].tolist() == [1100, 1100]
    assert odeg(sf.build("deep/out-hubs-2x1100"))[2150:2152].tolist() == [1100, 1100]
    g = sf.build("deep/130-accepts-3-starts")
    assert int(g["accept"].sum()) == 130 and np.flatnonzero(g["start"]).tolist() == [0, 1, 2150]
    for G in (1, 8, 64, 256):
        g = sf.build("g%d/300-accepts" % G)
        a32 = sf.sweep(g, np.float32, True)["alpha"]
        dead = g["dead_accepts"]
        assert int(g["accept"].sum()) == 300 and dead.size == 100 and np.isneginf(a32[dead]).all()
        live = sf.build("g%d/300-live-accepts" % G)
        assert int(live["accept"].sum()) == 300 and np.isfinite(sf.sweep(live, np.float32, True)["alpha"]).all()
        g = sf.build("g%d/starts-with-in-arcs" % G)
        st = np.flatnonzero(g["start"])
        assert (deg(g)[st] > 0).sum() == 2
        g = sf.build("g%d/neg-inf-arc" % G)
        bad = np.flatnonzero(np.isneginf(g["w"]))
        assert bad.size == 1 and bad[0] not in sf.case_yardstick("g%d/neg-inf-arc" % G)["trop_path"]
    assert sorted(set(deg(sf.build("g64/7x5/deg24-65-191"))[5:].tolist())) == [24, 65, 191]
    for w in (1, 2, 3):
        g = sf.build("g256/9x%d" % w)
        assert sorted(set(deg(g)[w:].tolist())) == [192, 257, 300, 513] and sf.sched_stats(g).max_width == w
    s = {n: sf.sched_stats(sf.build(n)) for n in sf.NARROW}
    assert (s["narrow/width=1024"].max_width, s["narrow/width=1025"].max_width) == (1024, 1025)
    assert (s["narrow/level-arcs=2048"].max_level_arcs, s["narrow/level-arcs=2049"].max_level_arcs) == (2048, 2049)
    assert [s["narrow/reach=%d" % r].max_reach for r in (4096, 4097, 2048, 2049)] == [4096, 4097, 2048, 2049]
    assert (s["narrow/A=16N"].A, s["narrow/A=16N+1"].A) == (16 * 256, 16 * 256 + 1)


def test_all_cases_and_yardsticks_build_quickly():
    """(mostly cached by now; from cold it is a few seconds)"""
    t0 = time.time()
    for name in ALL_CASES:
        for i, _ in enumerate(graphs_of(name)):
            if name not in sf.TIES:
                sf.case_yardstick(name, i if name in sf.BATCHES else None)
    assert time.time() - t0 < 60.0


def test_route_counters_answer_without_a_gpu(gtn):
    r = gtn.debug_shortest_routes()
    need = {"fwd/deep", "bwd/deep", "fwd/narrow/log", "fwd/narrow/log/inw", "bwd/narrow", "bwd/narrow/fused"}
    for G in (1, 8, 64, 256):
        need |= set(sf.generic_cells(G).values())
    assert need <= set(r) and len(r) == 28 and all(isinstance(v, int) and v >= 0 for v in r.values())
    if not has_gpu():
        g = gtn.Graph()
        g.add_node(True)
        g.add_node(False, True)
        g.add_arc(0, 1, 0)
        with pytest.raises(RuntimeError):
            gtn.forward_score(g)
        assert gtn.debug_shortest_routes() == r
        assert all(v == 0 for v in r.values())
