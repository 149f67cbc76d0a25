"""CPU half of the compose / intersect cell tests (tests/compose_cells.py, tests/test_compose_cells_gpu.py): the route
counters answer without a GPU; the case table names every cell that can be reached; every threshold has a case on
either side and the shapes really sit there; every case's product has, in the oracle, the sizes the table states; the
Python walk that stands in for the kernels' decisions reproduces the oracle's products; and the gradient case has both
kinds of chunk."""
import numpy as np
import pytest

import compose_cells as cc
from conftest import has_gpu
from oracle_lib import OGraph

ALL = list(cc.CASES)
SMALL_EXPLICIT = [n for n in ALL if n.startswith(("eps/", "pairs-pref/", "explicit/fast", "device-built/product"))]


def test_route_counters_answer_without_a_gpu(gtn):
    r = gtn.debug_compose_routes()
    assert list(r) == cc.CELLS and all(isinstance(v, int) and v >= 0 for v in r.values())
    if not has_gpu():
        g = gtn.linear_graph(2, 2)
        with pytest.raises(RuntimeError):
            gtn.compose(g, g)
        assert gtn.debug_compose_routes() == r and all(v == 0 for v in r.values())


def test_the_table_names_every_cell():
    """... but the one no input can reach (compose_cells.UNREACHABLE says why)"""
    named = set()
    for n in ALL:
        named |= set(cc.expected_routes(n))
    assert named == set(cc.CELLS) - cc.UNREACHABLE, set(cc.CELLS) ^ named


@pytest.mark.parametrize("name", ALL)
def test_case_is_what_the_table_states(name):
    """the oracle's product sizes, emptiness, the cells the case was designed for; and the walk agrees with the oracle"""
    c = cc.CASES[name]
    sizes = [(o.N, o.A) for o in cc.oracle_products(name)]
    assert sizes == [tuple(s) for s in c["sizes"]], sizes[:4]
    if "empty" in name or name.startswith(("degenerate/T0", "degenerate/no-", "degenerate/labels", "ctc/U3-T1", "ctc/U3-T2")):
        assert all(s == (0, 0) for s in sizes)
    else:
        assert all(a > 0 for _, a in sizes), sizes
    want = cc.expected_routes(name)
    assert c["cells"] <= set(want), c["cells"] - set(want)
    pairs = cc.build(name)
    detail = []
    cc.predict(pairs[slice(*cc.calls_of(name)[0])], c["mode"], c["env"], detail)
    for d, s in zip(detail, sizes):
        assert (d["walk"].N, d["walk"].A) == s


@pytest.mark.parametrize("name", SMALL_EXPLICIT)
def test_walk_reproduces_the_oracle_arc_for_arc(name):
    """sim_pairs is compose.hip's walk in Python: node ids, arc order and the input arcs behind every product arc"""
    for a, b in cc.build(name):
        w = cc.sim_pairs(cc.Facts(a), cc.Facts(b), False)
        oc = cc.to_oracle(a).compose(cc.to_oracle(b))
        _, _, src, dst, _, _, _ = cc.oracle_arrays(oc)
        assert [x[0] for x in w.arcs] == src.tolist() and [x[1] for x in w.arcs] == dst.tolist()
        assert [[x[2], x[3]] for x in w.arcs] == oc.grad_info().tolist()


def test_every_threshold_has_a_case_on_either_side():
    for what, (lo, hi) in cc.THRESHOLDS.items():
        assert lo in cc.CASES and hi in cc.CASES, what
        assert cc.expected_routes(lo) != cc.expected_routes(hi), what
    for what, (lo, hi) in cc.SAME_ROUTE_EDGES.items():
        assert cc.expected_routes(lo) == cc.expected_routes(hi) and "bitmap/classic" in cc.expected_routes(lo), what
        assert [cc.build(n)[0][0]["chain"][0] for n in (lo, hi)] == [1, 2] and cc.CASES[lo]["env"] == ("GTNX_CLASSIC_BITMAPS",)

    def detail(name):
        d = []
        c = cc.CASES[name]
        cc.predict(cc.build(name)[slice(*cc.calls_of(name)[0])], c["mode"], c["env"], d)
        return d[0]

    def partner(name):
        a, b = cc.build(name)[0]
        return cc.Facts(b if cc.is_chain(a) else a)

    for side in ("cf", "cs"):
        for mode in ("compose", "intersect"):
            v = "/%s/%s" % (side, mode)
            # KC = 4 candidates, out- and in-lists
            assert [max(len(o) for o in partner("degree/out-%d%s" % (k, v)).out) for k in (4, 5)] == [4, 5]
            assert [max(len(i) for i in partner("degree/in-%d%s" % (k, v)).inn) for k in (4, 5)] == [4, 5]
            assert max(len(o) for o in partner("degree/out-5-one-beyond-C" + v).out) == 5
            assert detail("degree/out-4" + v)["handback"] is None and detail("degree/out-5-one-beyond-C" + v)["handback"] is None
            assert detail("degree/out-5" + v)["handback"].startswith("F") and detail("degree/in-5" + v)["handback"].startswith("B")
            # 3/4 of the claim hash, and A <= 768 / 1536 for the deferred sizes
            for blk, lo, hi in ((256, 768, 769), (512, 1536, 1537)):
                dl, dh = detail("level-arcs/%dx%d%s" % (blk, lo, v)), detail("level-arcs/%dx%d%s" % (blk, hi, v))
                assert (dl["walk"].level_arcs_max, dh["walk"].level_arcs_max) == (lo, hi) == (3 * blk, 3 * blk + 1)
                assert dl["defer"] and not dh["defer"] and dl["handback"] is None and dh["handback"].startswith("F")
                assert (dl["wide"], dh["wide"]) == (blk == 512, blk == 512)
                assert partner("level-arcs/%dx%d%s" % (blk, hi, v)).max_deg <= 4      # only the A rule keeps the sizes back
            # partner widths
            for No in (256, 257, 512, 513, 1024, 1025):
                d = detail("strands/%d%s" % (No, v))
                assert partner("strands/%d%s" % (No, v)).N == No and d["walk"].width_max == No
                assert d["wide"] == (256 < No <= 512) and d["skip"] == (No <= 512)
                assert (d["slices"] > 0) == (No <= 1024) and d["handback"] is None
            assert not detail("strands/257/narrow" + v)["wide"]
            # compose_wide_node_cap()
            assert [partner("wide/%d%s" % (No, v)).N for No in (2048, 2049)] == [2048, 2049] == [cc.WIDE_NODE_CAP, cc.WIDE_NODE_CAP + 1]
            assert all(partner("wide/%d%s" % (No, v)).A > 4 * No for No in (2048, 2049))
            # the classic budget of a chain product, windows shorter than the chain, never-stationary partners
            assert 1025 * 6 <= 212992 < 1025 * 209 and not detail("strands/1025-T208" + v)["classic_ok"]
            for n, room, slices in (("window/ctc-U2-T13400", 13309, 69), ("window/strands-512-T700", 669, 576),
                                    ("ring/3x3-T13400", 13309, 67)):
                d = detail(n + v)
                assert not d["full_window"] and d["slices"] == slices and room < cc.build(n + v)[0][0 if side == "cf" else 1]["chain"][0] + 1
            assert detail("window/ctc-U2-T13400" + v)["handback"] is None and detail("window/strands-512-T700" + v)["wide"]
            assert detail("ring/3x3-T13400" + v)["handback"] == "B: chs >= Wmax"
            assert not detail("ring/3x3-T8" + v)["walk"].stationary and detail("ring/3x3-T8" + v)["handback"] is None
            assert not detail("ring/3x3-T13400" + v)["walk"].stationary and detail("window/ctc-U2-T13400" + v)["walk"].stationary
    # the classic budget of two explicit graphs: 2 * 4 * ceil(N1 N2 / 32) against 53248 bytes
    assert cc.bitmap_budget(256) == 53248 and cc.bitmap_budget(512) == 43008
    assert 8 * ((416 * 512 + 31) // 32) == 53248 and 8 * ((417 * 512 + 31) // 32) > 53248
    for n, (n1, n2) in (("budget/416x512", (416, 512)), ("budget/417x512", (417, 512)), ("budget/470x470", (470, 470))):
        a, b = cc.build(n)[0]
        assert (len(a["start"]), len(b["start"]), len(a["src"]), len(b["src"])) == (n1, n2, 3 * n1, 3 * n2)
    # the transpose pass of the big pairs scans more than one 2048-node chunk
    assert all(s[0][0] > 2 * 2048 for s in (cc.CASES[n]["sizes"] for n in ("budget/417x512", "budget/470x470")))
    # pairs_pref: A against 4 N, every matcher
    for m in cc.SORTS:
        (a, _), (b, _) = cc.build("pairs-pref/%s/4N" % m)[0], cc.build("pairs-pref/%s/4N+1" % m)[0]
        assert (len(a["src"]), len(b["src"])) == (4 * 12, 4 * 12 + 1) and len(a["start"]) == len(b["start"]) == 12
        assert "pairs" in cc.expected_routes("pairs-pref/%s/4N+1" % m) and "pairs" not in cc.expected_routes("pairs-pref/%s/4N" % m)
    # more than 128 pairs in one call
    assert len(cc.build("batch/130-inline")) == 130 and [hi - lo for lo, hi in cc.calls_of("batch/130-in-two-calls")] == [65, 65]
    # g1's LDS cache: on for a small g1, off when its records do not fit beside the bitmaps
    a, b = cc.build("explicit/grad-chunks")[0]
    assert cc.g1_cache_bytes(len(a["start"]), len(a["src"])) > cc.lds_budget(256)
    assert "g1_cache/on" in cc.expected_routes("explicit/fast-cache-on") and "g1_cache/off" in cc.expected_routes("explicit/grad-chunks")


def test_epsilon_cases_reach_the_accept_rule():
    """epsilons on the matched side of g1, of g2, of both; in the `both` cases some product node has epsilon_matched
    set with compose.cpp:461 holding g1's epsilon arcs back, and some node with :476 holding g2's back"""
    for m in cc.SORTS:
        for variant, gone in (("fast", False), ("general", True)):
            for where in ("g1", "g2", "both"):
                a, b = cc.build("eps/%s/%s/%s" % (m, where, variant))[0]
                assert ((np.asarray(a["ol"]) == cc.EPS).any(), (np.asarray(b["il"]) == cc.EPS).any()) == (where != "g2", where != "g1")
                w = cc.sim_pairs(cc.Facts(a), cc.Facts(b), False)
                assert bool(w.handback) == gone
                if where == "both":
                    n461, n476 = cc.eps_deciders(a, b, w)
                    assert n461 > 0 and n476 > 0


def test_gradient_case_has_both_kinds_of_chunk():
    """compose_grad_kernel: 4096 product arcs per workgroup, an LDS window while the chunk's input arcs span less than 4096
    ids, direct atomics otherwise"""
    a, b = cc.build("explicit/grad-chunks")[0]
    assert len(a["src"]) >= 6000
    gi = cc.oracle_products("explicit/grad-chunks")[0].grad_info()
    spans = []
    for k0 in range(0, len(gi), 4096):
        ids = gi[k0:k0 + 4096, 0]
        spans.append(int(ids.max() - ids.min()))
    assert len(spans) == 2 and spans[0] >= 4096 and spans[1] < 4096, spans
    assert int(gi[:, 1].max() - gi[:, 1].min()) < 4096


def test_mixed_batch_keeps_the_small_pairs_in_lds():
    detail = []
    cc.predict(cc.build("batch/mixed-big-and-small"), "compose", (), detail)
    assert [d["first"] for d in detail] == [0, 0, 0] and [d["classic_ok"] for d in detail] == [False, True, True]
    assert cc.expected_routes("batch/mixed-big-and-small")["general/lds"] == 2
