"""The path-graph routes of Batch.viterbi_align, Batch.viterbi_decode and Batch.linear_decode where they differ: what
each makes of a best path with nodes but no arcs, which planes it fills, and that a row stride shorter than the longest
path is refused before anything is uploaded.

All values are exact: labels are integers and 0.5 + 0.25 + 1.0 = 1.75 has no rounding in float32.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
S = -7  # sentinel: a cell the call did not write


def _batch(gtn, both_empty=False):
    """g0: one node, start and accepting, no arcs (its best path has a node and no arc); g1: a chain of 3 arcs"""
    def g0():
        g = gtn.Graph(False)
        g.add_node(True, True)
        return g

    g1 = gtn.Graph(False)
    g1.add_node(True, False)
    for i, (label, w) in enumerate(zip([2, 1, 2], [0.5, 0.25, 1.0])):
        g1.add_node(False, i == 2)
        g1.add_arc(i, i + 1, label, label, w)
    return gtn.Batch([g0(), g0() if both_empty else g1])


def _loops(gtn):
    """one node, start and accepting, a self-loop i:i of weight 0 for labels 0 .. 2: not a dense transitions graph, so
    viterbi_decode takes the path-graph route"""
    g = gtn.Graph(False)
    g.add_node(True, True)
    for i in range(3):
        g.add_arc(0, 0, i, i, 0.0)
    return g


def _ints(*shape):
    import torch
    return torch.full(shape, S, dtype=torch.int32, device="cuda:0")


def _floats(n):
    import torch
    return torch.full((n,), float(S), dtype=torch.float32, device="cuda:0")


def _np(*tensors):
    return [t.cpu().numpy() for t in tensors]


def test_align_zero_arc_path(gtn):
    lab, sc = _ints(2, 5), _floats(2)
    f0, b0 = gtn.debug_align_stats()
    _batch(gtn).viterbi_align(lab, None, sc)
    gtn.synchronize()
    f1, b1 = gtn.debug_align_stats()
    lab, sc = _np(lab, sc)
    assert lab.tolist() == [[-1, -1, -1, S, S], [2, 1, 2, S, S]]
    assert sc.tolist() == [0.0, 1.75]
    assert (f1 - f0, b1 - b0) == (0, 2)


def test_align_all_paths_empty(gtn):
    lab, sc = _ints(2, 5), _floats(2)
    _batch(gtn, both_empty=True).viterbi_align(lab, None, sc)
    gtn.synchronize()
    lab, sc = _np(lab, sc)
    assert (lab == S).all()  # (rows of width 0: no label plane is copied)
    assert sc.tolist() == [0.0, 0.0]


def test_viterbi_decode_zero_arc_path(gtn):
    lab, col, ln, sc = _ints(2, 5), _ints(2, 5), _ints(2), _floats(2)
    f0, b0 = gtn.debug_decode_stats()
    _batch(gtn).viterbi_decode(_loops(gtn), lab, sc, None, col, ln)
    gtn.synchronize()
    f1, b1 = gtn.debug_decode_stats()
    lab, col, ln, sc = _np(lab, col, ln, sc)
    assert (f1 - f0, b1 - b0) == (0, 2)
    assert lab.tolist() == [[-1, -1, -1, S, S], [2, 1, 2, S, S]]
    assert col.tolist() == [[-1, -1, -1, S, S], [2, 1, 2, S, S]]
    assert ln.tolist() == [0, 3]
    assert sc[0] == -np.inf  # (not the 0.0 of viterbi_align and linear_decode)
    assert sc[1] == 1.75


def test_linear_decode_starts_plane(gtn):
    lab, col, sta, ln, sc = _ints(2, 5), _ints(2, 5), _ints(2, 5), _ints(2), _floats(2)
    f0, b0 = gtn.debug_linear_decode_stats()
    _batch(gtn).linear_decode(lab, sc, None, 1, col, sta, ln)
    gtn.synchronize()
    f1, b1 = gtn.debug_linear_decode_stats()
    lab, col, sta, ln, sc = _np(lab, col, sta, ln, sc)
    assert (f1 - f0, b1 - b0) == (0, 2)
    assert lab.tolist() == [[-1, -1, -1, S, S], [2, 1, 2, S, S]]
    assert col.tolist() == [[-1, -1, -1, S, S], [2, 2, -1, S, S]]
    assert sta.tolist() == [[-1, -1, -1, S, S], [0, 2, -1, S, S]]
    assert ln.tolist() == [0, 2]
    assert sc.tolist() == [0.0, 1.75]


@pytest.mark.parametrize("entry", ["viterbi_align", "viterbi_decode", "linear_decode"])
def test_row_stride_shorter_than_the_longest_path(gtn, entry):
    """rows of 2 entries for a path of 3 arcs: refused, and every output is still the sentinel"""
    lab, col, sta, ln, sc = _ints(2, 2), _ints(2, 2), _ints(2, 2), _ints(2), _floats(2)
    x = _batch(gtn)
    with pytest.raises(ValueError, match="shorter than the longest path"):
        if entry == "viterbi_align":
            x.viterbi_align(lab, None, sc)
        elif entry == "viterbi_decode":
            x.viterbi_decode(_loops(gtn), lab, sc, None, col, ln)
        else:
            x.linear_decode(lab, sc, None, 1, col, sta, ln)
    gtn.synchronize()
    for t in _np(lab, col, sta, ln, sc):
        assert (t == S).all()
