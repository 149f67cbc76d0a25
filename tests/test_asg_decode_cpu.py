"""ASG decode, the parts that need no GPU: the float64 full-connect Viterbi of tests/asg_decode_fp.py (which
test_asg_decode_gpu.py judges the kernel by) is pinned to the oracle's shortest path on the lattice the reference would
build -- the emission chain composed with the transitions graph, both argument orders, transitions arc-sorted as
asgTransitions leaves them and as built -- on continuous inputs and, for the tie rule (smallest source label, smallest
final label), on integer-valued ones; the entry points exist, refuse bad arguments before they ask for a device, and fail
loudly without one."""
import ctypes
import os

import numpy as np
import pytest

from asg_decode_fp import FP_CASES, TIE_CASES, asg_decode_fp64, collapse, float32_agrees, seeded_case, tie_case
from conftest import ROOT, has_gpu
from oracle_lib import OGraph


def oracle_transitions(trans, start, sort=True):
    """examples/asg.cpp:36-47 with weights: arc i: <s> -> i (start[i]); arc N + i*N + j: j -> i (trans[i, j]);
    arc-sorted by input label as gtn::criteria::asgTransitions leaves it, or as built"""
    N = len(start)
    arcs = [(0, i + 1, i, start[i]) for i in range(N)]
    for i in range(N):
        for j in range(N):
            arcs.append((j + 1, i + 1, i, trans[i, j]))
    return OGraph.from_dict({
        "start": [1] + [0] * N, "accept": [0] + [1] * N,
        "src": [a[0] for a in arcs], "dst": [a[1] for a in arcs], "il": [a[2] for a in arcs],
        "ol": [a[2] for a in arcs], "w": [float(a[3]) for a in arcs], "sort": "i" if sort else None})


def oracle_path(em, trans, start, chain_first=True, sort=True):
    """score and labels of the reference's viterbiPath over the built lattice (shortest.cpp:190-272 over
    compose.cpp:377-522)"""
    T, N = em.shape
    e = OGraph.linear(T, N, em)
    tr = oracle_transitions(trans, start, sort)
    o = e.compose(tr) if chain_first else tr.compose(e)
    path, has = o.shortest_path()
    assert has, "every label node accepts: a path exists"
    d = o.to_dict()
    return o.shortest_distance(tropical=True), [d["il"][x] for x in path]


ORDERS = [(True, True), (False, True), (True, False), (False, False)]  # (chain first, transitions arc-sorted)


@pytest.mark.parametrize("chain_first,sort", ORDERS)
@pytest.mark.parametrize("seed,T,N,kind", TIE_CASES)
def test_fp64_viterbi_breaks_exact_ties_like_the_oracle(seed, T, N, kind, chain_first, sort):
    """integer-valued inputs (all-zero; 0/1 emissions; small-integer emissions, transitions and start), N = 2 .. 8,
    T = 1 .. 13: labels and scores == the oracle's, whichever side the chain is on, arc-sorted or not"""
    em, trans, start = tie_case(seed, T, N, kind)
    labels, score, col = asg_decode_fp64(em, trans, start)
    want_score, want = oracle_path(em, trans, start, chain_first, sort)
    assert labels.tolist() == want, (seed, T, N, kind)
    assert score == want_score  # (integers: float32 and float64 sums are both exact)
    assert col == collapse(want)


@pytest.mark.parametrize("chain_first,sort", ORDERS)
@pytest.mark.parametrize("seed,T,N", FP_CASES)
def test_fp64_viterbi_agrees_with_the_oracle(seed, T, N, chain_first, sort):
    """continuous inputs: the seeds are ones on which float32 and float64 pick the same path (a seed where rounding
    separated them would be replaced, not tolerated)"""
    em, trans, start = seeded_case(seed, T, N)
    assert float32_agrees(em, trans, start), "replace this seed"
    labels, score, col = asg_decode_fp64(em, trans, start)
    want_score, want = oracle_path(em, trans, start, chain_first, sort)
    assert labels.tolist() == want
    assert abs(score - want_score) <= 1e-5 * max(1.0, abs(want_score))
    assert col == collapse(want)


def test_fp64_viterbi_frame_counts():
    em, trans, start = seeded_case(3, 9, 5)
    full = asg_decode_fp64(em[:4], trans, start)
    labels, score, col = asg_decode_fp64(em, trans, start, frames=4)
    assert labels[:4].tolist() == full[0].tolist() and (labels[4:] == -1).all()
    assert score == full[1] and col == full[2]
    labels, score, col = asg_decode_fp64(em, trans, start, frames=0)
    assert (labels == -1).all() and score == -np.inf and col == []
    assert collapse([3, 3, 1, 1, 1, 3, 0, 0]) == [3, 1, 3, 0]


def test_entry_points_exist(gtn):
    from gtn_amd import torch_loss
    assert callable(torch_loss.asg_decode)
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    assert hasattr(lib, "gtn_asg_decode_n")
    assert callable(gtn.Batch.viterbi_decode)
    fast, fallback = gtn.debug_decode_stats()
    assert fast >= 0 and fallback >= 0


def _transitions(gtn, N):
    trans = gtn.Graph(False)
    trans.add_node(True)
    for i in range(N):
        trans.add_node(False, True)
        trans.add_arc(0, i + 1, i)
    for i in range(N):
        for j in range(N):
            trans.add_arc(j + 1, i + 1, i)
    return trans


def test_argument_errors_come_before_the_device(gtn):
    """what the arguments alone decide is refused as an invalid argument, with or without a device"""
    import torch
    from gtn_amd import torch_loss
    batch = gtn.Batch([gtn.linear_graph(2, 8)])
    trans = _transitions(gtn, 8)
    with pytest.raises(ValueError, match="row_stride"):
        batch.viterbi_decode(trans, 0)
    with pytest.raises(ValueError, match="lengths_out needs collapsed_out"):
        batch.viterbi_decode(trans, 0, lengths_out=0, row_stride=2)
    with pytest.raises(ValueError, match="one frame count per element"):
        batch.viterbi_decode(trans, 0, frames=[1, 1], row_stride=2)
    with pytest.raises(ValueError, match="null labels pointer"):
        batch.viterbi_decode(trans, 0, row_stride=2)
    with pytest.raises(ValueError, match="negative row stride"):
        batch.viterbi_decode(trans, 64, row_stride=-1)
    em = torch.zeros(2, 3, 8)
    with pytest.raises(ValueError, match="transitions must be"):
        torch_loss.asg_decode(em, torch.zeros(8, 7))
    with pytest.raises(ValueError, match="start must be"):
        torch_loss.asg_decode(em, torch.zeros(8, 8), start=torch.zeros(7))
    with pytest.raises(ValueError, match="input length outside 0 .. 3"):
        torch_loss.asg_decode(em, torch.zeros(8, 8), input_lengths=[4, 1])
    with pytest.raises(ValueError, match="input lengths for a batch of 2"):
        torch_loss.asg_decode(em, torch.zeros(8, 8), input_lengths=[1])
    with pytest.raises(ValueError, match="float32 tensor"):
        torch_loss.asg_decode(em.double(), torch.zeros(8, 8))
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        torch_loss.asg_decode(em, torch.zeros(8, 8))


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU behaviour")
def test_asg_decode_fails_loudly_without_gpu(gtn):
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    lib.gtn_asg_decode_n.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 6
    lib.gtn_asg_decode_n.restype = ctypes.c_int
    lib.gtn_criteria_last_error.restype = ctypes.c_char_p
    rc = lib.gtn_asg_decode_n(None, 1, 2, 8, None, None, None, None, None, None)
    assert rc == -1 and "no HIP device" in lib.gtn_criteria_last_error().decode()
    with pytest.raises(RuntimeError, match="no HIP device"):
        gtn.Batch([gtn.linear_graph(2, 8)]).viterbi_decode(_transitions(gtn, 8), 64, row_stride=2)
