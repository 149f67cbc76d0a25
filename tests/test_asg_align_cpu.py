"""ASG forced alignment, the parts that need no GPU: the float64 trellis Viterbi of tests/asg_align_fp.py (which
test_asg_align_gpu.py judges the kernel by) is pinned to the oracle's shortest path on the lattice the reference would
build -- compose(forceAlign(target), transitions) composed with the emission chain, both argument orders, transitions
arc-sorted as asgTransitions does -- on continuous inputs and, for the tie rule (the step wins), on integer-valued
ones; the entry points exist and fail loudly without a device."""
import ctypes
import os

import numpy as np
import pytest

from asg_align_fp import FP_CASES, TIE_CASES, asg_align_fp64, seeded_case, tie_case, tokens_from_labels
from conftest import ROOT, has_gpu
from oracle_lib import OGraph


def _graph(n_nodes, start, accept, arcs, sort=None):
    return OGraph.from_dict({
        "start": [int(i in start) for i in range(n_nodes)], "accept": [int(i in accept) for i in range(n_nodes)],
        "src": [a[0] for a in arcs], "dst": [a[1] for a in arcs], "il": [a[2] for a in arcs],
        "ol": [a[2] for a in arcs], "w": [float(a[3]) for a in arcs], "sort": sort})


def oracle_transitions(trans, start, sort=True):
    """examples/asg.cpp:36-47 with weights: arc i: <s> -> i (start[i]); arc N + i*N + j: j -> i (trans[i, j]);
    arc-sorted by input label as gtn::criteria::asgTransitions leaves it"""
    N = len(start)
    arcs = [(0, i + 1, i, start[i]) for i in range(N)]
    for i in range(N):
        for j in range(N):
            arcs.append((j + 1, i + 1, i, trans[i, j]))
    return _graph(N + 1, {0}, set(range(1, N + 1)), arcs, "i" if sort else None)


def oracle_path(em, trans, start, target, chain_first=False, sort=True):
    """score and labels of the reference's viterbiPath over the built lattice (shortest.cpp:190-272 over
    compose.cpp:377-522); (None, None) when no accepting path exists"""
    T, N = em.shape
    U = len(target)
    arcs = []
    for l in range(1, U + 1):
        arcs.append((l - 1, l, int(target[l - 1]), 0.0))
        arcs.append((l, l, int(target[l - 1]), 0.0))
    ft = _graph(U + 1, {0}, {U}, arcs).compose(oracle_transitions(trans, start, sort))
    e = OGraph.linear(T, N, em)
    o = e.compose(ft) if chain_first else ft.compose(e)
    path, has = o.shortest_path()
    if not has:
        return None, None
    d = o.to_dict()
    return o.shortest_distance(tropical=True), [d["il"][x] for x in path]


def _check_against_oracle(em, trans, start, target, frames, chain_first, sort, exact_score):
    f = int(frames)
    labels, tokens, score = asg_align_fp64(em, trans, start, target, f)
    want_score, want = oracle_path(em[:f], trans, start, target, chain_first, sort)
    assert want is not None, "every case is feasible"
    assert labels[:f].tolist() == want, (target, f, chain_first, sort)
    assert (labels[f:] == -1).all() and (tokens[f:] == -1).all()
    if exact_score:
        assert score == want_score  # (integers: float32 and float64 sums are both exact)
    else:
        assert abs(score - want_score) <= 1e-5 * max(1.0, abs(want_score))
    tk = tokens[:f]
    assert (labels[:f] == np.asarray(target)[tk]).all()
    steps = np.diff(tk)
    assert tk[0] == 0 and tk[-1] == len(target) - 1 and ((steps == 0) | (steps == 1)).all()
    determined = tokens_from_labels(want, target)
    if determined is not None:
        assert tk.tolist() == determined


@pytest.mark.parametrize("chain_first", [False, True])
@pytest.mark.parametrize("seed,B,T,N,Umax,ragged", FP_CASES)
def test_fp64_trellis_viterbi_agrees_with_the_oracle(seed, B, T, N, Umax, ragged, chain_first):
    """continuous inputs: the seeds are ones on which the oracle (float32) and float64 pick the same path on every
    utterance (a seed where rounding separated them would be replaced, not tolerated)"""
    em, trans, start, targets, frames = seeded_case(seed, B, T, N, Umax, ragged)
    for b in range(B):
        _check_against_oracle(em[b], trans, start, targets[b], frames[b], chain_first, True, False)


@pytest.mark.parametrize("chain_first,sort", [(False, True), (True, True), (False, False), (True, False)])
@pytest.mark.parametrize("seed,B,Tmax,Umax,nlab,rep,kind", TIE_CASES)
def test_step_wins_exact_ties_like_the_oracle(seed, B, Tmax, Umax, nlab, rep, kind, chain_first, sort):
    """integer-valued inputs (all-zero weights; 0/1 emissions; small-integer emissions, transitions and start
    weights), U up to 40, T up to 60, 2-8 labels, up to 70 % repeated labels: the fp64 path with the step-wins rule
    is the oracle's path, whichever side the chain is on and whether or not the transitions are arc-sorted"""
    utts, trans, start = tie_case(seed, B, Tmax, Umax, nlab, rep, kind)
    for em, target in utts:
        _check_against_oracle(em, trans, start, target, em.shape[0], chain_first, sort, True)


def test_fp64_trellis_viterbi_infeasible():
    em = np.zeros((3, 5), np.float32)
    trans, start = np.zeros((5, 5), np.float32), np.zeros(5, np.float32)
    labels, tokens, score = asg_align_fp64(em, trans, start, [1, 1, 2, 0])  # needs four frames
    assert score == -np.inf and (labels == -1).all() and (tokens == -1).all()
    assert oracle_path(em, trans, start, [1, 1, 2, 0]) == (None, None)
    labels, tokens, score = asg_align_fp64(em, trans, start, [1, 1, 2], frames=2)
    assert score == -np.inf and (labels == -1).all() and (tokens == -1).all()
    labels, tokens, score = asg_align_fp64(em, trans, start, [])  # no labels, three frames
    assert score == -np.inf and (labels == -1).all()
    assert oracle_path(em, trans, start, []) == (None, None)


def test_entry_points_exist(gtn):
    from gtn_amd import torch_loss
    assert callable(torch_loss.asg_forced_align)
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    assert hasattr(lib, "gtn_asg_align_n")
    assert callable(gtn.Batch.asg_force_align) and callable(gtn.Batch.viterbi_align)


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU behaviour")
def test_asg_align_fails_loudly_without_gpu(gtn):
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    lib.gtn_asg_align_n.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 5
    lib.gtn_asg_align_n.restype = ctypes.c_int
    lib.gtn_criteria_last_error.restype = ctypes.c_char_p
    tg, ln = np.array([1], np.int32), np.array([1], np.int32)
    rc = lib.gtn_asg_align_n(None, tg.ctypes.data, ln.ctypes.data, 1, 2, 4, None, None, None, None, None)
    assert rc == -1 and "no HIP device" in lib.gtn_criteria_last_error().decode()
    N = 4
    trans = gtn.Graph(False)
    trans.add_node(True)
    for i in range(N):
        trans.add_node(False, True)
        trans.add_arc(0, i + 1, i)
    for i in range(N):
        for j in range(N):
            trans.add_arc(j + 1, i + 1, i)
    with pytest.raises(RuntimeError, match="no HIP device"):
        gtn.Batch.asg_force_align([[1]], trans, N)
