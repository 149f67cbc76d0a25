"""Forced alignment, the parts that need no GPU: the float64 trellis Viterbi of tests/ctc_align_fp.py (which
test_align_gpu.py judges the torch entry point by) agrees with the oracle's shortest path on the built lattice for
the seeded float cases that test uses; the Python entry points exist and fail loudly without a device."""
import numpy as np
import pytest

import graphgen as gg
from conftest import has_gpu
from ctc_align_fp import FP_CASES, ctc_align_fp64, min_frames, seeded_case
from oracle_lib import OGraph


def oracle_path(em, target, blank=0, chain_first=False):
    """score and labels of the reference's viterbiPath over the built lattice (shortest.cpp:190-272 over
    compose.cpp:377-522); (None, None) when no accepting path exists"""
    T, C = em.shape
    a = OGraph.from_dict(gg.ctc_target_graph(list(target), blank))
    b = OGraph.linear(T, C, em)
    o = b.compose(a, "compose") if chain_first else a.compose(b, "intersect")
    arcs, has = o.shortest_path()
    if not has:
        return None, None
    d = o.to_dict()
    return o.shortest_distance(tropical=True), [d["il"][x] for x in arcs]


@pytest.mark.parametrize("seed,B,T,C,Umax,ragged", FP_CASES)
def test_fp64_trellis_viterbi_agrees_with_the_oracle(seed, B, T, C, Umax, ragged):
    em, targets, frames = seeded_case(seed, B, T, C, Umax, ragged)
    for b in range(B):
        f = int(frames[b])
        assert f >= min_frames(targets[b])
        labels, tokens, score = ctc_align_fp64(em[b], targets[b], 0, f)
        want_score, want = oracle_path(em[b, :f], targets[b])
        assert want is not None
        assert labels[:f].tolist() == want
        assert (labels[f:] == -1).all() and (tokens[f:] == -1).all()
        assert abs(score - want_score) <= 1e-5 * max(1.0, abs(want_score))
        tk = tokens[:f]
        on = tk >= 0
        assert (labels[:f][on] == np.asarray(targets[b])[tk[on]]).all() and (labels[:f][~on] == 0).all()
        steps = np.diff(tk[on])
        assert ((steps == 0) | (steps == 1)).all() and sorted(set(tk[on].tolist())) == list(range(len(targets[b])))


def test_fp64_trellis_viterbi_infeasible():
    em = np.zeros((3, 5), np.float32)
    labels, tokens, score = ctc_align_fp64(em, [1, 1, 2])  # needs four frames
    assert score == -np.inf and (labels == -1).all() and (tokens == -1).all()
    assert oracle_path(em, [1, 1, 2]) == (None, None)


def test_entry_points_exist(gtn):
    from gtn_amd import torch_loss
    assert callable(gtn.Batch.viterbi_align)
    assert callable(torch_loss.ctc_forced_align)
    fast, fallback = gtn.debug_align_stats()
    assert fast >= 0 and fallback >= 0


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU behaviour")
def test_align_fails_loudly_without_gpu(gtn):
    g = gtn.linear_graph(2, 2)
    with pytest.raises(RuntimeError, match="no HIP device"):
        gtn.Batch([g]).viterbi_align(0, row_stride=2)
    with pytest.raises(RuntimeError, match="no HIP device"):
        gtn.Batch.ctc_targets([[1]])
