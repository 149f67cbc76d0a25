"""ASG Viterbi alignment of token lattices, the parts that need no GPU.  The float32 transcription of
tests/asg_lattice_align_fp.py (which test_asg_lattice_align_gpu.py compares the kernel with bit for bit) is pinned to the
plain reference -- the float64 maximum over the lattice's enumerated paths of w(p) + the best ASG alignment of labels(p)
-- to the no-path rule and to asg_token_align_fp on a chain; the entry points exist in every layer."""
import ctypes
import itertools
import os

import numpy as np
import pytest

import asg_lattice_align_fp as fp
import asg_lattice_fp as afp
import asg_token_align_fp as tfp
from conftest import ROOT
from ctc_lattice_fp import chain_lattice, paths_of

NEG = -np.inf
GATE = afp.SCORE_GATE


def best64(em, table, lat, T):
    """the float64 maximum over the lattice's paths of w(p) + the best alignment of labels(p) under em[:T]"""
    if lat is None or T == 0:
        return NEG
    src, dst, lab, w, K = lat
    zs = [float(np.sum(w[p])) + tfp.align_pair64(em[:T], table, lab[p], len(p), T)[0]
          for p in paths_of(src, dst, K) if 0 < len(p) <= T and np.sum(w[p]) > NEG]
    return max([z for z in zs if z > NEG], default=NEG)


def first_wins(em, table, lat, T):
    """the (path, starts) the tie rule picks among ALL (path, spans) pairs of a small lattice, scored one by one in
    float64 (exact on integers): of the maxima the one whose frame arcs, read from the last frame down, come first --
    the lowest end arc, then per frame the arc itself before the arcs entering its src ascending"""
    src, dst, lab, w, K = lat
    pairs = []
    for p in paths_of(src, dst, K):
        for cut in itertools.combinations(range(1, T), len(p) - 1) if 0 < len(p) <= T else ():
            starts = (0,) + cut
            z = fp.rescore64(em[:T], table, lat, p, starts, cut + (T,))
            frame = np.repeat(p, np.diff(starts + (T,)))[::-1]
            key = (frame[0],) + tuple(0 if a == b else 1 + a for a, b in zip(frame[1:], frame[:-1]))
            pairs.append((-z, key, p, starts))
    return min(pairs)[2:] if pairs and min(pairs)[0] < -NEG else None


@pytest.mark.parametrize("li", range(len(fp.TIE_LATTICES)))
def test_ties_have_the_exact_optimum_and_the_first_wins_path(li):
    _, arcs, K, weights = fp.TIE_LATTICES[li]
    a, w = fp.sort_by_dst(arcs, weights)
    lat = afp.lattice_of(a, len(a), K, w, fp.TIE_C, 4096)
    table = afp.table_of(*fp.tie_table(li)[::-1])
    for T in fp.TIE_FRAMES:
        em = fp.tie_em("small", 5 * li + T)
        want = first_wins(em, table, lat, T)
        for dtype in (np.float32, np.float64):
            r = fp.align_lattice(em, table, lat, T, 8, dtype)
            assert float(r.score) == best64(em, table, lat, T)  # (exactly)
            n = r.path_len
            assert (want is None) == (n == 0)
            if n:
                assert (list(r.path_arcs[:n]), tuple(r.starts[:n])) == (list(want[0]), want[1])
                assert fp.rescore64(em[:T], table, lat, r.path_arcs[:n], r.starts[:n], r.ends[:n]) == float(r.score)


@pytest.mark.parametrize("name", ["s64", "edges", "ragged"])
def test_continuous_cases_reach_the_float64_optimum(name):
    c = afp.case(name)
    table = afp.table_of(c.start, c.trans)
    r = fp.result(name)
    for b in range(len(c.num_arcs)):  # (every utterance)
        T = c.em.shape[1] if c.frames is None else c.frames[b]
        lat = afp.lattice_for(c, b)
        want = best64(c.em[b], table, lat, T)
        n = r.path_len[b]
        assert (n == 0) == (want == NEG) == (r.scores[b] == NEG), b
        if n:
            z = fp.rescore64(c.em[b, :T], table, lat, r.path_arcs[b, :n], r.starts[b, :n], r.ends[b, :n])
            tol = GATE * max(1.0, abs(want))
            assert abs(float(r.scores[b]) - want) <= tol and abs(z - want) <= tol, b
            assert (r.path_tokens[b, :n] == lat[2][r.path_arcs[b, :n]]).all()
            assert (r.frame_arcs[b, :T] == np.repeat(r.path_arcs[b, :n], r.ends[b, :n] - r.starts[b, :n])).all()


@pytest.mark.parametrize("name", ["edges", "ragged", "sausage-capped"])
def test_no_path_exactly_where_the_score_is_minus_infinity(name):
    c = afp.case(name)
    r = fp.evaluate(c, P=4)
    dead = afp.result(name).scores == NEG
    assert dead.any() and not dead.all()
    assert ((r.scores == NEG) == dead).all() and ((r.path_len == 0) == dead).all()
    assert all((rows[dead] == -1).all() for rows in (r.path_arcs, r.path_tokens, r.starts, r.ends, r.frame_arcs))
    assert (r.token_scores[dead] == NEG).all() and (r.path_len[~dead] >= 1).all() and (r.starts[~dead, 0] == 0).all()


def test_a_chain_lattice_is_asg_token_align():
    """a seeded chain without ties: the scores inside the gate (the two sums are associated differently), equal spans"""
    em, trans, start, y = fp.chain_model()
    T, C = em.shape[1:]
    table = afp.table_of(start, trans)
    lat = afp.lattice_of(chain_lattice(y)[0], len(y), len(y) + 1, None, C, 4096)
    want = tfp.align_pair(em[0], table, y, len(y), T, 4096)
    for dtype in (np.float32, np.float64):
        r = fp.align_lattice(em[0], table, lat, T, len(y), dtype)
        assert abs(float(r.score) - float(want.score)) <= GATE * max(1.0, abs(float(want.score)))
        assert (r.starts == want.starts).all() and (r.ends == want.ends).all() and (r.frame_arcs == want.frame_tokens).all()
        assert (r.path_arcs == np.arange(len(y))).all() and r.path_len == len(y)


# ---- the entry points ----
def test_entry_points_exist_in_every_layer(gtn):
    from gtn_amd import torch_loss
    assert callable(torch_loss.asg_lattice_align) and callable(gtn.Batch.asg_lattice_align)
    assert hasattr(ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so")), "gtn_asg_lattice_align_n")
    eng = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_amd.so"))
    assert hasattr(eng, "gtnx_batch_asg_lattice_align") and hasattr(eng, "gtnx_batch_asg_lattice_align_stats")
    calls, utts = gtn.debug_asg_lattice_align_stats()
    assert calls >= 0 and utts >= 0
