"""criteria::ctcLossBatch as ONE launch (gtn_amd/csrc/ctc_step.hip: target records, forward sweep, loss, backward sweep by
one workgroup per utterance) against the graph-level operations it replaces, in one process: every case runs the
criterion twice through libgtn_criteria.so -- GTNX_CTC_STEP_FUSED=0, then the default -- and asks for BIT-IDENTICAL losses,
emission gradients and target-arc gradients (the sweeps are the same code; a difference is an ordering, visibility or
seed bug), then checks the fused result against float64 (tests/ctc_fp64.py) with the project's gates: loss 1e-4 relative,
emission gradient 1e-4 absolute, gradient rows summing to 0 within tests/test_batch_gpu.py's 5e-4.  Which path ran is read
off the profiler families: the graph-level step has a band_forward_score launch, the one-launch step only a
band_forward_score_grad one.

Shapes are the smallest at which the kernel can go wrong: T around the sweeps' blocks of 8 and 4 rows and the four-wave
skew, node counts 2U + 1 on both sides of every 64-node wave boundary, lengths mixed inside a batch (uniform strides
against per-utterance N), the three alphabets, target gradients on and off; B is 1, 3 or 5 throughout."""
import ctypes as C
import os

import numpy as np
import pytest

import graphgen as gg
from ctc_fp64 import ctc_loss_fp64

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_SUM_TOL = 5e-4  # tests/test_batch_gpu.py
U_TABLE = (1, 2, 31, 32, 63, 64, 95, 96, 127)


def _lib():
    lib = C.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    lib.gtn_ctc_loss_step_n.argtypes = [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p] * 3 + [C.c_int, C.c_void_p]
    lib.gtn_ctc_loss_step_n.restype = C.c_int
    lib.gtn_criteria_last_error.restype = C.c_char_p
    return lib


def _arc_counts(tg):
    return [(2 * len(t) + 1) + 2 * len(t) + sum(1 for i in range(1, len(t)) if t[i] != t[i - 1]) for t in tg]


class Step:
    """one call of ctcLossBatch, its outputs left on the device until fetch()"""

    def __init__(self, gtn, lib, em_dev, tg, T, Cn, fused, target_grad=True, frames=None, with_grad=True):
        import torch
        B = len(tg)
        self.lens = np.array([len(t) for t in tg], np.int32)
        self.flat = np.concatenate([np.asarray(t, np.int32) for t in tg] + [np.zeros(0, np.int32)]).astype(np.int32)
        self.fr = None if frames is None else np.asarray(frames, np.int32)
        self.loss = torch.full((B,), float("nan"), device="cuda:0")
        self.grad = torch.full((B, T, Cn), float("nan"), device="cuda:0") if with_grad else None
        n_arcs = int(sum(_arc_counts(tg)))
        self.tgrad = torch.full((max(n_arcs, 1),), float("nan"), device="cuda:0") if target_grad and with_grad else None
        torch.cuda.synchronize()
        if fused:
            os.environ.pop("GTNX_CTC_STEP_FUSED", None)
        else:
            os.environ["GTNX_CTC_STEP_FUSED"] = "0"
        try:
            rc = lib.gtn_ctc_loss_step_n(em_dev.data_ptr(), self.flat.ctypes.data, self.lens.ctypes.data, B, T, Cn, 0,
                                         None if self.fr is None else self.fr.ctypes.data, self.loss.data_ptr(),
                                         None if self.grad is None else self.grad.data_ptr(), 1 if target_grad else 0,
                                         None if self.tgrad is None else self.tgrad.data_ptr())
        finally:
            os.environ.pop("GTNX_CTC_STEP_FUSED", None)
        assert rc == 0, lib.gtn_criteria_last_error().decode()
        self.gtn = gtn

    def fetch(self):
        self.gtn.synchronize()
        return (self.loss.cpu().numpy(), None if self.grad is None else self.grad.cpu().numpy(),
                None if self.tgrad is None else self.tgrad.cpu().numpy())


def _profiled(gtn, make):
    """-> (make()'s fetched outputs, launches of the forward-sweep family, of the backward-sweep family)"""
    gtn.prof_reset()
    gtn.prof_enable(True)
    try:
        out = make().fetch()
    finally:
        gtn.prof_enable(False)
    names = gtn.prof_names()
    n = lambda k: gtn.prof_get(k)["launches"] if k in names else 0
    return out, n("band_forward_score"), n("band_forward_score_grad")


def _same_bits(a, b, what):
    assert a.shape == b.shape, what
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, float(np.nanmax(np.abs(a - b))))


def _both_paths(gtn, em, tg, T, Cn, target_grad=True, expect_fused=True, frames=None, with_grad=True):
    """the two runs of one case: identical bits, the expected path each; -> the default run's outputs"""
    import torch
    lib = _lib()
    em_dev = torch.from_numpy(np.ascontiguousarray(em)).to("cuda:0")
    kw = dict(target_grad=target_grad, frames=frames, with_grad=with_grad)
    old, f_old, g_old = _profiled(gtn, lambda: Step(gtn, lib, em_dev, tg, T, Cn, False, **kw))
    new, f_new, g_new = _profiled(gtn, lambda: Step(gtn, lib, em_dev, tg, T, Cn, True, **kw))
    assert f_old >= 1 and (g_old >= 1) == with_grad, ("GTNX_CTC_STEP_FUSED=0 runs the graph-level step", f_old, g_old)
    if expect_fused:
        assert (f_new, g_new) == (0, 1), ("the default runs the one-launch step", f_new, g_new)
    else:
        assert (f_new, g_new) == (f_old, g_old), ("this batch stays on the graph-level step", f_new, g_new)
    _same_bits(old[0], new[0], "losses")
    if with_grad:
        _same_bits(old[1], new[1], "emission gradients")
    if target_grad and with_grad:
        _same_bits(old[2], new[2], "target-arc gradients")
        assert np.all(np.isfinite(new[2]))
    return new


def _against_fp64(em, tg, out, frames=None):
    loss, grad, _ = out
    for b, t in enumerate(tg):
        f = em.shape[1] if frames is None else int(frames[b])
        want, wgrad, _ = ctc_loss_fp64(em[b, :f], t)
        if np.isfinite(want):
            assert abs(loss[b] - want) <= 1e-4 * max(1.0, abs(want)), (b, loss[b], want)
        else:
            assert loss[b] == np.inf, (b, loss[b])  # no path: the gradient is the normaliser's term alone
        if grad is None:
            continue
        assert np.abs(grad[b, :f] - wgrad).max() <= 1e-4, (b, np.abs(grad[b, :f] - wgrad).max())
        assert not np.any(grad[b, f:]), b
        if np.isfinite(want):  # (posteriors of a frame sum to one, and so does the softmax)
            assert np.abs(grad[b, :f].sum(axis=1)).max() <= ROW_SUM_TOL, (b, np.abs(grad[b, :f].sum(axis=1)).max())


def _inputs(seed, T, Cn, lens):
    em, tg = gg.ctc_inputs(seed, len(lens), T, Cn, max(max(lens), 1))
    return em, [tg[b][:u].copy() for b, u in enumerate(lens)]


def _lens(i, B):
    """B lengths: a short one that has a path at small T, then the table from position i on"""
    return [1 + i % 2] + [U_TABLE[(i + k) % len(U_TABLE)] for k in range(B - 1)]


# T: fewer rows than one block of either sweep (8 forward, 4 backward), exactly one, one over, fewer ticks than the
# four-wave skew; every U of the table and every C meets several T; B in {1, 3, 5}; target gradients alternate
_T = (1, 3, 4, 5, 7, 8, 9, 12, 33)
_CASES = []
for _i, _t in enumerate(_T):
    _b = (3, 5, 1)[_i % 3]
    _CASES.append((_t, (4, 28, 256)[_i % 3], [U_TABLE[_i % 9]] if _b == 1 else _lens(_i, _b), _i % 2 == 0))
for _i, _t in enumerate(_T):
    _CASES.append((_t, (28, 256, 4)[_i % 3], _lens(_i + 4, (5, 3)[_i % 2]), _i % 2 == 1))
# ... and with a path through every sweeper wave: T past the widest target
_CASES += [(300, 28, [127, 64, 95], True), (140, 4, [63, 32, 2, 31, 96], False), (260, 256, [127], True)]


@pytest.mark.parametrize("T,Cn,lens,target_grad", _CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else str(v))
def test_one_launch_step_is_the_graph_level_step(gtn, T, Cn, lens, target_grad):
    assert len(lens) in (1, 3, 5)
    em, tg = _inputs(1000 + T + Cn, T, Cn, lens)
    out = _both_paths(gtn, em, tg, T, Cn, target_grad=target_grad)
    _against_fp64(em, tg, out)


def test_every_node_count_of_the_table_in_one_pass(gtn):
    """the nine U of the table, three batches of three and five, at a T every one of them has a path at"""
    for Cn, lens in ((28, [1, 2, 31]), (256, [32, 63, 64, 95, 96]), (4, [127, 1, 96])):
        T = 2 * max(lens) + 3
        em, tg = _inputs(77 + Cn, T, Cn, lens)
        out = _both_paths(gtn, em, tg, T, Cn)
        _against_fp64(em, tg, out)
        assert np.all(np.isfinite(out[0]))


@pytest.mark.parametrize("what", ["U=128", "C=27", "frames", "no-grad"])
def test_fallback_cases_take_the_graph_level_step(gtn, what):
    T, Cn, lens, frames, with_grad = 12, 28, [3, 5, 2], None, True
    if what == "U=128":
        T, lens = 9, [128, 2, 5]  # two nodes per lane
    elif what == "C=27":
        Cn = 27
    elif what == "frames":
        frames = [12, 7, 12]  # one short utterance
    else:
        with_grad = False
    em, tg = _inputs(5, T, Cn, lens)
    out = _both_paths(gtn, em, tg, T, Cn, expect_fused=False, frames=frames, with_grad=with_grad)
    _against_fp64(em, tg, out, frames)


def test_full_frame_counts_are_no_padding(gtn):
    """a frames array whose every entry is T is the unpadded batch: the one-launch step"""
    em, tg = _inputs(6, 12, 28, [3, 5, 2])
    out = _both_paths(gtn, em, tg, 12, 28, frames=[12, 12, 12])
    _against_fp64(em, tg, out)


def test_content_edge_cases(gtn):
    T, Cn = 12, 28
    tg = [np.array([3, 3, 5, 5, 5, 2], np.int32),                 # immediate repeats: no skip arc between them
          np.array([7] * 5, np.int32),                             # all one label
          np.array([4, 9, 4, 9, 4], np.int32),                     # a label on more than two nodes (the drainers' run loop)
          np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13], np.int32),  # no path: T shorter than the target
          np.array([2, 2, 2, 2, 2, 2, 2], np.int32)]               # no path either: repeats need a blank between them
    em = gg.ctc_inputs(11, len(tg), T, Cn, 1)[0]
    out = _both_paths(gtn, em, tg, T, Cn)
    _against_fp64(em, tg, out)
    assert np.all(np.isfinite(out[0][:3])) and out[0][3] == np.inf and out[0][4] == np.inf
    assert not np.any(out[2][sum(_arc_counts(tg[:3])):])  # (no path: the arc gradients are written, as zeros)
    # eight and more blanks (the row sums carry the blank's element) with repeats and a thrice-used label
    tg = [np.array([4, 9, 4, 9, 4, 4, 1, 1, 2], np.int32)]
    em = gg.ctc_inputs(12, 1, 33, 4 * 7, 1)[0]
    out = _both_paths(gtn, em, tg, 33, 28)
    _against_fp64(em, tg, out)


def test_two_calls_back_to_back_reuse_the_pools(gtn):
    """five utterances, then three, on the same stream with nothing waited for in between: the staging block and arena
    the second call takes from the pools must not be the first call's while its launch is pending"""
    import torch
    lib = _lib()
    T, Cn = 33, 28
    em5, tg5 = _inputs(21, T, Cn, [31, 2, 12, 7, 1])
    em3, tg3 = _inputs(22, T, Cn, [5, 32, 3])
    d5 = torch.from_numpy(em5).to("cuda:0")
    d3 = torch.from_numpy(em3).to("cuda:0")
    want5 = Step(gtn, lib, d5, tg5, T, Cn, False).fetch()
    want3 = Step(gtn, lib, d3, tg3, T, Cn, False).fetch()
    a = Step(gtn, lib, d5, tg5, T, Cn, True)
    b = Step(gtn, lib, d3, tg3, T, Cn, True)
    got5, got3 = a.fetch(), b.fetch()
    for want, got in ((want5, got5), (want3, got3)):
        for w, g, what in zip(want, got, ("losses", "emission gradients", "target-arc gradients")):
            _same_bits(w, g, what)
    _against_fp64(em5, tg5, got5)
    _against_fp64(em3, tg3, got3)
