"""The one-launch CTC step's host side, without a device: gtnx_batch_ctc_loss_step refuses bad arguments before anything
is launched, and gtnx_batch_ctc_loss_step_ok -- the predicate by which criteria::ctcLossBatch chooses between that launch
and the graph-level operations -- is a pure host function (tests/test_ctc_step_fused_gpu.py has the table's GPU side)."""
import ctypes

import numpy as np
import pytest

P = ctypes.c_void_p
A16 = 0x10000  # a 16-byte aligned address: the predicate only looks at the pointers' alignment


def _lib():
    import gtn_amd
    lib = gtn_amd._lib
    lib.gtnx_last_error.restype = ctypes.c_char_p
    return lib


def _ok(lib, targets, T, C, blank=0, em=A16, grad=A16):
    lens = np.array([len(t) for t in targets], np.int32)
    flat = np.concatenate([np.asarray(t, np.int32) for t in targets] + [np.zeros(0, np.int32)]).astype(np.int32)
    ok = ctypes.c_int(-1)
    rc = lib.gtnx_batch_ctc_loss_step_ok(flat.ctypes.data if flat.size else None, lens.ctypes.data, len(targets), T, C, blank,
                                         P(em) if em else None, P(grad) if grad else None, ctypes.byref(ok))
    assert rc == 0, lib.gtnx_last_error().decode()
    return ok.value


def test_bad_arguments_are_refused_before_the_device(gtn):
    """GTNX_INVALID_ARGUMENT (1) for a negative length, B = 0 and a null loss pointer -- with or without a GPU, so nothing
    was launched"""
    lib = _lib()
    call = lib.gtnx_batch_ctc_loss_step
    lab = np.array([1, 2, 3], np.int32)
    lens = np.array([2, 1], np.int32)
    #        em      labels            lengths          n  T  C  blank loss    grad   tgrad tgrad_dev
    good = [P(A16), lab.ctypes.data, lens.ctypes.data, 2, 5, 8, 0, P(A16), P(A16), 1, None]
    neg = np.array([2, -1], np.int32)
    for i, v, text in ((3, 0, "the batch size must be positive"), (3, -2, "the batch size must be positive"),
                       (7, None, "null emissions, lengths, loss or gradient"),
                       (8, None, "null emissions, lengths, loss or gradient"),
                       (0, None, "null emissions, lengths, loss or gradient"),
                       (2, neg.ctypes.data, "negative length"), (4, 0, "T and C must be positive"),
                       (1, None, "null labels")):
        a = list(good)
        a[i] = v
        assert call(*a) == 1, (i, v)
        assert lib.gtnx_last_error().decode() == "[gtnx_batch_ctc_loss_step] " + text, (i, v)
    # a batch the launch has no cell for is refused by the entry point as well (ctcLossBatch never sends one)
    a = list(good)
    a[5] = 27
    assert call(*a) == 1
    assert "not a batch the one-launch step takes" in lib.gtnx_last_error().decode()
    ok = ctypes.c_int(0)
    assert lib.gtnx_batch_ctc_loss_step_ok(lab.ctypes.data, lens.ctypes.data, 2, 5, 8, 0, P(A16), P(A16), None) == 1


def test_fallback_predicate_table(gtn):
    lib = _lib()
    t = lambda U, lo=1: [lo + (i % 3) for i in range(U)]
    # taken: every U of the GPU test's table, the three alphabets, mixed lengths, an empty target
    for U in (1, 2, 31, 32, 63, 64, 95, 96, 127):
        for C in (4, 28, 256):
            assert _ok(lib, [t(U), t(1), t(5)], 33, C) == 1, (U, C)
    assert _ok(lib, [[], t(3)], 1, 4) == 1
    assert _ok(lib, [t(100)] * 5, 1000, 256) == 1      # the benchmark's shape
    assert _ok(lib, [t(100)], 50, 512) == 1            # (rows per block 4 forward, 2 backward)
    assert _ok(lib, [t(127)], 50, 256) == 1            # (8 forward, 2 backward: four rows of 256 nodes do not fit LDS)
    # not taken
    assert _ok(lib, [t(128), t(3)], 33, 28) == 0       # two nodes per lane
    assert _ok(lib, [t(5)], 33, 27) == 0               # C not a multiple of 4
    assert _ok(lib, [t(5)], 33, 516) == 0              # past the non-BIG range
    assert _ok(lib, [t(5)], 33, 1024) == 0
    assert _ok(lib, [[1, -1, 2]], 33, 28) == 0         # a negative label
    assert _ok(lib, [[1, 28, 2]], 33, 28) == 0         # a label outside the alphabet
    assert _ok(lib, [t(5)], 33, 28, blank=28) == 0
    assert _ok(lib, [t(5)], 33, 28, em=A16 + 4) == 0   # emissions not 16-byte aligned
    assert _ok(lib, [t(5)], 33, 28, grad=A16 + 8) == 0
    assert _ok(lib, [t(5)], 33, 28, grad=None) == 0    # no gradient buffer
    assert _ok(lib, [t(5)], 0, 28) == 0
    assert _ok(lib, [], 33, 28) == 0
