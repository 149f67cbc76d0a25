"""gtnx_batch_ctc_loss_step16_ok, the host predicate of the 16-bit CTC step, at the edges of the launch's range: a pure
host function, so it answers without a device (tests/test_ctc_step16_gpu.py has the kernel's side)."""
import ctypes

import numpy as np

P = ctypes.c_void_p
A16 = 0x10000  # a 16-byte aligned address: the predicate only looks at the pointers' alignment


def _ok(lib, targets, T, C, blank=0, frames=None, em=A16, grad=A16):
    lens = np.array([len(t) for t in targets], np.int32)
    flat = np.concatenate([np.asarray(t, np.int32) for t in targets] + [np.zeros(0, np.int32)]).astype(np.int32)
    fr = None if frames is None else np.asarray(frames, np.int32)
    ok = ctypes.c_int(-1)
    rc = lib.gtnx_batch_ctc_loss_step16_ok(flat.ctypes.data if flat.size else None, lens.ctypes.data,
                                           None if fr is None else fr.ctypes.data, len(targets), T, C, blank, P(em),
                                           P(grad), ctypes.byref(ok))
    assert rc == 0
    return ok.value


def test_predicate_at_the_range_edges(gtn):
    lib = gtn._lib
    t = lambda U: [1 + (i % 7) for i in range(U)]
    assert _ok(lib, [t(5), []], 33, 8) == 1
    assert _ok(lib, [t(5)], 33, 4) == 0
    assert _ok(lib, [t(5)], 33, 4096) == 1
    assert _ok(lib, [t(5)], 33, 4104) == 0
    assert _ok(lib, [t(5)], 33, 12) == 0               # no 16-byte pieces
    assert _ok(lib, [t(511), t(3)], 1 << 20, 8) == 1
    assert _ok(lib, [t(512), t(3)], 600, 8) == 0
    assert _ok(lib, [t(5)], (1 << 20) + 1, 8) == 0
    assert _ok(lib, [[1, 8, 2]], 33, 8) == 0           # a label equal to C
    assert _ok(lib, [[1, -1, 2]], 33, 8) == 0
    assert _ok(lib, [t(5)], 33, 8, blank=8) == 0
    assert _ok(lib, [t(5), t(2)], 33, 8, frames=[1, 33]) == 1
    assert _ok(lib, [t(5), t(2)], 33, 8, frames=[0, 33]) == 0
    assert _ok(lib, [t(5), t(2)], 33, 8, frames=[5, 34]) == 0
    assert _ok(lib, [t(5)], 33, 8, em=A16 + 2) == 0
    assert _ok(lib, [t(5)], 33, 8, grad=A16 + 8) == 0
