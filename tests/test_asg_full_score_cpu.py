"""The batched ASG full-connect score for up to 1024 labels, the parts that need no GPU: the entry
points exist in every layer, refuse bad arguments before they ask for a device and name themselves, and the float32
transcription of the scaled recursion (tests/asg_full_f32.py) stays within HALF of each gate against asg_fp64 on every
shape tests/test_asg_full_score_gpu.py launches, so the gates are within reach of float32 before a GPU is involved."""
import ctypes
import os

import numpy as np
import pytest

import asg_full_score_fp as fp
from asg_full_f32 import asg_full_f32
from conftest import ROOT


def test_entry_points_exist(gtn):
    from gtn_amd import torch_loss
    assert callable(torch_loss.asg_full_score)
    lib = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_criteria.so"))
    assert hasattr(lib, "gtn_asg_full_score_n") and hasattr(lib, "gtn_asg_full_score_grad_n")
    eng = ctypes.CDLL(os.path.join(ROOT, "gtn_amd", "lib", "libgtn_amd.so"))
    for name in ("gtnx_batch_asg_full_score", "gtnx_batch_asg_full_score_grad", "gtnx_batch_asg_full_score_stats"):
        assert hasattr(eng, name), name
    assert callable(gtn.Batch.asg_full_score) and callable(gtn.Batch.asg_full_score_grad)
    calls, utts = gtn.debug_asg_full_score_stats()
    assert calls >= 0 and utts >= 0
    for header, name in (("include/gtn/batch.h", "asgFullScoreGrad"), ("include/gtn/batch.h", "asgFullScore"),
                         ("gtn_amd/criteria/asg_criterion.h", "asgFullScoreBatch"),
                         ("gtn_amd/csrc/Makefile", "asg_full_wide.hip")):
        with open(os.path.join(ROOT, header)) as f:
            assert name in f.read(), header


def test_argument_errors_come_before_the_device(gtn):
    import gtn_amd
    lib = gtn_amd._lib
    lib.gtnx_last_error.restype = ctypes.c_char_p
    batch = gtn.Batch([gtn.linear_graph(2, 8)])
    p = ctypes.c_void_p
    score, grad = lib.gtnx_batch_asg_full_score, lib.gtnx_batch_asg_full_score_grad
    before = gtn.debug_asg_full_score_stats()
    #          ems       frames table  scores | weights grad_em grad_table
    for args, text in (((None, None, p(64), p(64)), "null batch"), ((batch._h, None, None, p(64)), "null table"),
                       ((batch._h, None, p(64), None), "null scores")):
        assert score(*args) == 1, text
        msg = lib.gtnx_last_error().decode()
        assert msg.startswith("[gtnx_batch_asg_full_score] " + text) or args[0] is None and "null batch" in msg, msg
    for args, text in (((None, None, p(64), p(64), p(64), p(64)), "null batch"),
                       ((batch._h, None, None, p(64), p(64), p(64)), "null table"),
                       ((batch._h, None, p(64), None, p(64), p(64)), "null weights"),
                       ((batch._h, None, p(64), p(64), None, None), "neither gradient")):
        assert grad(*args) == 1, text
        msg = lib.gtnx_last_error().decode()
        assert msg.startswith("[gtnx_batch_asg_full_score_grad] " + text) or args[0] is None and "null batch" in msg, msg
    assert gtn.debug_asg_full_score_stats() == before  # (nothing launched)
    with pytest.raises(ValueError, match="neither grad_out nor grad_table_out"):
        batch.asg_full_score_grad(64, 64)
    with pytest.raises(ValueError, match="one frame count per element"):
        batch.asg_full_score(64, 64, frames=[1, 2])


@pytest.mark.parametrize("shape", fp.SHAPES, ids=str)
def test_the_transcription_stays_within_half_the_gates(shape):
    em, trans, start, frames, w, *want = fp.case(shape)
    B, T, C = shape
    tw = np.concatenate([start, trans.reshape(-1)])
    Z, g_em, g_tab = np.full(B, -np.inf), np.zeros((B, T, C), np.float32), np.zeros(C + C * C)
    for b, f in enumerate(frames):
        if f > 0:
            Z[b], g_em[b, :f], part = asg_full_f32(em[b, :f], tw, w[b])
            g_tab += part.astype(np.float64)
    fp.check(str(shape), Z, g_em, g_tab, want, frames, part=0.5)
