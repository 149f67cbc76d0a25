"""The transducer entries over bfloat16 / float16 logits, the parts that need no GPU: the engine
refuses a dtype code that is neither GTNX_DTYPE_F16 nor GTNX_DTYPE_BF16 before a device is asked for, as it refuses what the
float32 entries refuse; gtn_amd.torch_loss still refuses float64 logits with the float32 entries' text and 16-bit host
tensors as host tensors."""
import ctypes

import pytest

ENTRIES = [("gtnx_batch_transducer_score16", False, 2), ("gtnx_batch_transducer_score_grad16", False, 3),
           ("gtnx_batch_transducer_pruned_score16", True, 2), ("gtnx_batch_transducer_pruned_score_grad16", True, 3)]


@pytest.mark.parametrize("name,pruned,outs", ENTRIES)
def test_engine_refuses_a_bad_dtype_before_the_device(gtn, name, pruned, outs):
    import gtn_amd
    lib = gtn_amd._lib
    lib.gtnx_last_error.restype = ctypes.c_char_p
    p = ctypes.c_void_p(64)
    before = gtn.debug_transducer_stats(), gtn.debug_transducer_pruned_stats()
    sizes = (1, 2, 2, 3, 4, 0, 1) if pruned else (1, 2, 3, 4, 0, 1)  # B, T, [S,] U, C, blank, normalize
    pointers = (p,) * (4 if pruned else 3)
    for dtype in (0, 3, 4, -1):  # (3 is GTNX_DTYPE_F32: the float32 entries' own)
        assert getattr(lib, name)(p, dtype, *pointers, *sizes, *(p,) * outs) == 1, dtype
        assert lib.gtnx_last_error().decode() == f"[{name}] the logits must be GTNX_DTYPE_F16 or GTNX_DTYPE_BF16"
    for dtype in (1, 2):  # (a good dtype: the float32 entries' refusals, in their words)
        bad = sizes[:-3] + (0,) + sizes[-2:]
        assert getattr(lib, name)(p, dtype, *pointers, *bad, *(p,) * outs) == 1
        assert lib.gtnx_last_error().decode() == f"[{name}] C outside 1 .. 2^20"
        assert getattr(lib, name)(p, dtype, *pointers, 0, *sizes[1:], *(p,) * outs) == 0  # (no utterance: nothing to do)
    assert (gtn.debug_transducer_stats(), gtn.debug_transducer_pruned_stats()) == before  # (nothing launched)


@pytest.mark.parametrize("pruned", [False, True])
def test_torch_entries_refuse_float64_and_host_tensors(pruned):
    import torch
    import gtn_amd.torch_loss as tl
    x, y = torch.zeros(2, 3, 4, 5), torch.zeros(2, 3, dtype=torch.int32)
    n = torch.ones(2, dtype=torch.int32)
    score, loss = (tl.transducer_pruned_score, tl.transducer_pruned_loss) if pruned else (tl.transducer_score,
                                                                                        tl.transducer_loss)
    index = (torch.zeros(2, 3, dtype=torch.int32), y, n, n) if pruned else (y, n, n)
    for call in (score, loss):
        with pytest.raises(ValueError, match=r"logits must be a float32 tensor \[.*\] \(or bfloat16 / float16\)"):
            call(x.double(), *index)
        for dtype in (torch.float32, torch.bfloat16, torch.float16):
            with pytest.raises(RuntimeError, match="logits must be a CUDA tensor"):
                call(x.to(dtype), *index)
    with pytest.raises(ValueError, match="dtype = float16 is not what logits says"):
        import gtn_amd
        entry = gtn_amd.transducer_pruned_score if pruned else gtn_amd.transducer_score
        entry(x.bfloat16(), *index, n.float(), dtype="float16")
