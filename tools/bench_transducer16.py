"""Times the transducer score and its pruned form over bfloat16 / float16 logits (gtn_amd/csrc/transducer16.hip, DESIGN
section 45) at B 32, T 400, U 100, C 1024 (full lattice) and S 5 (band), normalised, full lengths: the score call, score
plus gradient through torch_loss (the rows plane kept), torch's peak allocation above the inputs, and the rows16 / grad16
kernels with their achieved bytes/s.

The comparison is the only route a caller with 16-bit logits had before: logits.float() -> the float32 entry -> the
gradient cast back to the dtype.  Its kernels are the float32 ones, which this tool runs in the same session.  The two
routes alternate, ROUNDS windows each of at least 0.5 s (a host clock around a closing synchronise), and every figure is
the (least, median, greatest) of its windows, so the run-to-run spread stands beside every ratio.  Kernel means are the
engine's own event timings (gtn_amd.prof_*, the GTNX_PROF scopes) over a few calls after the timed windows; bytes are the
scopes' algorithmic counts with 2-byte elements.  The values of both routes are compared after the record is written.
Every figure is printed as soon as it exists.  Writes profiles/transducer16.json (or --out).

    python tools/bench_transducer16.py [--out PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, T, U, S, C = 32, 400, 100, 5, 1024
ROUNDS = 5


def window(fn, sync, least=0.5):
    """seconds per call of fn over a window of at least `least` seconds, closed by one synchronise"""
    calls, t0 = 0, time.perf_counter()
    while True:
        fn()
        calls += 1
        sync()
        dt = time.perf_counter() - t0
        if dt >= least:
            return dt / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transducer16.json"))
    a = ap.parse_args()
    import torch
    import gtn_amd
    import gtn_amd.torch_loss as tl
    assert torch.cuda.is_available(), "the benchmark measures the GPU and has no other route"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    esync = lambda: (gtn_amd.synchronize(), torch.cuda.synchronize())
    rec = {"tool": "tools/bench_transducer16.py", "shape": {"B": B, "T": T, "U": U, "S": S, "C": C}, "rounds": ROUNDS,
           "timing": "calls: host clock, alternating windows >= 0.5 s, [least, median, greatest] ms; kernels: the "
                     "engine's event timings",
           "cast_route": "logits.float() -> the float32 entry -> gradient cast back; float32 kernels, same session",
           "not_measured": "ragged lengths, C > 4096, the 2-byte path"}

    def fig(key, v):
        rec[key] = v
        print("FIG " + json.dumps([key, v]), flush=True)

    def spread(fns):
        """{name: [least, median, greatest] ms} of the routes, their windows alternating"""
        for fn in fns.values():
            fn(), esync()
        ms = {k: [] for k in fns}
        for _ in range(ROUNDS):
            for k, fn in fns.items():
                ms[k].append(1e3 * window(fn, esync))
        return {k: [min(v), statistics.median(v), max(v)] for k, v in ms.items()}

    def peak(fn):
        esync()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        esync()
        return torch.cuda.max_memory_allocated() - base

    g = torch.Generator(device="cuda:0").manual_seed(1)
    blank = 0
    y = torch.randint(1, C, (B, U), device="cuda:0", generator=g, dtype=torch.int32)
    frames = torch.full((B,), T, device="cuda:0", dtype=torch.int32)
    tlens = torch.full((B,), U, device="cuda:0", dtype=torch.int32)
    w = torch.linspace(0.5, 1.5, B, device="cuda:0")
    scores = torch.empty(B, device="cuda:0")
    gtn_amd.set_stream(None)
    # (the band on the diagonal, as tools/bench_transducer_pruned.py has it)
    ranges = ((torch.arange(T, device="cuda:0") * (U + 1 - S)) // (T - 1)).to(torch.int32)[None].repeat(B, 1).contiguous()

    def logits(width, dtype):
        x = torch.randn(B, T, width, C, device="cuda:0", generator=g)
        x[..., blank] += 3 + 6.93  # (peaked as the tests' cases are, so that |score| stays small)
        return x.to(dtype)

    for entry, width in (("full", U + 1), ("pruned", S)):
        index = (y, frames, tlens) if entry == "full" else (ranges, y, frames, tlens)
        raw, torch_score, names = ((gtn_amd.transducer_score, tl.transducer_score, ("transducer16_rows", "transducer16_grad"))
                                   if entry == "full" else
                                   (gtn_amd.transducer_pruned_score, tl.transducer_pruned_score,
                                    ("transducer16_pruned_rows", "transducer16_pruned_grad")))
        for dtype in (torch.bfloat16, torch.float16):
            key = f"{entry}_{str(dtype)[6:]}"
            x = logits(width, dtype)

            def both(cast):
                xr = x.detach().requires_grad_(True)
                out = torch_score(xr.float() if cast else xr, *index, blank)
                out.backward(w)
                return out.detach(), xr.grad

            out = {"logits_bytes": x.numel() * 2}
            out["score_ms"] = spread({"direct": lambda: raw(x, *index, scores, None, blank),
                                      "cast": lambda: raw(x.float(), *index, scores, None, blank)})
            out["score_grad_ms"] = spread({"direct": lambda: both(False), "cast": lambda: both(True)})
            for k in ("score_ms", "score_grad_ms"):
                out[k]["cast_over_direct_median"] = out[k]["cast"][1] / out[k]["direct"][1]
            # (torch's allocator only; the engine's pooled scratch, 8 bytes per node, is the same on both routes)
            out["peak_torch_bytes_above_inputs"] = {"direct": peak(lambda: both(False)), "cast": peak(lambda: both(True))}
            gtn_amd.prof_enable(True)
            gtn_amd.prof_reset()
            for _ in range(3):
                both(False)
            esync()
            prof = {k: gtn_amd.prof_get(k) for k in names}
            gtn_amd.prof_enable(False)
            for k, v in prof.items():
                ms = v["total_ms"] / max(v["launches"], 1)
                per = v["algorithmic_bytes"] / max(v["launches"], 1)
                out[k] = {"mean_ms": ms, "model_bytes": per, "model_GBps": per / ms / 1e6 if ms else None}
            fig(key, out)
            with open(a.out, "w") as f:
                json.dump(rec, f, indent=1, sort_keys=True)
            (sd, gd), (sc, gc) = both(False), both(True)
            err, gerr = (sd - sc).abs().max().item(), (gd.float() - gc.float()).abs().max().item()
            print(f"{key}: agreement with the cast route: score {err} gradient {gerr}", flush=True)
            rec[key]["agreement_with_cast_route"] = {"score_abs": err, "gradient_abs": gerr}
            assert err <= 1e-4 * max(1.0, sc.abs().max().item()), (key, err)
            assert gerr <= 2.0 ** -7 * max(1.0, gc.float().abs().max().item()), (key, gerr)  # (two roundings of the output)
            del x, sd, gd, sc, gc
            torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
