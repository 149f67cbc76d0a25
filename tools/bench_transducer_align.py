"""Times the transducer forced alignment (gtn_amd/csrc/transducer_align.hip) at section 42's shape,
B 32, T 400, U 100, C 1024, normalised, full lengths, for float32 and bfloat16 logits: the align call from the logits
with all four outputs and with the two required ones, the align call from a kept rows plane, and transducer_score's
forward call on the same inputs.  The routes alternate, ROUNDS windows each of at least 0.5 s (a host clock around a
closing synchronise), and every figure is the (least, median, greatest) of its windows.

Kernel means are the engine's own event timings (gtn_amd.prof_*, the GTNX_PROF scopes) over a few calls after the timed
windows.  The align kernel is one launch, sweep and walk together; its walk and output share is the difference to the
same launch over a plane whose last blank arc is closed, where the sweep is the same and the walk is skipped.  The
microseconds per step divide by the T + U / K steps of the skewed sweep, for the align kernel and for the score call's
logadd sweep.

The stated baseline is the plain-torch route: log_softmax, two gathers, torch.maximum along the anti-diagonals, .cpu() and
a host back-trace; its time, torch's peak allocation above the inputs, and its agreement with the align call (scores
within 1e-4 max(1, |score|), asserted after the record is written; the number of token frames that differ, recorded --
the two normalisers differ in their last bits, so a near-tie may legitimately differ).
Every figure is printed as soon as it exists.  Writes profiles/transducer_align.json (or --out).

    python tools/bench_transducer_align.py [--out PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, T, U, C = 32, 400, 100, 1024
K = 2  # (columns per lane at U + 1 = 101)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transducer_align.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import gtn_amd
    assert torch.cuda.is_available(), "the benchmark measures the GPU and has no other route"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    esync = lambda: (gtn_amd.synchronize(), torch.cuda.synchronize())
    steps = T + U // K
    rec = {"tool": "tools/bench_transducer_align.py", "shape": {"B": B, "T": T, "U": U, "C": C}, "rounds": ROUNDS,
           "sweep_steps": steps,
           "timing": "calls: host clock, alternating windows >= 0.5 s, [least, median, greatest] ms; kernels: the "
                     "engine's event timings",
           "not_measured": "ragged lengths, T above 960 rows (the bit plane in scratch), K other than 2"}

    def fig(key, v):
        rec[key] = v
        print("FIG " + json.dumps([key, v]), flush=True)

    def spread(fns):
        for fn in fns.values():
            fn(), esync()
        ms = {k: [] for k in fns}
        for _ in range(ROUNDS):
            for k, fn in fns.items():
                ms[k].append(1e3 * window(fn, esync))
        return {k: [min(v), statistics.median(v), max(v)] for k, v in ms.items()}

    def kernels(fn, names):
        gtn_amd.prof_enable(True)
        gtn_amd.prof_reset()
        for _ in range(5):
            fn()
        esync()
        prof = {k: gtn_amd.prof_get(k) for k in names}
        gtn_amd.prof_enable(False)
        return {k: v["total_ms"] / max(v["launches"], 1) for k, v in prof.items()}

    g = torch.Generator(device="cuda:0").manual_seed(1)
    blank = 0
    y = torch.randint(1, C, (B, U), device="cuda:0", generator=g, dtype=torch.int32)
    frames = torch.full((B,), T, device="cuda:0", dtype=torch.int32)
    tlens = torch.full((B,), U, device="cuda:0", dtype=torch.int32)
    scores, scores2 = torch.empty(B, device="cuda:0"), torch.empty(B, device="cuda:0")
    tf = torch.empty(B, U, dtype=torch.int32, device="cuda:0")
    ts = torch.empty(B, U, device="cuda:0")
    ft = torch.empty(B, T, dtype=torch.int32, device="cuda:0")
    rows = torch.empty(B, T, U + 1, 3, device="cuda:0")
    gtn_amd.set_stream(None)
    ninf = float("-inf")

    def torch_route(x):
        """(scores [B] on the device, token frames [B, U] on the host) in plain torch and numpy"""
        lp = torch.log_softmax(x.float(), dim=-1)
        lpb = lp[..., blank].contiguous()
        lpl = torch.gather(lp[:, :, :U], 3, y.long()[:, None, :, None].expand(B, T, U, 1)).squeeze(3).contiguous()
        del lp
        v = torch.full((B, T, U + 1), ninf, device=x.device)
        label = torch.zeros((B, T, U + 1), dtype=torch.bool, device=x.device)
        v[:, 0, 0] = 0
        for d in range(1, T + U):
            t = torch.arange(max(0, d - U), min(T - 1, d) + 1, device=x.device)
            u = d - t
            up = torch.where(t > 0, v[:, t - 1, u] + lpb[:, t - 1, u], ninf)
            left = torch.where(u > 0, v[:, t, u - 1] + lpl[:, t, u - 1], ninf)
            label[:, t, u] = left > up
            v[:, t, u] = torch.maximum(up, left)
        out = v[:, T - 1, U] + lpb[:, T - 1, U]
        lab = label.cpu().numpy()
        token_frames = np.zeros((B, U), np.int32)
        for b in range(B):
            t, u = T - 1, U
            while t or u:
                if lab[b, t, u]:
                    u -= 1
                    token_frames[b, u] = t
                else:
                    t -= 1
        return out, token_frames

    for dtype in (torch.float32, torch.bfloat16):
        key = str(dtype)[6:]
        x = torch.randn(B, T, U + 1, C, device="cuda:0", generator=g)
        x[..., blank] += 3 + 6.93  # (peaked as the tests' cases are, so that |score| stays small)
        x = x.to(dtype)
        index = (y, frames, tlens)
        gtn_amd.transducer_score(x, *index, scores, rows, blank)
        esync()
        closed = rows.clone()
        closed[:, T - 1, U, 0] = ninf  # (no path: the sweep is the same and the walk is skipped)
        out = {"logits_bytes": x.numel() * x.element_size()}
        calls = {"align_all": lambda: gtn_amd.transducer_align(x, *index, scores, tf, ts, ft, None, blank),
                 "align_required": lambda: gtn_amd.transducer_align(x, *index, scores, tf, None, None, None, blank),
                 "align_rows_all": lambda: gtn_amd.transducer_align_rows(rows, frames, tlens, scores, tf, ts, ft),
                 "score_forward": lambda: gtn_amd.transducer_score(x, *index, scores2, None, blank),
                 "torch_route": lambda: torch_route(x)}
        out["calls_ms"] = spread(calls)
        esync()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        want_scores, want_frames = torch_route(x)
        esync()
        out["torch_route_peak_bytes_above_inputs"] = torch.cuda.max_memory_allocated() - base
        rows_name = "transducer_rows" if dtype == torch.float32 else "transducer16_rows"
        k = kernels(calls["align_all"], (rows_name, "transducer_align"))
        k["transducer_align_after_rows"] = k.pop("transducer_align")  # (behind the streaming rows kernel)
        k.update(kernels(calls["score_forward"], ("transducer_sweep",)))  # (behind the same rows kernel)
        # the two below run alone on a kept plane, so they compare with each other and not with the two above
        k["transducer_align"] = kernels(calls["align_rows_all"], ("transducer_align",))["transducer_align"]
        k["transducer_align_walk_skipped"] = kernels(
            lambda: gtn_amd.transducer_align_rows(closed, frames, tlens, scores2, tf, ts, ft), ("transducer_align",)
        )["transducer_align"]
        out["kernels_ms"] = k
        out["us_per_step"] = {"align_after_rows": 1e3 * k["transducer_align_after_rows"] / steps,
                              "score_logadd_sweep_after_rows": 1e3 * k["transducer_sweep"] / steps,
                              "align_on_kept_rows": 1e3 * k["transducer_align"] / steps,
                              "align_on_kept_rows_walk_skipped": 1e3 * k["transducer_align_walk_skipped"] / steps}
        out["walk_and_outputs_ms"] = k["transducer_align"] - k["transducer_align_walk_skipped"]
        calls["align_all"]()
        esync()
        err = (scores - want_scores).abs().max().item()
        differ = int((tf.cpu().numpy() != want_frames).sum())
        out["agreement_with_torch_route"] = {"score_abs": err, "token_frames_that_differ": differ, "of": B * U}
        fig(key, out)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
        assert err <= 1e-4 * max(1.0, want_scores.abs().max().item()), (key, err)
        del x, closed
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
