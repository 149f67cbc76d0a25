"""Times torch_loss.asg_full_score (gtn_amd/csrc/asg_full_wide.hip) at the ASG benchmark shape C4
(B 512, T 1000, C 512) and at C 1024, full-length and ragged (T_b uniform in [T/2, T]), for every group size G, beside
the routes the parent commit has: (a) asg_full_connect at full length (the dense regime), forward and forward plus
backward; (b) asg_full_connect(input_lengths=) on the per-length fallback for sixteen utterances, scaled per utterance.

Call timings are a host clock around a closing synchronise over windows of at least 0.5 s, in --procs fresh processes
(the median is kept).  Kernel means are the engine's own event timings (gtn_amd.prof_*, the GTNX_PROF scopes
asg_full_score_prep / _forward / _backward / _table / _reduce) over a few steps after the timed windows; from them come
the time per frame of a workgroup's chain (forward kernel / max T_b) and the table kernel's share of the f32 MFMA
floor.  A `rocprofv3 --kernel-trace --stats` run takes `--child` as the program behind `--`.  G is switched through
GTNX_ASG_FULL_SCORE_GROUP inside the process: the engine reads it per call.  Every figure is printed as soon as it
exists, and a route that fails is recorded with its message beside what ran.  Writes profiles/asg_full_score_c4.json.

    python tools/bench_asg_full_score.py [--procs 3] [--skip-fallback]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"c4": (512, 1000, 512), "c1024": (512, 1000, 1024)}
MFMA_F32_FLOPS = 157.3e12  # v_mfma_f32_32x32x2_f32 over the chip (gtn_amd/csrc/lazy.hip's arithmetic)
KERNELS = ("prep", "forward", "backward", "table", "reduce")


def window(fn, sync, least=0.5):
    """seconds per call of fn over a window of at least `least` seconds, closed by one synchronise"""
    fn(), sync()
    calls, t0 = 0, time.perf_counter()
    while True:
        fn()
        calls += 1
        if calls % 4 == 0 or calls == 1:
            sync()
            dt = time.perf_counter() - t0
            if dt >= least:
                return dt / calls


def child(skip_fallback):
    import numpy as np
    import torch
    import gtn_amd
    import gtn_amd.torch_loss as tl
    sync = torch.cuda.synchronize

    def fig(shape, key, fn):
        try:
            v = fn()
        except Exception as e:  # (recorded beside what ran, with the statement that raised)
            at = traceback.extract_tb(e.__traceback__)[-1]
            v = f"failed: {str(e).splitlines()[0]} (raised in {at.name}, {os.path.basename(at.filename)}:{at.lineno})"
        print("FIG " + json.dumps([shape, key, v]), flush=True)
        try:  # (an error code a call left behind would be reported by the next launch: say whose it is)
            torch.ones(4, device="cuda:0").sum().item()
        except Exception as e:
            print("FIG " + json.dumps([shape, key + "_left_a_pending_error", str(e).splitlines()[0]]), flush=True)

    for name, (B, T, C) in SHAPES.items():
        g = torch.Generator(device="cuda:0").manual_seed(1)
        x = torch.log_softmax(torch.randn(B, T, C, device="cuda:0", generator=g), -1)
        tr = torch.randn(C, C, device="cuda:0", generator=g)
        st = torch.randn(C, device="cuda:0", generator=g)
        w = torch.linspace(0.5, 1.5, B, device="cuda:0")
        ragged = np.random.default_rng(2).integers(T // 2, T + 1, B).astype(np.int32)
        cpad = (C + 31) // 32 * 32
        for frames_name, frames in (("full", None), ("ragged", ragged)):
            max_T = T if frames is None else int(frames.max())
            sum_T = float(B * T if frames is None else frames.sum())

            def step():
                xr, trr = x.detach().requires_grad_(True), tr.detach().requires_grad_(True)
                tl.asg_full_score(xr, trr, st, frames).backward(w)
            for G in (4, 8, 16):
                os.environ["GTNX_ASG_FULL_SCORE_GROUP"] = str(G)
                tag = f"{frames_name}_G{G}_"
                fig(name, tag + "forward_ms", lambda: 1e3 * window(lambda: tl.asg_full_score(x, tr, st, frames), sync))
                fig(name, tag + "forward_backward_ms", lambda: 1e3 * window(step, sync))
                fig(name, tag + "l2_bytes_per_frame_model", lambda: -(-B // G) * 4 * cpad * cpad)

                def kernels():
                    gtn_amd.prof_enable(True)
                    gtn_amd.prof_reset()
                    for _ in range(3):
                        step()
                    sync()
                    got = {k: gtn_amd.prof_get("asg_full_score_" + k) for k in KERNELS}
                    gtn_amd.prof_enable(False)
                    # (a step is a forward call -- prep, forward -- and a gradient call -- prep, forward, backward, ...)
                    ms = {k: v["total_ms"] / max(v["launches"], 1) for k, v in got.items()}
                    floor = 2.0 * cpad * cpad * (sum_T - B) / MFMA_F32_FLOPS * 1e3
                    return {"kernel_mean_ms": ms, "chain_us_per_frame": 1e3 * ms["forward"] / max_T,
                            "table_mfma_floor_ms": floor, "table_share_of_floor": floor / ms["table"] if ms["table"] else None}
                fig(name, tag + "kernels", kernels)
            os.environ.pop("GTNX_ASG_FULL_SCORE_GROUP")
            fig(name, f"{frames_name}_default_forward_ms",
                lambda: 1e3 * window(lambda: tl.asg_full_score(x, tr, st, frames), sync))
            fig(name, f"{frames_name}_default_forward_backward_ms", lambda: 1e3 * window(step, sync))
        # (a) the dense regime at full length
        fig(name, "a_full_connect_forward_ms", lambda: 1e3 * window(lambda: tl.asg_full_connect(x, tr, start=st), sync))

        def dense_step():
            xr, trr = x.detach().requires_grad_(True), tr.detach().requires_grad_(True)
            tl.asg_full_connect(xr, trr, start=st).sum().backward()
        fig(name, "a_full_connect_forward_backward_ms", lambda: 1e3 * window(dense_step, sync))
        # (b) the per-length fallback, sixteen utterances, scaled to the batch

        def fallback():
            x16 = x[:16].contiguous()
            sync()
            t0 = time.perf_counter()
            tl.asg_full_connect(x16, tr, start=st, input_lengths=ragged[:16])
            sync()
            return 1e3 * (time.perf_counter() - t0) * B / 16
        fig(name, "b_fallback_forward_ms_scaled", (lambda: "not measured") if skip_fallback else fallback)
        del x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--skip-fallback", action="store_true")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.skip_fallback)
    runs = []
    for i in range(a.procs):  # (fresh child processes, one after the other; the fallback in the first only)
        cmd = [sys.executable, os.path.abspath(__file__), "--child"] + (["--skip-fallback"] if a.skip_fallback or i else [])
        p = subprocess.run(cmd, capture_output=True, text=True)
        got = {}
        for line in p.stdout.splitlines():
            if line.startswith("FIG "):
                shape, key, v = json.loads(line[4:])
                got.setdefault(shape, {})[key] = v
        if p.returncode:
            got["process_failed"] = (p.stderr.strip().splitlines() or ["exit status %d" % p.returncode])[-1]
        runs.append(got)

    def merge(vals):
        vals = [v for v in vals if v is not None and v != "not measured"] or ["not measured"]
        if isinstance(vals[0], dict):
            return {k: merge([v.get(k) for v in vals if isinstance(v, dict)]) for k in vals[0]}
        nums = [v for v in vals if isinstance(v, (int, float))]
        return statistics.median(nums) if nums else vals[0]
    keys = sorted({k for r in runs for k in r})
    rec = {"tool": "tools/bench_asg_full_score.py", "processes": a.procs,
           "timing": "calls: host clock, windows >= 0.5 s, median of the processes; kernels: the engine's event timings",
           "shapes": {k: list(v) for k, v in SHAPES.items()}, "results": {k: merge([r.get(k) for r in runs]) for k in keys}}
    path = os.path.join(ROOT, "profiles", "asg_full_score_c4.json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print(json.dumps(rec["results"], indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
