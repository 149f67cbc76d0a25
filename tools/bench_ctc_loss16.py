"""CTC loss + backward on bfloat16 emissions at C3 (B = 512, T = 1000, C = 256, U = 100), two ways alternated in one
process: `ctc_loss(x_bf16)` -- the one-launch 16-bit step (gtn_amd/csrc/ctc_step16.hip) -- and the cast route around the
float32 path, `ctc_loss(x_bf16.float())` with the gradient cast back to bfloat16, which runs code the 16-bit step does
not touch.  With full frame counts and with ragged ones (uniform in [T/2, T]).  A pass of its own under the engine's
event profiler gives the kernel time and its rate on the 6-bytes-per-element model (read 2 forward, read 2 and write 2
backward).  Needs a GPU; writes profiles/ctc_loss16_c3.json.  The kernel's own time per launch comes from a traced
run of its own (`--worker trace`: the 16-bit call alone, full then ragged frame counts, nothing timed), merged into the
same file afterwards:

    python tools/bench_ctc_loss16.py [--reps 20] [--warmup 3] [--out profiles/ctc_loss16_c3.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_ctc_loss16.py --worker trace
    python tools/bench_ctc_loss16.py --merge-stats DIR/.../*_kernel_stats.csv [--out profiles/ctc_loss16_c3.json]
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gtn_amd as gtn  # noqa: E402
from gtn_amd.torch_loss import ctc_loss  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", type=int, nargs=4, default=[512, 1000, 256, 100], metavar=("B", "T", "C", "U"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_loss16_c3.json"))
    ap.add_argument("--worker", choices=["trace"], help="trace: run the 16-bit call alone, for a traced run")
    ap.add_argument("--merge-stats", metavar="CSV", help="add the ctc_step16 kernels of a rocprofv3 stats file to --out")
    args = ap.parse_args()
    if args.merge_stats:
        with open(args.out) as f:
            result = json.load(f)
        with open(args.merge_stats) as f:
            rows = [r for r in csv.DictReader(f) if "ctc_step16_kernel" in r["Name"]]
        result["traced_kernels"] = [{"name": r["Name"], "calls": int(r["Calls"]), "mean_ms": float(r["AverageNs"]) * 1e-6,
                                     "min_ms": float(r["MinNs"]) * 1e-6, "max_ms": float(r["MaxNs"]) * 1e-6}
                                    for r in rows]
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        return
    assert torch.cuda.is_available(), "bench_ctc_loss16.py needs a GPU"
    B, T, C, U = args.shape
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.standard_normal((B, T, C)).astype(np.float32)).to("cuda", torch.bfloat16)
    targets = rng.integers(1, C, size=(B, U)).tolist()
    ragged = rng.integers(T // 2, T + 1, size=B).tolist()

    def step16(frames):
        lp = x.detach().requires_grad_(True)
        ctc_loss(lp, targets, reduction="sum", input_lengths=frames).backward()
        return lp.grad

    def cast(frames):
        lp = x.detach().requires_grad_(True)
        ctc_loss(lp.float(), targets, reduction="sum", input_lengths=frames).backward()
        return lp.grad

    if args.worker == "trace":
        for frames in (None, ragged):
            for _ in range(args.warmup + args.reps):
                step16(frames)
        torch.cuda.synchronize()
        return

    def timed(fn, frames):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(frames)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    result = {"shape": {"B": B, "T": T, "C": C, "U": U}, "dtype": "bfloat16", "reps": args.reps, "device":
              torch.cuda.get_device_name(0)}
    for name, frames in (("full", None), ("ragged", ragged)):
        for _ in range(args.warmup):
            g16, gc = step16(frames), cast(frames)
        diff = (g16.float() - gc.float()).abs().max().item()  # (same inputs: the two routes differ by roundings)
        ms = {"step16": [], "cast": []}
        for _ in range(args.reps):  # alternated
            ms["step16"].append(timed(step16, frames))
            ms["cast"].append(timed(cast, frames))
        gtn.prof_reset()
        gtn.prof_enable(True)
        for _ in range(args.reps):
            step16(frames)
        torch.cuda.synchronize()
        gtn.synchronize()
        prof = gtn.prof_get("ctc_step16")
        total_ms, launches = prof["total_ms"], prof["launches"]
        gtn.prof_enable(False)
        kernel_ms = total_ms / args.reps  # (every launch of a call that is cut into slices)
        rows = B * T if frames is None else sum(frames)
        model_bytes = 6.0 * rows * C
        med = {k: statistics.median(v) for k, v in ms.items()}
        result[name] = {
            "step16_ms_median": med["step16"], "cast_route_ms_median": med["cast"],
            "step16_ms_min_max": [min(ms["step16"]), max(ms["step16"])],
            "cast_route_ms_min_max": [min(ms["cast"]), max(ms["cast"])],
            "cast_over_step16": med["cast"] / med["step16"],
            "kernel_ms_per_call": kernel_ms, "launches_per_call": launches / args.reps,
            "model_bytes": model_bytes, "kernel_GBps_on_6_byte_model": model_bytes / (kernel_ms * 1e-3) / 1e9,
            "max_abs_grad_difference_between_routes": diff,
        }
        print(name, json.dumps(result[name]))
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
