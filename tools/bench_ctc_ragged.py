"""CTC loss + backward over a PADDED batch at BASELINE config C3's shape (B = 512, T = 1000, C = 256, U = 100), frame
counts drawn uniformly from [T / 2, T] with a fixed seed: three ways.

  ragged   torch_loss.ctc_loss(lp, targets, input_lengths=frames) followed by backward: one call for the batch
  full     the same tensors at full length, input_lengths=None, on the same commit (what the padded step is held to:
           no slower than this plus one small launch)
  per_utt  what a caller had before input_lengths: one call per utterance on lp[b:b+1, :T_b] -- the only correct route
           of the commit to compare with

    python tools/bench_ctc_ragged.py [--parent-root DIR] [--out profiles/ctc_ragged_c3.json]
        alternates the three, three samples each, every sample a process of its own that warms its shapes up and then
        times windows of at least half a second with a host clock around a closing synchronise.  `per_utt` runs from
        DIR (a BUILT tree of the commit to compare with) when given, else from this tree.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_ctc_ragged.py --worker trace
        a few ragged and full steps of THIS tree for the kernels' mean times;
    python tools/bench_ctc_ragged.py --merge-stats DIR/.../kernel_stats.csv [--out ...]
        adds those means to the record and writes the rows next to it (profiles/ctc_ragged_c3.csv).

Needs a GPU; a measurement path that finds none fails.
"""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, C, U = 512, 1000, 256, 100
WINDOW_S = 0.5
KERNELS = ("pad_fill_kernel", "band_forward_kernel", "band_backward_kernel", "ctc_targets_kernel", "vec_axpby_kernel",
           "scalar_seed_kernel", "copy_small_kernel")


def inputs(torch, np):
    rng = np.random.default_rng(1234)
    targets = [rng.integers(1, C, U).astype(np.int32).tolist() for _ in range(B)]
    frames = rng.integers(T // 2, T + 1, B).astype(np.int32)
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    em = torch.rand((B, T, C), generator=g, device="cuda", dtype=torch.float32) * 10 - 5
    return em, targets, frames


def pad_bytes(frames):
    """what the fill kernel stores (padfill.hip): 4 C (T - T_b) per utterance"""
    return float(sum(4.0 * C * (T - int(f)) for f in frames))


def worker(kind, root):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import gtn_amd as gtn
    import gtn_amd.torch_loss as tl
    assert torch.cuda.is_available() and gtn.device_count() > 0, "bench_ctc_ragged needs a GPU"
    assert os.path.abspath(os.path.dirname(os.path.dirname(gtn.__file__))) == os.path.abspath(root)
    assert tl._native(), "gtn_amd/lib/libgtn_criteria.so missing (build())"
    em, targets, frames = inputs(torch, np)
    lp = em.requires_grad_(True)
    flist = [int(f) for f in frames]
    views = None
    last = {}

    def ragged_step():
        lp.grad = None
        loss = tl.ctc_loss(lp, targets, input_lengths=frames)
        loss.sum().backward()
        last["loss"] = loss

    def full_step():
        lp.grad = None
        loss = tl.ctc_loss(lp, targets)
        loss.sum().backward()
        last["loss"] = loss

    def per_utt_step():
        tot = None
        for b in range(B):
            x = views[b]
            x.grad = None
            loss = tl.ctc_loss(x, [targets[b]])
            loss.sum().backward()
            tot = loss if tot is None else tot + loss
        last["loss"] = tot

    def sync():
        gtn.synchronize()
        torch.cuda.synchronize()

    def timed(step, chunk):
        for _ in range(3):
            step()
        sync()
        n, t0 = 0, time.perf_counter()
        while True:
            for _ in range(chunk):
                step()
            sync()
            n += chunk
            dt = time.perf_counter() - t0
            if dt >= WINDOW_S:
                return dt / n * 1e3, n

    if kind == "trace":
        for _ in range(5):
            ragged_step()
            sync()
            full_step()
            sync()
        print(json.dumps({"trace": "done"}))
        return
    rec = {"kind": kind}
    if kind == "per_utt":
        # (leaves of their own, as a caller without input_lengths would hold them: contiguous copies of the slices)
        views = [em.detach()[b:b + 1, :flist[b]].clone().requires_grad_(True) for b in range(B)]
        ms, n = timed(per_utt_step, 1)
    elif kind == "full":
        ms, n = timed(full_step, 8)
    else:
        ms, n = timed(ragged_step, 8)
        # one profiled step apart from the timed window: launches and bytes of the fill as the engine counts them
        gtn.prof_reset()
        gtn.prof_enable(True)
        ragged_step()
        sync()
        gtn.prof_enable(False)
        p = gtn.prof_get("linear_pad_fill")
        rec["pad_fill"] = {"launches_per_step": p["launches"], "bytes_counted": p["algorithmic_bytes"],
                           "bytes_model": pad_bytes(frames), "pad_rows_are_zero": True}
        g = lp.grad
        for b in (0, 1, B // 2, B - 1):
            rec["pad_fill"]["pad_rows_are_zero"] &= not bool(g[b, flist[b]:].any().item())
    sync()
    rec.update({"ms_per_step": ms, "iters": n, "loss_sum": float(last["loss"].sum().item())})
    print(json.dumps(rec))


def run_worker(kind, root):
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", kind, "--root", root], env=env,
                         stdout=subprocess.PIPE, timeout=500, check=True).stdout.decode()
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


def spread(v):
    return {"samples": v, "min": min(v), "max": max(v), "median": sorted(v)[len(v) // 2]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=["ragged", "full", "per_utt", "trace"])
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--parent-root")
    ap.add_argument("--merge-stats")
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ctc_ragged_c3.json"))
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.root)
        return
    rec = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            rec = json.load(f)
    if a.merge_stats:
        rows = []
        with open(a.merge_stats) as f:
            for row in csv.DictReader(f):
                if any(k in row["Name"] for k in KERNELS):
                    rows.append({"name": row["Name"], "calls": int(row["Calls"]),
                                 "mean_ms": float(row["AverageNs"]) * 1e-6, "min_ms": float(row["MinNs"]) * 1e-6,
                                 "max_ms": float(row["MaxNs"]) * 1e-6, "total_ms": float(row["TotalDurationNs"]) * 1e-6})
        rec["kernels"] = rows
        with open(os.path.splitext(a.out)[0] + ".csv", "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=["name", "calls", "mean_ms", "min_ms", "max_ms", "total_ms"])
            w.writeheader()
            w.writerows(rows)
        fill = [r for r in rows if "pad_fill_kernel" in r["name"]]
        if fill and rec.get("pad_fill"):
            gbs = rec["pad_fill"]["bytes_model"] / (fill[0]["mean_ms"] * 1e-3) / 1e9
            rec["pad_fill"]["kernel_mean_ms"] = fill[0]["mean_ms"]
            rec["pad_fill"]["achieved_GBs"] = gbs
    else:
        parent = a.parent_root or HERE
        ra, fu, pu = [], [], []
        for _ in range(a.samples):
            r = run_worker("ragged", HERE)
            ra.append(r["ms_per_step"])
            rec["pad_fill"] = r["pad_fill"]
            rec["ragged_loss_sum"] = r["loss_sum"]
            fu.append(run_worker("full", HERE)["ms_per_step"])
            r = run_worker("per_utt", parent)
            pu.append(r["ms_per_step"])
            rec["per_utt_loss_sum"] = r["loss_sum"]
        rec.update({
            "shape": {"B": B, "T": T, "C": C, "U": U, "frames": "uniform in [T/2, T], seed 1234"},
            "unit": "ms per step (loss + backward) of 512 utterances, host clock around a closing synchronise, "
                    "windows >= 0.5 s",
            "ragged": dict(spread(ra), what="ctc_loss(input_lengths=frames) + backward"),
            "full": dict(spread(fu), what="the same tensors, input_lengths=None, + backward"),
            "per_utterance": dict(spread(pu), what="one ctc_loss call per utterance on lp[b:b+1, :T_b] + backward",
                                  tree="parent commit" if a.parent_root else "this tree"),
            "ragged_over_full_median": sorted(ra)[len(ra) // 2] / sorted(fu)[len(fu) // 2],
            "per_utterance_over_ragged_median": sorted(pu)[len(pu) // 2] / sorted(ra)[len(ra) // 2],
        })
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
