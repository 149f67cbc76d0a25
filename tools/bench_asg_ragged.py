"""ASG loss + backward over a PADDED batch (B = 512, T = 1000, U = 100, N = 32 and N = 128), frame counts drawn
uniformly from [T / 2, T] with a fixed seed: four ways.

  ragged    (a) torch_loss.asg_loss(em, trans, targets, input_lengths=frames) + backward: the full-connect term is the
            one launch each way of asg_full.hip
  full      (b) the same tensors at full length, input_lengths=None: the dense regime's launch per frame (more work:
            context, not a comparison of routes)
  full_fc   (c) the same at full length under GTNX_FULL_CONNECT=1: identical work to (b) on the new launch
  per_utt   (d) what a caller had before input_lengths: one asg_loss call per utterance on em[b:b+1, :T_b], run from a
            BUILT tree of the commit to compare with (--parent-root), over the first --per-utt-batch utterances and
            scaled to B (it runs for seconds: said in the record)

    python tools/bench_asg_ragged.py [--labels 32 128] [--parent-root DIR] [--out profiles/asg_ragged.json]
        alternates the four per alphabet, every sample a process of its own that warms its shapes up and then times
        windows of at least half a second with a host clock around a closing synchronise.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_asg_ragged.py --worker trace --n-labels 128
        a few ragged steps of THIS tree for the kernels' mean times;
    python tools/bench_asg_ragged.py --merge-stats DIR/.../kernel_stats.csv --n-labels 128 [--out ...]
        adds those means, the time per frame-step they imply (mean / mean T_b: one workgroup walks one utterance, so
        that is the latency of one step, barriers included) and writes the rows next to the record (.csv).

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
B, T, U = 512, 1000, 100
WINDOW_S = 0.5
KERNELS = ("asg_full_forward_kernel", "asg_full_backward_kernel", "asg_full_reduce_kernel", "pad_fill_kernel",
           "band_forward_kernel", "band_backward_kernel", "lazy_mfma")


def inputs(torch, np, N):
    rng = np.random.default_rng(4321)
    targets = [rng.integers(0, N, U).astype(np.int32).tolist() for _ in range(B)]
    frames = rng.integers(T // 2, T + 1, B).astype(np.int32)
    g = torch.Generator(device="cuda")
    g.manual_seed(4321)
    em = torch.randn((B, T, N), generator=g, device="cuda", dtype=torch.float32)
    trans = torch.randn((N, N), generator=g, device="cuda", dtype=torch.float32)
    start = torch.randn((N,), generator=g, device="cuda", dtype=torch.float32)
    return em, trans, start, targets, frames


def worker(kind, root, N, per_utt_batch):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import gtn_amd as gtn
    import gtn_amd.torch_loss as tl
    assert torch.cuda.is_available() and gtn.device_count() > 0, "bench_asg_ragged needs a GPU"
    assert os.path.abspath(os.path.dirname(os.path.dirname(gtn.__file__))) == os.path.abspath(root)
    assert tl._native(), "gtn_amd/lib/libgtn_criteria.so missing (build())"
    if kind == "full_fc":
        assert os.environ.get("GTNX_FULL_CONNECT") == "1"
    em, trans, start, targets, frames = inputs(torch, np, N)
    em.requires_grad_(True), trans.requires_grad_(True), start.requires_grad_(True)
    flist = [int(f) for f in frames]
    last = {}

    def step(lengths):
        em.grad = trans.grad = start.grad = None
        loss = tl.asg_loss(em, trans, targets, start=start, reduction="sum", input_lengths=lengths)
        loss.backward()
        last["loss"] = loss

    views = None

    def per_utt_step():
        tot = 0.0
        for b in range(per_utt_batch):
            x = views[b]
            x.grad = trans.grad = start.grad = None
            loss = tl.asg_loss(x, trans, [targets[b]], start=start, reduction="sum")
            loss.backward()
            tot = loss + tot
        last["loss"] = tot

    def sync():
        gtn.synchronize()
        torch.cuda.synchronize()

    def timed(fn, chunk):
        for _ in range(2):
            fn()
        sync()
        n, t0 = 0, time.perf_counter()
        while True:
            for _ in range(chunk):
                fn()
            sync()
            n += chunk
            dt = time.perf_counter() - t0
            if dt >= WINDOW_S:
                return dt / n * 1e3, n

    if kind == "trace":
        for _ in range(5):
            step(frames)
            sync()
        print(json.dumps({"trace": "done"}))
        return
    rec = {"kind": kind, "N": N}
    if kind == "per_utt":
        views = [em.detach()[b:b + 1, :flist[b]].clone().requires_grad_(True) for b in range(per_utt_batch)]
        ms, n = timed(per_utt_step, 1)
        ms *= B / per_utt_batch
        rec["utterances_timed"] = per_utt_batch
    elif kind == "ragged":
        s0 = gtn.debug_full_connect_stats() if hasattr(gtn, "debug_full_connect_stats") else None
        ms, n = timed(lambda: step(frames), 2)
        if s0 is not None:
            s1 = gtn.debug_full_connect_stats()
            rec["full_connect_stats_delta"] = [s1[0] - s0[0], s1[1] - s0[1]]
    else:
        ms, n = timed(lambda: step(None), 2)
    sync()
    rec.update({"ms_per_step": ms, "iters": n, "loss": float(last["loss"].item()), "mean_frames": float(frames.mean())})
    print(json.dumps(rec))


def run_worker(kind, root, N, per_utt_batch):
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    env.pop("GTNX_FULL_CONNECT", None)
    if kind == "full_fc":
        env["GTNX_FULL_CONNECT"] = "1"
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", kind, "--root", root, "--n-labels", str(N),
                          "--per-utt-batch", str(per_utt_batch)], env=env, stdout=subprocess.PIPE, timeout=900,
                         check=True).stdout.decode()
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


def spread(v):
    return {"samples": v, "min": min(v), "max": max(v), "median": sorted(v)[len(v) // 2]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=["ragged", "full", "full_fc", "per_utt", "trace"])
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--n-labels", type=int, default=128)
    ap.add_argument("--labels", type=int, nargs="*", default=[32, 128])
    ap.add_argument("--parent-root")
    ap.add_argument("--per-utt-batch", type=int, default=16)
    ap.add_argument("--merge-stats")
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "asg_ragged.json"))
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.root, a.n_labels, a.per_utt_batch)
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
        key = f"N{a.n_labels}"
        mean_frames = rec.get(key, {}).get("mean_frames", 0.75 * T)
        for r in rows:
            if "asg_full_forward" in r["name"] or "asg_full_backward" in r["name"]:
                # (B <= the workgroups resident at once is assumed: the kernel's time is its longest utterance's, T steps)
                r["us_per_frame_step_upper"] = r["mean_ms"] * 1e3 / mean_frames
                r["us_per_frame_step_lower"] = r["mean_ms"] * 1e3 / T
        rec.setdefault(key, {})["kernels"] = rows
        with open(os.path.splitext(a.out)[0] + ".csv", "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=["name", "calls", "mean_ms", "min_ms", "max_ms", "total_ms",
                                              "us_per_frame_step_upper", "us_per_frame_step_lower"])
            w.writeheader()
            w.writerows(rows)
    else:
        parent = a.parent_root or HERE
        for N in a.labels:
            ra, fu, fc, pu = [], [], [], []
            r = {}
            for _ in range(a.samples):
                r = run_worker("ragged", HERE, N, a.per_utt_batch)
                ra.append(r["ms_per_step"])
                fu.append(run_worker("full", HERE, N, a.per_utt_batch)["ms_per_step"])
                fc.append(run_worker("full_fc", HERE, N, a.per_utt_batch)["ms_per_step"])
                pu.append(run_worker("per_utt", parent, N, a.per_utt_batch)["ms_per_step"])
            med = lambda v: sorted(v)[len(v) // 2]
            rec[f"N{N}"] = {
                "shape": {"B": B, "T": T, "N": N, "U": U, "frames": "uniform in [T/2, T], seed 4321"},
                "mean_frames": r.get("mean_frames"),
                "full_connect_stats_delta": r.get("full_connect_stats_delta"),
                "unit": "ms per step (loss + backward) of 512 utterances, host clock around a closing synchronise, "
                        "windows >= 0.5 s",
                "a_ragged": dict(spread(ra), what="asg_loss(input_lengths=frames) + backward"),
                "b_full": dict(spread(fu), what="the same tensors, input_lengths=None, + backward (existing route)"),
                "c_full_new_route": dict(spread(fc), what="as (b) under GTNX_FULL_CONNECT=1"),
                "d_per_utterance": dict(spread(pu), what="one asg_loss call per utterance on em[b:b+1, :T_b] + backward, "
                                        f"{a.per_utt_batch} utterances timed and scaled to {B}",
                                        tree="parent commit" if a.parent_root else "this tree"),
                "c_over_b_median": med(fc) / med(fu),
                "a_over_b_median": med(ra) / med(fu),
                "d_over_a_median": med(pu) / med(ra),
            }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
