"""ASG posterior sampling with the results on the device at BASELINE config C4's shape (B = 512, T = 1000, C = 512) with
N = 4 and N = 16 samples per utterance, and at a letter alphabet (C = 32, same B and T).

There was no route for this call before Batch.asg_sample, so no speed-up is claimed.  What is reported:

  call     Batch.asg_sample (tokens, lengths, logq, logz), three samples per (shape, N), every sample a process of its own
           that warms its shapes up and then times windows of at least half a second with a host clock around a closing
           synchronise
  kernels  from `rocprofv3 --kernel-trace --stats` in a run of its own: the filter, the draw, the collapse and the prep
           launch; the draw's microseconds per frame of its serial chain; beside the filter the shipped full-connect
           forward on the same tensor (asg_loss's forward: asg_full_forward_kernel at C = 32, the dense-regime forward
           sweep at C = 512), the one existing kernel that does the same arithmetic
  host     for scale only: forward filtering, backward sampling in numpy (float64, scaled, matrix-vector products) on a
           few utterances, EXTRAPOLATED to the batch and labelled as such

    python tools/bench_asg_sample.py [--out profiles/asg_sample_c4.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_asg_sample.py --worker trace:c4:4
        (and trace:c4:16, trace:letters:4) a few calls of the sampler and of asg_loss's forward;
    python tools/bench_asg_sample.py --merge-stats DIR/.../kernel_stats.csv --cfg c4 --n 4 [--out ...]
        adds the kernels' mean times to the record.

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
B, T = 512, 1000
SHAPES = {"c4": 512, "letters": 32}
WINDOW_S = 0.5
SEED = 1234
HOST_UTTERANCES = 2


def inputs(torch, C):
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    em = torch.log_softmax(torch.rand((B, T, C), generator=g, device="cuda", dtype=torch.float32) * 10 - 5, dim=2)
    tr = torch.randn((C, C), generator=g, device="cuda", dtype=torch.float32)
    tr += torch.eye(C, device="cuda") * 2.0  # (labels last a few frames: the collapse has work)
    st = torch.zeros(C, device="cuda", dtype=torch.float32)
    return em.contiguous(), tr.contiguous(), st


def host_ffbs(np, em, start, W, N, rng):
    """forward filtering, backward sampling of one utterance in numpy float64 (scaled probabilities)"""
    Tn, C = em.shape
    E = np.exp(W - W.max())
    q = np.empty((Tn, C))
    a = np.exp(start + em[0] - (start + em[0]).max())
    q[0] = a / a.sum()
    for t in range(1, Tn):
        a = (E @ q[t - 1]) * np.exp(em[t] - em[t].max())
        q[t] = a / a.sum()
    lab = np.empty((N, Tn), np.int64)
    for k in range(N):
        p = q[Tn - 1]
        for t in range(Tn - 1, -1, -1):
            if t < Tn - 1:
                p = q[t] * E[lab[k, t + 1]]
            c = np.cumsum(p)
            lab[k, t] = min(int(np.searchsorted(c, rng.random() * c[-1], side="right")), C - 1)
    return lab


def worker(spec):
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    import gtn_amd as gtn
    from gtn_amd import torch_loss
    assert torch.cuda.is_available() and gtn.device_count() > 0, "bench_asg_sample needs a GPU"
    kind, cfg, N = spec.split(":")
    C, N = SHAPES[cfg], int(N)
    em, tr, st = inputs(torch, C)
    if kind == "host":
        rng = np.random.default_rng(1)
        x, W, s = em[:HOST_UTTERANCES].cpu().numpy().astype(np.float64), tr.cpu().numpy().astype(np.float64), \
            st.cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        for b in range(HOST_UTTERANCES):
            host_ffbs(np, x[b], s, W, N, rng)
        per = (time.perf_counter() - t0) / HOST_UTTERANCES
        print(json.dumps({"kind": kind, "cfg": cfg, "N": N, "utterances_measured": HOST_UTTERANCES,
                          "s_per_utterance": per, "ms_per_batch_EXTRAPOLATED": per * B * 1e3}))
        return
    table = torch_loss._asg_weights(st, tr)
    tokens = torch.empty((B, N, T), dtype=torch.int32, device="cuda")
    lengths = torch.empty((B, N), dtype=torch.int32, device="cuda")
    logq = torch.empty((B, N), dtype=torch.float32, device="cuda")
    logz = torch.empty((B,), dtype=torch.float32, device="cuda")
    calls = [0]

    def sample_step():
        calls[0] += 1
        ems = gtn.Batch.linear(B, T, C, em, False, True)
        ems.asg_sample(tokens, lengths, table, logq, None, logz, None, N, SEED + calls[0], 1.0)

    def sync():
        gtn.synchronize()
        torch.cuda.synchronize()

    if kind == "trace":
        targets = [[1]] * B
        for _ in range(3):
            sample_step()
            sync()
            # (forward only: the full-connect forward on the same tensor; frame counts, all T, take the one-launch
            #  asg_full_forward_kernel up to 128 labels, where the call without them composes a graph)
            torch_loss.asg_loss(em, tr, targets, st, input_lengths=[T] * B if C <= 128 else None)
            sync()
        print(json.dumps({"trace": "done"}))
        return
    for _ in range(2):
        sample_step()
    sync()
    c0, u0 = gtn.debug_asg_sample_stats()
    n, t0 = 0, time.perf_counter()
    while True:
        sample_step()
        sync()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= WINDOW_S:
            break
    c1, u1 = gtn.debug_asg_sample_stats()
    print(json.dumps({"kind": kind, "cfg": cfg, "N": N, "utterances": B, "ms_per_batch": dt / n * 1e3, "iters": n,
                      "mean_length": float(lengths.float().mean().item()),
                      "logz_finite": bool(torch.isfinite(logz).all().item()), "sampled_utterances": u1 - u0}))


def run_worker(spec):
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", spec], env=env,
                         stdout=subprocess.PIPE, timeout=500, check=True).stdout.decode()
    rec = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    print(f"[bench_asg_sample] {spec}: {rec}", file=sys.stderr, flush=True)
    return rec


def spread(v):
    return {"samples": v, "min": min(v), "max": max(v), "median": sorted(v)[len(v) // 2]}


RUNS = [("c4", 4), ("c4", 16), ("letters", 4)]
KERNELS = ("asg_sample_prep_kernel", "asg_sample_filter_kernel", "asg_sample_filter_wide_kernel",
           "asg_sample_draw_kernel", "asg_sample_collapse_kernel", "asg_full_forward_kernel")
DENSE = ("lazy_mfma", "lazy_dense")  # the dense-regime forward sweep's kernels (one launch per frame)
# what asg_loss's forward runs instead where it composes emissions o transitions as a graph (full-length batches of a
# letter alphabet): the compose kernels and the built-graph forward sweep
COMPOSED = ("sd_forward_kernel", "tr_scatter_kernel", "tr_count_kernel", "tr_offsets_kernel", "tr_chunk_", "compose_wide_")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker")
    ap.add_argument("--merge-stats")
    ap.add_argument("--cfg", choices=sorted(SHAPES))
    ap.add_argument("--n", type=int)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "asg_sample_c4.json"))
    a = ap.parse_args()
    if a.worker:
        worker(a.worker)
        return
    rec = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            rec = json.load(f)
    if a.merge_stats:
        assert a.cfg and a.n, "--merge-stats needs --cfg and --n"
        means, dense_total_ns, composed_total_ns, traced_calls = {}, 0.0, 0.0, 3
        with open(a.merge_stats) as f:
            for row in csv.DictReader(f):
                for key in KERNELS:
                    if key + "<" in row["Name"] or key + "(" in row["Name"] or row["Name"].endswith(key):
                        e = means.setdefault(key, {"calls": 0, "total_ms": 0.0})
                        e["calls"] += int(row["Calls"])
                        e["total_ms"] += float(row["AverageNs"]) * int(row["Calls"]) * 1e-6
                if any(d in row["Name"] for d in DENSE):
                    dense_total_ns += float(row["AverageNs"]) * int(row["Calls"])
                if any(d in row["Name"] for d in COMPOSED):
                    composed_total_ns += float(row["AverageNs"]) * int(row["Calls"])
        for e in means.values():
            e["mean_ms"] = e["total_ms"] / e["calls"]
            e["ms_per_sampler_call"] = e["total_ms"] / traced_calls
        sec = rec.setdefault(f"{a.cfg} N={a.n}", {})
        sec["kernels"] = means
        if dense_total_ns:
            sec["dense_regime_forward_ms_per_call"] = dense_total_ns * 1e-6 / traced_calls
        if composed_total_ns:
            sec["composed_route_forward_ms_per_call"] = composed_total_ns * 1e-6 / traced_calls
        d = means.get("asg_sample_draw_kernel")
        if d:
            sec["draw_us_per_frame_of_its_serial_chain"] = d["mean_ms"] * 1e3 / T
            sec["draw_note"] = "of one launch; a sampler call launches the draw once per scratch slice, one after the other"
    else:
        for cfg, n in RUNS:
            ms, lens = [], []
            for _ in range(3):
                r = run_worker(f"sample:{cfg}:{n}")
                ms.append(r["ms_per_batch"])
                lens.append(r["mean_length"])
                assert r["sampled_utterances"] > 0 and r["logz_finite"], r
            sec = rec.setdefault(f"{cfg} N={n}", {})
            sec.update({"call": dict(spread(ms), what="Batch.asg_sample (tokens, lengths, logq, logz)", utterances=B),
                        "mean_collapsed_length": {"min": min(lens), "max": max(lens)}})
        for cfg in ("c4", "letters"):
            r = run_worker(f"host:{cfg}:4")
            rec.setdefault(f"{cfg} N=4", {})["host_numpy_ffbs_for_scale_only"] = r
        rec.update({"shapes": {"B": B, "T": T, "C": SHAPES},
                    "unit": "ms per batch, host clock around a closing synchronise, windows >= 0.5 s"})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
