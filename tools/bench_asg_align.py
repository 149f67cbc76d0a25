"""ASG frame labels on the device at BASELINE config C4's shape (B = 512, T = 1000, N = 512 labels, U = 50..100): the two ways.

  path   what a caller had before the ASG launch of Batch.viterbi_align: viterbi_path over
         compose(ems, Batch.asg_force_align(...)), the labels read from the 512 path graphs into one host array, one
         upload
  align  Batch.viterbi_align on the same product: one launch, labels, tokens and scores written into the caller's
         tensors, no copy back

    python tools/bench_asg_align.py --parent-root DIR [--out profiles/asg_align_c4.json]
        alternates `path` run from DIR (a BUILT tree of the commit to compare with, whose viterbi_align sends this
        product through the path graphs) and `align` run from this tree, three samples each, every sample a process
        of its own (two builds of the engine do not share a process) that warms its shapes up and then times windows
        of at least half a second with a host clock around a closing synchronise.  Without --parent-root `path` runs
        from this tree.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_asg_align.py --worker trace
        the new launch, and the CTC alignment launch on a CTC batch of the same T, C and U (two nodes per lane there
        as here: U <= 100 gives 101 ASG nodes; the CTC targets are cut to 63 labels = 127 nodes for equal NPL, and a
        second CTC batch keeps the full targets, NPL = 4), a few calls each, for the kernels' mean times;
    python tools/bench_asg_align.py --merge-stats DIR/.../kernel_stats.csv [--out ...]
        adds those means, and the new kernel's rate on its own byte model, to the record.

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
HBM_PEAK_GBS = 8000.0
B, T, C, UMIN, UMAX = 512, 1000, 512, 50, 100
WINDOW_S = 0.5


def inputs(torch, np):
    rng = np.random.default_rng(1234)
    targets = [rng.integers(0, C, int(rng.integers(UMIN, UMAX + 1))).astype(np.int32) for _ in range(B)]
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    em = torch.rand((B, T, C), generator=g, device="cuda", dtype=torch.float32) * 10 - 5
    tw = (torch.rand((C + C * C,), generator=g, device="cuda", dtype=torch.float32) * 2 - 1).cpu().numpy()
    return em, targets, tw


def transitions(gtn, np, tw):
    """gtn::criteria::asgTransitions(C) with weights tw: arc i = start -> label i, arc C + i C + j = j -> i"""
    g = gtn.Graph(False)
    g.add_nodes(np.array([1] + [0] * C, np.uint8), np.array([0] + [1] * C, np.uint8))
    n = np.arange(C)
    src = np.concatenate([np.zeros(C, np.int32), np.tile(n + 1, C).astype(np.int32)])
    dst = np.concatenate([n + 1, np.repeat(n + 1, C)]).astype(np.int32)
    lab = np.concatenate([n, np.repeat(n, C)]).astype(np.int32)
    g.add_arcs(src, dst, lab, lab, tw.astype(np.float32))
    g.arc_sort()
    return g


def align_bytes(targets):
    """the kernel's byte model (asg_align.hip): 4 T C + T N / 4 + 8 T per utterance, N = U + 1"""
    return float(sum(4.0 * T * C + 0.25 * T * (len(t) + 1) + 8.0 * T for t in targets))


def worker(kind, root):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import gtn_amd as gtn
    assert torch.cuda.is_available() and gtn.device_count() > 0, "bench_asg_align needs a GPU"
    assert os.path.abspath(os.path.dirname(os.path.dirname(gtn.__file__))) == os.path.abspath(root)
    em, targets, tw = inputs(torch, np)
    trans = transitions(gtn, np, tw)
    labels = torch.empty((B, T), dtype=torch.int32, device="cuda")
    tokens = torch.empty((B, T), dtype=torch.int32, device="cuda")
    scores = torch.empty((B,), dtype=torch.float32, device="cuda")
    host = torch.empty((B, T), dtype=torch.int32).pin_memory()
    host_np = host.numpy()
    lib = gtn._lib

    def product():
        ems = gtn.Batch.linear(B, T, C, em, False, True)
        return gtn.compose(ems, gtn.Batch.asg_force_align(targets, trans, C))

    def path_step():
        paths = gtn.viterbi_path(product())
        for b in range(B):  # (straight into the rows of one array: labels_to_list() without the list)
            rc = lib.gtnx_graph_labels_to_array(paths[b]._h, host_np[b].ctypes.data, 1)
            assert rc == 0
        labels.copy_(host, non_blocking=True)

    def align_step():
        product().viterbi_align(labels, tokens, scores)

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
        ctc2 = [(1 + t[:63] % (C - 1)).astype(np.int32) for t in targets]  # <= 127 nodes: two per lane, as the ASG batch
        ctc4 = [(1 + t % (C - 1)).astype(np.int32) for t in targets]       # 101 .. 201 nodes: four per lane
        for _ in range(5):
            align_step()
            sync()
            for tg in (ctc2, ctc4):
                ems = gtn.Batch.linear(B, T, C, em, False, True)
                gtn.intersect(gtn.Batch.ctc_targets(tg, 0, False), ems).viterbi_align(labels, tokens, scores)
                sync()
        print(json.dumps({"trace": "done"}))
        return
    f0, b0 = gtn.debug_align_stats()
    ms, n = timed(path_step, 1) if kind == "path" else timed(align_step, 16)
    sync()
    f1, b1 = gtn.debug_align_stats()
    print(json.dumps({"kind": kind, "ms_per_batch": ms, "iters": n, "labels_checksum": int(labels.sum().item()),
                      "algorithmic_bytes": align_bytes(targets), "launch_utterances": f1 - f0,
                      "path_graph_utterances": b1 - b0}))


def run_worker(kind, root):
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", kind, "--root", root], env=env,
                         stdout=subprocess.PIPE, timeout=500, check=True).stdout.decode()
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


def spread(v):
    return {"samples": v, "min": min(v), "max": max(v), "median": sorted(v)[len(v) // 2]}


KERNELS = (("asg_viterbi_align_kernel<2>", "asg_viterbi_align_kernel<2>"),
           ("band_viterbi_align_kernel<2>", "band_viterbi_align_kernel<2>"),
           ("band_viterbi_align_kernel<4>", "band_viterbi_align_kernel<4>"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=["path", "align", "trace"])
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--parent-root")
    ap.add_argument("--merge-stats")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "asg_align_c4.json"))
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.root)
        return
    rec = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            rec = json.load(f)
    if a.merge_stats:
        means = {}
        with open(a.merge_stats) as f:
            for row in csv.DictReader(f):
                for key, tag in KERNELS:
                    if key in row["Name"]:
                        means[tag] = {"calls": int(row["Calls"]), "mean_ms": float(row["AverageNs"]) * 1e-6,
                                      "min_ms": float(row["MinNs"]) * 1e-6, "max_ms": float(row["MaxNs"]) * 1e-6}
        rec["kernels"] = means
        k = means.get("asg_viterbi_align_kernel<2>")
        if k and rec.get("algorithmic_bytes"):
            gbs = rec["algorithmic_bytes"] / (k["mean_ms"] * 1e-3) / 1e9
            rec["align_kernel_hbm"] = {"achieved_GBs": gbs, "peak_GBs": HBM_PEAK_GBS, "frac": gbs / HBM_PEAK_GBS,
                                       "bytes": "4 T C + T N / 4 + 8 T per utterance"}
    else:
        parent = a.parent_root or HERE
        pa, al, checks = [], [], set()
        for _ in range(3):
            r = run_worker("path", parent)
            pa.append(r["ms_per_batch"])
            checks.add(r["labels_checksum"])
            r = run_worker("align", HERE)
            al.append(r["ms_per_batch"])
            checks.add(r["labels_checksum"])
            assert r["path_graph_utterances"] == 0, r
            rec["algorithmic_bytes"] = r["algorithmic_bytes"]
        rec.update({
            "shape": {"B": B, "T": T, "C": C, "U": [UMIN, UMAX]},
            "unit": "ms per batch of 512, host clock around a closing synchronise, windows >= 0.5 s",
            "path_route": dict(spread(pa), what="viterbi_path over compose(ems, Batch.asg_force_align) + labels read "
                               "from the path graphs + one upload",
                               tree="parent commit" if a.parent_root else "this tree"),
            "align_route": dict(spread(al), what="Batch.viterbi_align (labels, tokens, scores)"),
            "speedup_median": sorted(pa)[1] / sorted(al)[1],
            "speedup_worst_case": min(pa) / max(al),
            "slowest_new_faster_than_fastest_parent": max(al) < min(pa),
            "same_labels": len(checks) == 1,
        })
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
