"""ASG Viterbi decode with the results on the device at BASELINE config C4's shape (B = 512, T = 1000, N = 512 labels):
the two ways, at full length and with per-utterance frame counts uniform in [T / 2, T].

  path    what a caller had before Batch.viterbi_decode: viterbi_path over compose(ems, [transitions]) (symbolic: the
          max-plus sweeps + one back-trace per utterance), the labels read from the path graphs into one host array,
          one upload.  With frame counts the chains come from Batch.linear(rows=): one group -- one chain of T_b
          launches -- per distinct length, so that route is timed at RAGGED_PARENT_B utterances only
  decode  Batch.viterbi_decode: one sweep of the padded batch, one launch, labels / scores / collapsed sequences /
          lengths written into the caller's tensors, no copy back

    python tools/bench_asg_decode.py --parent-root DIR [--out profiles/asg_decode_c4.json]
        alternates `path` run from DIR (a BUILT tree of the commit to compare with, which has no viterbi_decode) and
        `decode` run from this tree, three samples each, every sample a process of its own (two builds of the engine
        do not share a process) that warms its shapes up and then times windows of at least half a second with a host
        clock around a closing synchronise; then the same for the ragged batch.  Without --parent-root `path` runs
        from this tree.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_asg_decode.py --worker trace
        a few calls of each route at full length, for the mean times of asg_decode_kernel and maxplus_path_kernel (and
        of the sweep's step kernel);
    python tools/bench_asg_decode.py --merge-stats DIR/.../kernel_stats.csv [--out ...]
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
B, T, C = 512, 1000, 512
RAGGED_PARENT_B = 32  # the parent's ragged route costs one chain of launches per distinct length
WINDOW_S = 0.5


def inputs(torch, np, nb):
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    em = torch.rand((nb, T, C), generator=g, device="cuda", dtype=torch.float32) * 10 - 5
    tw = (torch.rand((C + C * C,), generator=g, device="cuda", dtype=torch.float32) * 2 - 1).cpu().numpy()
    frames = np.random.default_rng(1234).integers(T // 2, T + 1, nb).astype(np.int32)
    return em, tw, frames


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


def decode_bytes(frames):
    """the back-trace's byte model (asg_decode.hip): per frame one alpha row (4 N', N' = C + 1 nodes), one emission row
    (4 C) and the visited node's in-row (16 B x (C + 1) records); 4 T of labels out, 4 T_b + 4 T for the collapsed pass"""
    return float(sum(f * (4.0 * (C + 1) + 4.0 * C + 16.0 * (C + 1)) + 4.0 * T + 4.0 * f + 4.0 * T for f in frames))


def worker(kind, root):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import gtn_amd as gtn
    assert torch.cuda.is_available() and gtn.device_count() > 0, "bench_asg_decode needs a GPU"
    assert os.path.abspath(os.path.dirname(os.path.dirname(gtn.__file__))) == os.path.abspath(root)
    ragged = kind.endswith("_ragged") or kind.endswith("_ragged_small")
    nb = RAGGED_PARENT_B if kind in ("path_ragged", "decode_ragged_small") else B
    em, tw, frames = inputs(torch, np, nb)
    if not ragged:
        frames = np.full(nb, T, np.int32)
    trans = transitions(gtn, np, tw)
    labels = torch.empty((nb, T), dtype=torch.int32, device="cuda")
    collapsed = torch.empty((nb, T), dtype=torch.int32, device="cuda")
    scores = torch.empty((nb,), dtype=torch.float32, device="cuda")
    lengths = torch.empty((nb,), dtype=torch.int32, device="cuda")
    host = torch.full((nb, T), -1, dtype=torch.int32).pin_memory()
    host_np = host.numpy()
    lib = gtn._lib
    gtn.compose_mode(1)  # the product stays symbolic (262 M arcs per utterance otherwise)

    def path_step():
        ems = gtn.Batch.linear(nb, T, C, em, False, True, frames.tolist() if ragged else None)
        paths = gtn.viterbi_path(gtn.compose([ems[b] for b in range(nb)], [trans]))
        for b in range(nb):  # (straight into the rows of one array: labels_to_list() without the list)
            rc = lib.gtnx_graph_labels_to_array(paths[b]._h, host_np[b].ctypes.data, 1)
            assert rc == 0
        labels.copy_(host, non_blocking=True)

    def decode_step():
        ems = gtn.Batch.linear(nb, T, C, em, False, True)
        ems.viterbi_decode(trans, labels, scores, frames if ragged else None, collapsed, lengths)

    def sync():
        gtn.synchronize()
        torch.cuda.synchronize()

    def timed(step):
        for _ in range(3):
            step()
        sync()
        n, t0 = 0, time.perf_counter()
        while True:
            step()
            sync()
            n += 1
            dt = time.perf_counter() - t0
            if dt >= WINDOW_S:
                return dt / n * 1e3, n

    if kind == "trace":
        for _ in range(3):
            decode_step()
            sync()
            path_step()
            sync()
        print(json.dumps({"trace": "done"}))
        return
    is_decode = kind.startswith("decode")
    stats = getattr(gtn, "debug_decode_stats", None)
    f0, b0 = stats() if stats else (0, 0)
    ms, n = timed(decode_step if is_decode else path_step)
    sync()
    f1, b1 = stats() if stats else (0, 0)
    print(json.dumps({"kind": kind, "utterances": nb, "ms_per_batch": ms, "iters": n,
                      "labels_checksum": int(labels.to(torch.int64).sum().item()),
                      "algorithmic_bytes": decode_bytes(frames.tolist()), "launch_utterances": f1 - f0,
                      "path_graph_utterances": b1 - b0}))


def run_worker(kind, root):
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", kind, "--root", root], env=env,
                         stdout=subprocess.PIPE, timeout=500, check=True).stdout.decode()
    rec = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    print(f"[bench_asg_decode] {kind}: {rec['ms_per_batch']:.3f} ms per batch of {rec['utterances']}", file=sys.stderr,
          flush=True)
    return rec


def spread(v):
    return {"samples": v, "min": min(v), "max": max(v), "median": sorted(v)[len(v) // 2]}


KERNELS = (("asg_decode_kernel", "asg_decode_kernel"), ("maxplus_path_kernel", "maxplus_path_kernel"),
           ("maxplus_step_kernel", "maxplus_step_kernel"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=["path", "decode", "path_ragged", "decode_ragged", "decode_ragged_small", "trace"])
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--parent-root")
    ap.add_argument("--merge-stats")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "asg_decode_c4.json"))
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
        k = means.get("asg_decode_kernel")
        if k and rec.get("algorithmic_bytes"):
            gbs = rec["algorithmic_bytes"] / (k["mean_ms"] * 1e-3) / 1e9
            rec["decode_kernel_on_its_byte_model"] = {
                "achieved_GBs": gbs, "peak_GBs": HBM_PEAK_GBS, "frac": gbs / HBM_PEAK_GBS,
                "bytes": "T_b (4 N' + 4 C + 16 N') + 4 T + (4 T_b + 4 T) per utterance, N' = C + 1"}
    else:
        parent = a.parent_root or HERE
        tree = "parent commit" if a.parent_root else "this tree"
        pa, de, checks = [], [], set()
        for _ in range(3):
            r = run_worker("path", parent)
            pa.append(r["ms_per_batch"])
            checks.add(r["labels_checksum"])
            r = run_worker("decode", HERE)
            de.append(r["ms_per_batch"])
            checks.add(r["labels_checksum"])
            assert r["path_graph_utterances"] == 0, r
            rec["algorithmic_bytes"] = r["algorithmic_bytes"]
        rp, rd, rs, rchecks = [], [], [], set()
        for _ in range(3):
            r = run_worker("path_ragged", parent)
            rp.append(r["ms_per_batch"])
            rchecks.add(r["labels_checksum"])
            r = run_worker("decode_ragged_small", HERE)
            rs.append(r["ms_per_batch"])
            rchecks.add(r["labels_checksum"])
            assert r["path_graph_utterances"] == 0, r
            r = run_worker("decode_ragged", HERE)
            rd.append(r["ms_per_batch"])
            assert r["path_graph_utterances"] == 0, r
        rec.update({
            "shape": {"B": B, "T": T, "C": C},
            "unit": "ms per batch, host clock around a closing synchronise, windows >= 0.5 s",
            "full_length": {
                "path_route": dict(spread(pa), what="viterbi_path over compose(ems, [transitions]) + labels read from "
                                   "the path graphs + one upload", tree=tree, utterances=B),
                "decode_route": dict(spread(de), what="Batch.viterbi_decode (labels, scores, collapsed, lengths)",
                                     utterances=B),
                "speedup_median": sorted(pa)[1] / sorted(de)[1],
                "slowest_new_not_slower_than_fastest_parent": max(de) <= min(pa),
                "same_labels": len(checks) == 1,
            },
            "frames_uniform_in_half_T_to_T": {
                "path_route": dict(spread(rp), what="the same over the elements of Batch.linear(rows=): one group per "
                                   "distinct length", tree=tree, utterances=RAGGED_PARENT_B),
                "decode_route_same_batch": dict(spread(rs), what="Batch.viterbi_decode(frames=)",
                                                utterances=RAGGED_PARENT_B),
                "decode_route": dict(spread(rd), what="Batch.viterbi_decode(frames=)", utterances=B),
                "same_labels_at_the_small_batch": len(rchecks) == 1,
            },
        })
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
