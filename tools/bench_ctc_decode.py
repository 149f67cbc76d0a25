"""CTC best-path decode with the results on the device at BASELINE config C3's shape (B = 512, T = 1000, C = 256):
the two ways, at full length and with per-utterance frame counts uniform in [T / 2, T].

  path    what a caller had before Batch.linear_decode: viterbi_path over the Batch.linear (the elements materialised,
          one path graph per utterance), the labels read from the path graphs into one host array, the CTC collapse on
          the host (numpy), one upload of labels / tokens / starts / lengths.  No scores (the caller would add the path
          weights up as well: this route is given that for free).  With frame counts the chains come from
          Batch.linear(rows=)
  decode  Batch.linear_decode: two launches, labels / scores / tokens / starts / lengths written into the caller's
          tensors, no copy back

    python tools/bench_ctc_decode.py --parent-root DIR [--out profiles/ctc_decode_c3.json]
        alternates `path` run from DIR (a BUILT tree of the commit to compare with, which has no linear_decode) and
        `decode` run from this tree, three samples each, every sample a process of its own (two builds of the engine
        do not share a process) that warms its shapes up and then times windows of at least half a second with a host
        clock around a closing synchronise; then the same for the ragged batch.  Without --parent-root `path` runs
        from this tree.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_ctc_decode.py --worker trace
        a few calls of `decode` at full length, for the mean times of the two kernels;
    python tools/bench_ctc_decode.py --merge-stats DIR/.../kernel_stats.csv [--out ...]
        adds those means, and the kernels' rates on their own byte model beside the stream-rate floor, to the record.

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
STREAM_GBS = 6300.0  # the achievable HBM stream rate the floor is derived from
B, T, C = 512, 1000, 256
BLANK = 0
WINDOW_S = 0.5


def inputs(torch, np):
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    em = torch.rand((B, T, C), generator=g, device="cuda", dtype=torch.float32) * 10 - 5
    # a blank that wins about half of the frames, in runs, so that the collapse has work of both kinds
    em[:, :, BLANK] += (torch.rand((B, T // 8 + 1, 1), generator=g, device="cuda") < 0.5).repeat_interleave(
        8, dim=1)[:, :T, 0] * 20.0
    frames = np.random.default_rng(1234).integers(T // 2, T + 1, B).astype(np.int32)
    return em, frames


def byte_model(frames, collapse=True):
    """per utterance: 4 C T_b read; 8 T_b written (label and maximum); 8 T_b read back; 4 (M - T_b) pad; with collapse
    8 M more -- (rows kernel, collapse kernel)"""
    rows = float(sum(4.0 * C * f + 8.0 * f for f in frames))
    col = float(sum(8.0 * f + 4.0 * (T - f) + (8.0 * T if collapse else 0.0) for f in frames))
    return rows, col


def host_collapse(np, lab, frames, out_tok, out_sta, out_len):
    prev = np.empty_like(lab)
    prev[:, 0] = -1
    prev[:, 1:] = lab[:, :-1]
    keep = (lab != prev) & (lab != BLANK) & (np.arange(T)[None, :] < frames[:, None])
    out_tok.fill(-1)
    out_sta.fill(-1)
    for b in range(lab.shape[0]):
        idx = np.nonzero(keep[b])[0]
        out_tok[b, :idx.size] = lab[b, idx]
        out_sta[b, :idx.size] = idx
        out_len[b] = idx.size


def worker(kind, root):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import gtn_amd as gtn
    assert torch.cuda.is_available() and gtn.device_count() > 0, "bench_ctc_decode needs a GPU"
    assert os.path.abspath(os.path.dirname(os.path.dirname(gtn.__file__))) == os.path.abspath(root)
    ragged = kind.endswith("_ragged")
    em, frames = inputs(torch, np)
    if not ragged:
        frames = np.full(B, T, np.int32)
    labels = torch.empty((B, T), dtype=torch.int32, device="cuda")
    tokens = torch.empty((B, T), dtype=torch.int32, device="cuda")
    starts = torch.empty((B, T), dtype=torch.int32, device="cuda")
    scores = torch.empty((B,), dtype=torch.float32, device="cuda")
    lengths = torch.empty((B,), dtype=torch.int32, device="cuda")
    dev3 = torch.empty((3 * B * T + B,), dtype=torch.int32, device="cuda")  # the path route's one upload
    host = torch.full((3 * B * T + B,), -1, dtype=torch.int32).pin_memory()
    h = host.numpy()
    h_lab, h_tok, h_sta = (h[i * B * T:(i + 1) * B * T].reshape(B, T) for i in range(3))
    h_len = h[3 * B * T:]
    lib = gtn._lib

    def path_step():
        ems = gtn.Batch.linear(B, T, C, em, False, True, frames.tolist() if ragged else None)
        paths = gtn.viterbi_path(ems)
        h_lab.fill(-1)
        for b in range(B):  # (straight into the rows of one array: labels_to_list() without the list)
            rc = lib.gtnx_graph_labels_to_array(paths[b]._h, h_lab[b].ctypes.data, 1)
            assert rc == 0
        host_collapse(np, h_lab, frames, h_tok, h_sta, h_len)
        dev3.copy_(host, non_blocking=True)

    def decode_step():
        ems = gtn.Batch.linear(B, T, C, em, False, True)
        ems.linear_decode(labels, scores, frames if ragged else None, BLANK, tokens, starts, lengths)

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
        for _ in range(5):
            decode_step()
            sync()
        print(json.dumps({"trace": "done"}))
        return
    is_decode = kind.startswith("decode")
    stats = getattr(gtn, "debug_linear_decode_stats", None)
    f0, b0 = stats() if stats else (0, 0)
    ms, n = timed(decode_step if is_decode else path_step)
    sync()
    f1, b1 = stats() if stats else (0, 0)
    if is_decode:
        sums = [int(t.to(torch.int64).sum().item()) for t in (labels, tokens, starts, lengths)]
    else:
        sums = [int(dev3[i * B * T:(i + 1) * B * T].to(torch.int64).sum().item()) for i in range(3)]
        sums.append(int(dev3[3 * B * T:].to(torch.int64).sum().item()))
    rows_bytes, col_bytes = byte_model(frames.tolist())
    print(json.dumps({"kind": kind, "utterances": B, "ms_per_batch": ms, "iters": n, "checksums": sums,
                      "rows_bytes": rows_bytes, "collapse_bytes": col_bytes, "launch_utterances": f1 - f0,
                      "path_graph_utterances": b1 - b0}))


def run_worker(kind, root):
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", kind, "--root", root], env=env,
                         stdout=subprocess.PIPE, timeout=500, check=True).stdout.decode()
    rec = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    print(f"[bench_ctc_decode] {kind}: {rec['ms_per_batch']:.3f} ms per batch of {rec['utterances']}", file=sys.stderr,
          flush=True)
    return rec


def spread(v):
    return {"samples": v, "min": min(v), "max": max(v), "median": sorted(v)[len(v) // 2]}


KERNELS = (("linear_decode_rows_kernel", "linear_decode_rows_kernel"),
           ("linear_decode_collapse_kernel", "linear_decode_collapse_kernel"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=["path", "decode", "path_ragged", "decode_ragged", "trace"])
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--parent-root")
    ap.add_argument("--merge-stats")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ctc_decode_c3.json"))
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
        k = means.get("linear_decode_rows_kernel")
        if k and rec.get("rows_bytes"):
            gbs = rec["rows_bytes"] / (k["mean_ms"] * 1e-3) / 1e9
            rec["rows_kernel_on_its_byte_model"] = {
                "achieved_GBs": gbs, "stream_rate_GBs": STREAM_GBS, "frac": gbs / STREAM_GBS,
                "floor_ms": rec["rows_bytes"] / (STREAM_GBS * 1e9) * 1e3, "bytes": "(4 C + 8) T_b per utterance"}
        k = means.get("linear_decode_collapse_kernel")
        if k and rec.get("collapse_bytes"):
            rec["collapse_kernel_on_its_byte_model"] = {
                "achieved_GBs": rec["collapse_bytes"] / (k["mean_ms"] * 1e-3) / 1e9,
                "bytes": "8 T_b + 4 (M - T_b) + 8 M per utterance"}
    else:
        parent = a.parent_root or HERE
        tree = "parent commit" if a.parent_root else "this tree"
        out = {}
        for tag, pk, dk in (("full_length", "path", "decode"), ("frames_uniform_in_half_T_to_T", "path_ragged",
                                                                 "decode_ragged")):
            pa, de, checks = [], [], set()
            for _ in range(3):
                r = run_worker(pk, parent)
                pa.append(r["ms_per_batch"])
                checks.add(tuple(r["checksums"]))
                r = run_worker(dk, HERE)
                de.append(r["ms_per_batch"])
                checks.add(tuple(r["checksums"]))
                assert r["path_graph_utterances"] == 0 and r["launch_utterances"] > 0, r
                if tag == "full_length":
                    rec["rows_bytes"], rec["collapse_bytes"] = r["rows_bytes"], r["collapse_bytes"]
            out[tag] = {
                "path_route": dict(spread(pa), what="viterbi_path(Batch.linear) + labels read from the path graphs + "
                                   "host collapse + one upload (no scores)", tree=tree, utterances=B),
                "decode_route": dict(spread(de), what="Batch.linear_decode (labels, scores, tokens, starts, lengths)",
                                     utterances=B),
                "speedup_median": sorted(pa)[1] / sorted(de)[1],
                "slowest_new_not_slower_than_fastest_parent": max(de) <= min(pa),
                "same_outputs": len(checks) == 1,
            }
        rec.update({"shape": {"B": B, "T": T, "C": C, "blank": BLANK},
                    "unit": "ms per batch, host clock around a closing synchronise, windows >= 0.5 s"})
        rec.update(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
