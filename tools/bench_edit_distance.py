"""Batched edit distance with the results on the device at BASELINE config C3's shape: B = 512 utterances, hypotheses
from `Batch.ctc_beam_decode` on the bench tensor (T = 1000, C = 256, beam_size 16, cutoff_top_n 16) with nbest 1 and 16,
references of 100 tokens.

  ops    gtn_amd.edit_distance with dist and ops (the walk keeps 16 bytes per (column, block) in scratch)
  plain  gtn_amd.edit_distance with dist only: one launch
  host   the route a user has without the call: download of tokens and lengths, a numpy Levenshtein (one vectorised row
         of the table at a time) over the B * nbest pairs, one upload of the distances

    python tools/bench_edit_distance.py [--out profiles/edit_distance_c3.json]
        per nbest three samples of `ops` and `plain`, every sample a process of its own that warms its shapes up and
        then times windows of at least half a second with a host clock around a closing synchronise, and one sample of
        `host` (a single pass: it takes seconds)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_edit_distance.py --worker trace --nbest N
        a few calls of both forms, for the mean times of the kernels (a run of its own: no counters, no other tracing)
    python tools/bench_edit_distance.py --merge-stats DIR/.../kernel_stats.csv --nbest N [--out ...]
        adds those means to the record: per launch, per (token, block) step of the recurrence, and the rate on the byte
        model -- which is not the kernel's bound: the recurrence is a dependent chain of wave-uniform integer operations.

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
BLANK, BEAM, TOPN = 0, 16, 16
WINDOW_S = 0.5


def inputs(torch, gtn, nbest):
    """(tokens [B, nbest, T], lengths [B, nbest]) of the beam search on the bench tensor of tools/bench_ctc_beam.py,
    references [B, U] of U seeded labels, their lengths"""
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    em = torch.randn((B, T, C), generator=g, device="cuda", dtype=torch.float32) * 3.0
    em[:, :, BLANK] += (torch.rand((B, T // 8 + 1, 1), generator=g, device="cuda") < 0.5).repeat_interleave(
        8, dim=1)[:, :T, 0] * 12.0
    em = torch.log_softmax(em, dim=2).contiguous()
    tokens = torch.empty((B, nbest, T), dtype=torch.int32, device="cuda")
    lengths = torch.empty((B, nbest), dtype=torch.int32, device="cuda")
    scores = torch.empty((B, nbest), dtype=torch.float32, device="cuda")
    gtn.Batch.linear(B, T, C, em, False, True).ctc_beam_decode(tokens, lengths, scores, None, BLANK, BEAM, TOPN, nbest)
    ref = torch.randint(1, C, (B, U), generator=g, device="cuda", dtype=torch.int32)
    ref_len = torch.full((B,), U, dtype=torch.int32, device="cuda")
    gtn.synchronize()
    return tokens, lengths, ref, ref_len


def host_levenshtein(np, ref, hyp):
    m, n = len(ref), len(hyp)
    cols = np.arange(n + 1)
    row = cols.copy()
    for i in range(1, m + 1):
        t = np.empty(n + 1, np.int64)
        t[0] = i
        t[1:] = np.minimum(row[:-1] + (hyp != ref[i - 1]), row[1:] + 1)
        row = np.minimum.accumulate(t - cols) + cols
    return int(row[n])


def worker(kind, nbest):
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    import gtn_amd as gtn
    assert torch.cuda.is_available() and gtn.device_count() > 0, "bench_edit_distance needs a GPU"
    tokens, lengths, ref, ref_len = inputs(torch, gtn, nbest)
    dist = torch.empty((B, nbest), dtype=torch.int32, device="cuda")
    ops = torch.empty((B, nbest, 3), dtype=torch.int32, device="cuda")

    def ops_step():
        gtn.edit_distance(tokens, lengths, ref, ref_len, dist, ops)

    def plain_step():
        gtn.edit_distance(tokens, lengths, ref, ref_len, dist)

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
            ops_step()
            plain_step()
            sync()
        print(json.dumps({"trace": "done"}))
        return
    ln = lengths.cpu().numpy()
    rec = {"kind": kind, "nbest": nbest, "pairs": B * nbest, "mean_hyp_length": float(ln.mean()),
           "max_hyp_length": int(ln.max()), "token_block_steps": int(ln.sum()) * ((U + 63) // 64)}
    if kind == "host":
        sync()
        t0 = time.perf_counter()
        tk, ln, rf, rl = tokens.cpu().numpy(), lengths.cpu().numpy(), ref.cpu().numpy(), ref_len.cpu().numpy()
        out = np.empty((B, nbest), np.int32)
        for b in range(B):
            for k in range(nbest):
                out[b, k] = host_levenshtein(np, rf[b, :rl[b]], tk[b, k, :ln[b, k]])
        up = torch.from_numpy(out).to("cuda")
        sync()
        rec.update(ms_per_batch=(time.perf_counter() - t0) * 1e3, iters=1)
        plain_step()
        sync()
        rec["agrees_with_the_device"] = bool((up == dist).all().item())
    else:
        c0 = gtn.debug_edit_distance_stats()
        ms, n = timed(ops_step if kind == "ops" else plain_step)
        c1 = gtn.debug_edit_distance_stats()
        rec.update(ms_per_batch=ms, iters=n, pairs_counted=c1[1] - c0[1], mean_dist=float(dist.float().mean().item()))
    print(json.dumps(rec))


def run_worker(kind, nbest):
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", kind, "--nbest", str(nbest)], env=env,
                         stdout=subprocess.PIPE, timeout=500, check=True).stdout.decode()
    rec = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    print(f"[bench_edit_distance] {kind} nbest {nbest}: {rec['ms_per_batch']:.3f} ms per {rec['pairs']} pairs",
          file=sys.stderr, flush=True)
    return rec


def spread(v):
    return {"samples": v, "min": min(v), "max": max(v), "median": sorted(v)[len(v) // 2]}


def byte_model(nbest, with_ops):
    """by the widths, as the engine's profile scope counts them: every token and length once, the distance out; with
    ops the (Pv, Mv) words of every (column, block) out and back in and the three counts"""
    pairs = float(B) * nbest
    io = pairs * (4.0 * T + 8.0) + B * (4.0 * U + 4.0)
    return io + (pairs * (2.0 * 16.0 * T * ((U + 63) // 64) + 12.0) if with_ops else 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=["ops", "plain", "host", "trace"])
    ap.add_argument("--nbest", type=int, default=1)
    ap.add_argument("--merge-stats")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "edit_distance_c3.json"))
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.nbest)
        return
    rec = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            rec = json.load(f)
    if a.merge_stats:
        key = f"nbest {a.nbest}"
        steps = rec.get(key, {}).get("token_block_steps")
        means = {}
        with open(a.merge_stats) as f:
            for row in csv.DictReader(f):
                if "edit_distance_kernel" in row["Name"]:
                    form = "ops" if "Lb1" in row["Name"] or "<true>" in row["Name"] else "plain"
                    ms = float(row["AverageNs"]) * 1e-6
                    means[form] = {"calls": int(row["Calls"]), "mean_ms": ms, "min_ms": float(row["MinNs"]) * 1e-6,
                                   "max_ms": float(row["MaxNs"]) * 1e-6,
                                   "achieved_GBs_on_the_byte_model": byte_model(a.nbest, form == "ops") / (ms * 1e-3) / 1e9}
                    if steps:
                        # 256 CUs x 4 SIMDs run the pairs side by side: the per-step cost of ONE wave's chain is the
                        # launch time over the steps of the longest-running SIMD's share, which this does not resolve;
                        # the figure below is launch time over all steps (throughput), in nanoseconds
                        means[form]["ns_per_token_block_step_of_the_batch"] = ms * 1e6 / steps
        rec.setdefault(key, {})["kernels"] = means
    else:
        rec["shape"] = {"B": B, "T": T, "C": C, "U": U, "beam_size": BEAM, "cutoff_top_n": TOPN}
        rec["unit"] = "ms per call, host clock around a closing synchronise, windows >= 0.5 s (host: one pass)"
        for nbest in (1, 16):
            op, pl, last = [], [], None
            for _ in range(3):
                last = run_worker("ops", nbest)
                assert last["pairs_counted"] > 0, last
                op.append(last["ms_per_batch"])
                pl.append(run_worker("plain", nbest)["ms_per_batch"])
            host = run_worker("host", nbest)
            assert host["agrees_with_the_device"], host
            rec.setdefault(f"nbest {nbest}", {}).update({
                "pairs": B * nbest, "mean_hyp_length": last["mean_hyp_length"], "max_hyp_length": last["max_hyp_length"],
                "token_block_steps": last["token_block_steps"], "mean_dist": last["mean_dist"],
                "ops": dict(spread(op), what="gtn_amd.edit_distance with dist and ops"),
                "plain": dict(spread(pl), what="gtn_amd.edit_distance with dist only"),
                "host": {"ms": host["ms_per_batch"], "what": "download, numpy Levenshtein per pair, one upload",
                         "agrees_with_the_device": True},
                "bytes_plain": byte_model(nbest, False), "bytes_ops": byte_model(nbest, True)})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
