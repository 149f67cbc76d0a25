"""Time-stamped ASG N-best hypotheses at BASELINE config C4's shape: B = 512 utterances, T = 1000, C = 512, the nbest-4
hypotheses of `asg_beam_decode` (beam_size 16, cutoff_top_n 16) on the seeded tensor and table of tools/bench_asg_beam.py,
`max_length` the largest that holds them (up to 4096).

  token_align  torch_loss.asg_token_align with token scores and frame tokens: one call, sliced by its scratch cap
  spans_only   the same without the two optional outputs
  host_route   the only route the parent commit offers for the same numbers: tokens and lengths .tolist() (a download
               and a wait), nbest calls of asg_forced_align on the same tensor, one hypothesis per utterance each, the
               token planes downloaded, starts and ends derived from them with numpy, one upload.  asg_forced_align's
               kernel takes targets of up to 511 labels; a longer one sends the whole batch down the path-graph route, so
               this route aligns the FIRST 511 LABELS in the place of every longer hypothesis (the record counts them):
               the work of a hypothesis that just fits, not the work asked for.  It uses nothing this tool's commit
               adds, so it runs on the parent commit's build as well (--host-tree: a checkout of it, built).

    python tools/bench_asg_token_align.py [--out profiles/asg_token_align_c4.json] [--host-tree DIR]
        three samples of each route, alternating, every sample a process of its own that warms up and then times windows
        of at least half a second with a host clock around a closing synchronise; --host-tree: the checkout whose build
        runs the host route (default: this one)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_asg_token_align.py --worker trace
    python tools/bench_asg_token_align.py --merge-stats DIR/.../kernel_stats.csv [--out ...]
        adds the kernel's mean time per launch and its rate on the byte model of DESIGN section 28 to the record.

Needs a GPU; without one it fails.
"""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, C = 512, 1000, 512
BEAM, TOPN, NBEST = 16, 16, 4
ALIGNER_MAX = 511  # the longest target asg_forced_align's kernel takes
KERNEL = "asg_token_align_kernel"
WINDOW_S = 0.5


def inputs(torch):
    """the tensor and the table of tools/bench_asg_beam.py (kept here as well: the host route also runs from a tree that
    has no such file)"""
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    em = torch.randn((B, T, C), generator=g, device="cuda", dtype=torch.float32) * 3.0
    lifted = torch.randint(0, C, (B, T // 8 + 1), generator=g, device="cuda").repeat_interleave(8, dim=1)[:, :T]
    em.scatter_add_(2, lifted.unsqueeze(2), torch.full((B, T, 1), 12.0, device="cuda"))
    g = torch.Generator(device="cuda")
    g.manual_seed(4321)
    table = torch.randn((C + C * C,), generator=g, device="cuda", dtype=torch.float32).contiguous()
    return torch.log_softmax(em, dim=2).contiguous(), table


def byte_model(max_length, mean_len, optional):
    """bytes of one call by DESIGN section 28.3 with T_b = T: the sweep over the mean length, the walk's windows, the
    rows and the tokens"""
    pairs = B * NBEST
    sweep = (4.0 + 0.125) * mean_len * T
    walk = 8.0 * T
    rows = 12.0 * mean_len + 8.0 + 8.0 * T
    extra = (4.0 * T + 4.0 * T) + 4.0 * T if optional else 0.0
    return pairs * (sweep + walk + rows + extra)


def worker(kind, tree):
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    import gtn_amd as gtn
    from gtn_amd import torch_loss
    if not (torch.cuda.is_available() and gtn.device_count() > 0):
        raise SystemExit("bench_asg_token_align: needs a GPU")
    em, table = inputs(torch)
    start, trans = table[:C].contiguous(), table[C:].reshape(C, C).contiguous()
    tokens, lengths, _ = torch_loss.asg_beam_decode(em, trans, start=start, beam_size=BEAM, cutoff_top_n=TOPN, nbest=NBEST)
    torch.cuda.synchronize()
    L = tokens.shape[2]
    ln = lengths.clamp(0, L)
    max_length = max(1, min(int(ln.max().item()), 4096))

    def token_align():
        return torch_loss.asg_token_align(em, trans, tokens, lengths, start, None, max_length, True, True)

    def spans_only():
        return torch_loss.asg_token_align(em, trans, tokens, lengths, start, None, max_length)

    def host_route():
        tk, lh = tokens.tolist(), lengths.tolist()  # (the download and the wait)
        starts = np.full((B, NBEST, L), -1, np.int32)
        ends = np.full((B, NBEST, L), -1, np.int32)
        scores = []
        rows = np.arange(B)[:, None]
        for k in range(NBEST):
            targets = [tk[b][k][:min(lh[b][k], ALIGNER_MAX)] for b in range(B)]
            _, plane, sc = torch_loss.asg_forced_align(em, trans, targets, start=start)
            scores.append(sc)
            p = plane.cpu().numpy()
            prev = np.concatenate([np.full((B, 1), -2, np.int32), p[:, :-1]], axis=1)
            t = np.broadcast_to(np.arange(T, dtype=np.int32), p.shape)
            first = (p >= 0) & (p != prev)
            starts[:, k][np.broadcast_to(rows, p.shape)[first], p[first]] = t[first]
            nxt = np.concatenate([p[:, 1:], np.full((B, 1), -2, np.int32)], axis=1)
            last = (p >= 0) & (p != nxt)
            ends[:, k][np.broadcast_to(rows, p.shape)[last], p[last]] = t[last] + 1
        return torch.stack(scores, dim=1), torch.from_numpy(starts).to(em.device), torch.from_numpy(ends).to(em.device)

    if kind == "trace":
        for _ in range(10):
            token_align()
        torch.cuda.synchronize()
        print(json.dumps({"trace": "done"}))
        return
    step = {"token_align": token_align, "spans_only": spans_only, "host_route": host_route}[kind]
    for _ in range(2):
        out = step()
    torch.cuda.synchronize()
    best = None
    for _ in range(2):
        n, t0 = 0, time.perf_counter()
        while True:
            out = step()
            torch.cuda.synchronize()
            n += 1
            dt = time.perf_counter() - t0
            if dt >= WINDOW_S and n >= 3:
                break
        best = dt / n if best is None else min(best, dt / n)
    rec = {"kind": kind, "seconds": best, "max_length": max_length,
           "lengths": {"mean": float(ln.float().mean().item()), "max": int(ln.max().item()),
                       "above_511": int((ln > ALIGNER_MAX).sum().item()), "pairs": B * NBEST,
                       "empty_slots": int((ln == 0).sum().item())}}
    if kind == "token_align":
        # the host route's numbers on the same build, once: the same spans and score bits wherever both align the whole
        hs, hst, hen = host_route()
        both = (ln <= ALIGNER_MAX) & (ln > 0)
        s, st, en = out[:3]
        rec["routes_agree_where_both_align"] = bool((st[both] == hst[both]).all() and (en[both] == hen[both]).all()
                                                    and (s[both] == hs[both]).all())
        rec["pairs_with_a_path"] = int(torch.isfinite(s).sum().item())
    print(json.dumps(rec))


def run_worker(kind, tree):
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", kind, "--host-tree", tree], env=env,
                         stdout=subprocess.PIPE, timeout=900, check=True).stdout.decode()
    rec = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    print(f"[bench_asg_token_align] {kind}: {rec['seconds'] * 1e3:.3f} ms per call", file=sys.stderr, flush=True)
    return rec


def spread(v):
    return {"samples": v, "min": min(v), "max": max(v), "median": sorted(v)[len(v) // 2]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "asg_token_align_c4.json"))
    ap.add_argument("--worker", choices=["token_align", "spans_only", "host_route", "trace"])
    ap.add_argument("--host-tree", default=HERE)
    ap.add_argument("--merge-stats")
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, os.path.abspath(a.host_tree) if a.worker == "host_route" else HERE)
        return
    if a.merge_stats:
        with open(a.out) as f:
            rec = json.load(f)
        with open(a.merge_stats) as f:
            for row in csv.DictReader(f):
                if KERNEL in row["Name"]:
                    launches = rec["launches_per_call"]
                    ms = float(row["AverageNs"]) * 1e-6
                    rec["kernel"] = {"name": KERNEL, "launches": int(row["Calls"]), "mean_ms_per_launch": ms,
                                     "min_ms": float(row["MinNs"]) * 1e-6, "max_ms": float(row["MaxNs"]) * 1e-6,
                                     "ms_per_call": ms * launches,
                                     "GBps_on_the_byte_model": rec["byte_model_bytes"] / (ms * launches * 1e-3) / 1e9}
    else:
        samples = {"token_align": [], "spans_only": [], "host_route": []}
        last = {}
        for _ in range(3):
            for kind in samples:
                last[kind] = run_worker(kind, a.host_tree)
                samples[kind].append(last[kind]["seconds"])
        la = last["token_align"]
        max_length, mean_len = la["max_length"], la["lengths"]["mean"]
        pairs = B * NBEST
        per_pair = 4 * ((T + 31) // 32) * max_length
        slice_pairs = max(1, (256 << 20) // per_pair)
        med = {k: sorted(v)[1] for k, v in samples.items()}
        rec = {"shape": {"B": B, "T": T, "C": C, "beam_size": BEAM, "cutoff_top_n": TOPN, "nbest": NBEST,
                         "max_length": max_length},
               "unit": "seconds per call, host clock around a closing synchronise, windows >= 0.5 s, a process per sample",
               "hypothesis_lengths": dict(la["lengths"], above_511_given_their_first_511_labels_on_the_host_route=la[
                   "lengths"]["above_511"]),
               "pairs_with_a_path": la["pairs_with_a_path"],
               "routes_agree_where_both_align": la["routes_agree_where_both_align"],
               "host_route_build": "this checkout" if os.path.abspath(a.host_tree) == HERE else "another checkout (--host-tree)",
               "seconds": {k: spread(v) for k, v in samples.items()},
               "speedup_of_the_medians": med["host_route"] / med["token_align"],
               "scratch_bytes_per_pair": per_pair, "scratch_bytes_unsliced": per_pair * pairs,
               "launches_per_call": -(-pairs // slice_pairs),
               "byte_model_bytes": byte_model(max_length, mean_len, True),
               "byte_model_GBps_end_to_end": byte_model(max_length, mean_len, True) / med["token_align"] / 1e9}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
