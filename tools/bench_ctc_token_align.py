"""Time-stamped N-best hypotheses at BASELINE config C3's shape: B = 512 utterances, T = 1000, C = 256, hypotheses from
`ctc_beam_decode` (beam_size 16, cutoff_top_n 16, nbest 4) on the seeded log-softmax tensor of tools/bench_ctc_score.py
(243 labels on average, 321 at most), `max_length` 256.

  token_align  torch_loss.ctc_token_align with token scores and frame tokens: one call, sliced by its scratch cap
  spans_only   the same without the two optional outputs
  host_route   the only route the parent commit offers for the same numbers: tokens and lengths .tolist() (a download
               and a wait), nbest calls of ctc_forced_align on the same tensor, one hypothesis per utterance each, the
               token planes downloaded, starts and ends derived from them with numpy, one upload.  ctc_forced_align's
               kernel takes targets of up to 255 labels; a longer one sends the whole batch down the path-graph route, so
               this route aligns the empty sequence in the place of every hypothesis above 255 labels (the record counts
               them): that favours it.

    python tools/bench_ctc_token_align.py [--out profiles/ctc_token_align_c3.json] [--windows 3]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_ctc_token_align.py --worker trace
    python tools/bench_ctc_token_align.py --merge-stats DIR/.../kernel_stats.csv [--out ...]

Every figure of the first form is the best of `--windows` windows of at least half a second (at least three calls),
timed with a host clock around a closing synchronise after a warm-up of two calls.  `--worker trace` runs the call ten
times for the profiler; `--merge-stats` adds the kernel's mean time per launch (a call at this shape is two launches) and
its rate on the byte model of DESIGN section 24 to the record.  Needs a GPU; without one it fails.
"""
import argparse
import csv
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))
from bench_ctc_score import B, BEAM, BLANK, C, MAX_LENGTH, NBEST, T, TOPN, best_window, inputs  # noqa: E402

ALIGNER_MAX = 255  # the longest target ctc_forced_align's kernel takes
KERNEL = "ctc_token_align_kernel"


def byte_model(mean_len):
    """bytes of one call by DESIGN section 24.3, with the mean hypothesis length in the place of the width"""
    SM = 2 * MAX_LENGTH + 1
    pairs = B * NBEST
    return pairs * ((4.0 + 0.25) * SM * T + 32.0 * T + 4.0 * mean_len + 8.0 + 8.0 * T + 4.0 * T + 4.0 * T + 4.0 * T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ctc_token_align_c3.json"))
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--worker", choices=["trace"])
    ap.add_argument("--merge-stats")
    args = ap.parse_args()
    if args.merge_stats:
        with open(args.out) as f:
            rec = json.load(f)
        with open(args.merge_stats) as f:
            for row in csv.DictReader(f):
                if KERNEL in row["Name"]:
                    launches = rec["launches_per_call"]
                    ms = float(row["AverageNs"]) * 1e-6
                    rec["kernel"] = {"name": KERNEL, "launches": int(row["Calls"]), "mean_ms_per_launch": ms,
                                     "min_ms": float(row["MinNs"]) * 1e-6, "max_ms": float(row["MaxNs"]) * 1e-6,
                                     "ms_per_call": ms * launches,
                                     "GBps_on_the_byte_model": rec["byte_model_bytes"] / (ms * launches * 1e-3) / 1e9}
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        print(json.dumps(rec))
        return
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    import gtn_amd as gtn
    from gtn_amd import torch_loss
    if not (torch.cuda.is_available() and gtn.device_count() > 0):
        raise SystemExit("bench_ctc_token_align: needs a GPU")
    em, tokens, lengths, beam, _ = inputs(torch, torch_loss)
    L = tokens.shape[2]

    def token_align():
        return torch_loss.ctc_token_align(em, tokens, lengths, BLANK, None, MAX_LENGTH, True, True)

    if args.worker:
        for _ in range(10):
            token_align()
        torch.cuda.synchronize()
        return

    def spans_only():
        return torch_loss.ctc_token_align(em, tokens, lengths, BLANK, None, MAX_LENGTH)

    def host_route():
        tk, lh = tokens.tolist(), lengths.tolist()  # (the download and the wait)
        starts = np.full((B, NBEST, L), -1, np.int32)
        ends = np.full((B, NBEST, L), -1, np.int32)
        scores = []
        rows = np.arange(B)[:, None]
        for k in range(NBEST):
            targets = [tk[b][k][:lh[b][k]] if lh[b][k] <= ALIGNER_MAX else [] for b in range(B)]
            _, plane, sc = torch_loss.ctc_forced_align(em, targets, BLANK)
            scores.append(sc)
            p = plane.cpu().numpy()
            prev = np.concatenate([np.full((B, 1), -2, np.int32), p[:, :-1]], axis=1)
            nxt = np.concatenate([p[:, 1:], np.full((B, 1), -2, np.int32)], axis=1)
            t = np.broadcast_to(np.arange(T, dtype=np.int32), p.shape)
            first, last = (p >= 0) & (p != prev), (p >= 0) & (p != nxt)
            starts[:, k][np.broadcast_to(rows, p.shape)[first], p[first]] = t[first]
            ends[:, k][np.broadcast_to(rows, p.shape)[last], p[last]] = t[last] + 1
        return torch.stack(scores, dim=1), torch.from_numpy(starts).to(em.device), torch.from_numpy(ends).to(em.device)

    # the two routes give the same spans and the same score bits wherever both align the hypothesis
    s, st, en, _, _ = token_align()
    hs, hst, hen = host_route()
    ln = lengths.clamp(0, L)
    both = ln <= ALIGNER_MAX
    agree = bool((st[both] == hst[both]).all() and (en[both] == hen[both]).all() and (s[both] == hs[both]).all())
    times = {name: best_window(torch, fn, args.windows) for name, fn in
             (("token_align", token_align), ("spans_only", spans_only), ("host_route", host_route))}
    pairs = B * NBEST
    SM = 2 * MAX_LENGTH + 1
    per_pair = 4 * ((T + 15) // 16) * SM
    slice_pairs = max(1, (256 << 20) // per_pair)
    mean_len = float(ln.float().mean().item())
    rec = {
        "shape": {"B": B, "T": T, "C": C, "beam_size": BEAM, "cutoff_top_n": TOPN, "nbest": NBEST,
                  "max_length": MAX_LENGTH},
        "device": torch.cuda.get_device_name(0),
        "hypothesis_lengths": {"mean": mean_len, "max": int(ln.max().item()),
                               "above_max_length": int((ln > MAX_LENGTH).sum().item()),
                               "above_255_aligned_as_empty_by_the_host_route": int((ln > ALIGNER_MAX).sum().item())},
        "routes_agree_where_both_align": agree,
        "seconds": times,
        "speedup": times["host_route"] / times["token_align"],
        "scratch_bytes_per_pair": per_pair,
        "scratch_bytes_unsliced": per_pair * pairs,
        "launches_per_call": -(-pairs // slice_pairs),
        "byte_model_bytes": byte_model(mean_len),
        "byte_model_GBps_end_to_end": byte_model(mean_len) / times["token_align"] / 1e9,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
