"""The best (lattice path, alignment) pair of word-piece lattices at the shape of tools/bench_ctc_lattice.py: B = 512
utterances, T = 1000, C = 256, transcripts of 100 units, every piece of up to 4 units, 101 nodes, 394 arcs and 495 states
per lattice, max_states = 512, the same seeded emissions.

  align        torch_loss.ctc_lattice_align with token scores and frame arcs: one call
  paths_only   the same without the two optional outputs
  score        torch_loss.ctc_lattice_score on the same inputs, in the same session: the sum-product sweep the max-plus
               one copies -- the difference is what the back-pointer stores and the walk add
  built        the route without the call, on the first `--built-utterances` utterances (default 16): the alignment graph
               of every lattice built on the host as a transducer (a token arc reads its arc index + 1 and writes its
               label, a blank arc reads 0), compose with Batch.linear, viterbi_path, the input labels read out of the path
               graphs, path arcs and spans derived with numpy, one upload
The tool asserts that the scores of the two routes agree within 1e-4 max(1, |score|) on those utterances, after it has
written its record.

    python tools/bench_ctc_lattice_align.py [--out profiles/ctc_lattice_align_c3.json] [--windows 3]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_ctc_lattice_align.py --worker trace
    python tools/bench_ctc_lattice_align.py --merge-stats DIR/.../kernel_stats.csv [--out ...]

Every figure of the first form is the best of `--windows` windows of at least half a second (at least three calls),
timed with a host clock around a closing synchronise after a warm-up of two calls.  `--worker trace` runs the call ten
times (and ctc_lattice_score ten times) for the profiler; `--merge-stats` adds the kernels' mean times and the align
kernel's rate on the byte model of DESIGN section 38 to the record.  Needs a GPU; without one it fails.
"""
import argparse
import csv
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))
from bench_ctc_lattice import B, BLANK, C, MAX_STATES, T, best_window, lattices  # noqa: E402

KERNELS = ("ctc_lattice_align_kernel", "ctc_lattice_forward_kernel")


def transducer(gtn, np, arcs, K):
    """the CTC alignment graph of a lattice without weights: a token arc reads its arc index + 1 and writes its label"""
    src, dst, lab = (arcs[:, i].astype(np.int64) for i in range(3))
    A = len(arcs)
    g = gtn.Graph(False)
    start = np.arange(K + A) == 0
    accept = np.concatenate([np.arange(K) == K - 1, dst == K - 1])
    g.add_nodes(start.tolist(), accept.tolist())
    tok = K + np.arange(A)
    follow = [(K + p, K + a, a + 1, lab[a]) for a in range(A) for p in np.nonzero((dst == src[a]) & (lab != lab[a]))[0]]
    f = np.array(follow, dtype=np.int64).reshape(-1, 4)
    s = np.concatenate([np.arange(K), tok, src, tok, f[:, 0]])
    d = np.concatenate([np.arange(K), tok, tok, dst, f[:, 1]])
    i = np.concatenate([np.zeros(K, np.int64), 1 + np.arange(A), 1 + np.arange(A), np.zeros(A, np.int64), f[:, 2]])
    o = np.concatenate([np.full(K, BLANK), lab, lab, np.full(A, BLANK), f[:, 3]])
    g.add_arcs(s.astype(np.int32), d.astype(np.int32), i.astype(np.int32), o.astype(np.int32))
    g.arc_sort(True)
    return g


def byte_model(states, A, P, optional):
    """bytes of one call by DESIGN section 38.3 with the lattices' own state count in the place of max_states"""
    per = (4.0 + 2.0) * states * T + 2.0 * T + 12.0 * A + 12.0 + 8.0 + 16.0 * P
    return B * (per + ((4.0 * T + 4.0 * P) + 4.0 * T if optional else 0.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ctc_lattice_align_c3.json"))
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--built-utterances", type=int, default=16)
    ap.add_argument("--worker", choices=["trace"])
    ap.add_argument("--merge-stats")
    args = ap.parse_args()
    if args.merge_stats:
        with open(args.out) as f:
            rec = json.load(f)
        rec["kernels"] = []
        with open(args.merge_stats) as f:
            for row in csv.DictReader(f):
                for kernel in (k for k in KERNELS if k in row["Name"]):
                    ms = float(row["AverageNs"]) * 1e-6
                    rec["kernels"].append({"name": kernel, "launches": int(row["Calls"]),
                                           "mean_ms": ms, "min_ms": float(row["MinNs"]) * 1e-6,
                                           "max_ms": float(row["MaxNs"]) * 1e-6})
                    if KERNELS[0] in row["Name"]:
                        per_call = ms * rec["launches_per_call"]
                        rec["align_kernel_ms_per_call"] = per_call
                        rec["align_kernel_GBps_on_the_byte_model"] = rec["byte_model_bytes"] / (per_call * 1e-3) / 1e9
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
        raise SystemExit("bench_ctc_lattice_align: needs a GPU")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    em = torch.randn((B, T, C), generator=gen, device="cuda", dtype=torch.float32) * 3.0
    em[:, :, BLANK] += (torch.rand((B, T // 8 + 1, 1), generator=gen, device="cuda") < 0.875).repeat_interleave(
        8, dim=1)[:, :T, 0] * 12.0
    em = torch.log_softmax(em, dim=2).contiguous()
    lats = lattices(gtn)
    arcs_h, na_h, nn_h, _ = gtn.pack_lattices(lats)
    arcs, na, nn_ = (torch.from_numpy(a).cuda() for a in (arcs_h, na_h, nn_h))
    A = arcs.shape[1]
    P = int(nn_h.max()) - 1  # (a path has at most nodes - 1 arcs)

    def align():
        return torch_loss.ctc_lattice_align(em, arcs, na, nn_, None, BLANK, None, MAX_STATES, P, True, True)

    def paths_only():
        return torch_loss.ctc_lattice_align(em, arcs, na, nn_, None, BLANK, None, MAX_STATES, P)

    def score():
        return torch_loss.ctc_lattice_score(em, arcs, na, nn_, None, BLANK, None, MAX_STATES)

    if args.worker:
        for _ in range(10):
            align()
            score()
        torch.cuda.synchronize()
        return
    n = max(1, min(args.built_utterances, B))
    graphs = gtn.Batch([transducer(gtn, np, lats[b][0], lats[b][1]) for b in range(n)])
    xb = em[:n].clone().contiguous()

    def built():
        ems = gtn.Batch.linear(n, T, C, xb, calc_grad=False, borrow=True)
        paths = gtn.viterbi_path(gtn.compose(graphs, ems))
        sc = np.full(n, -np.inf, np.float32)
        rows = np.full((4, n, P), -1, np.int32)
        for b in range(n):
            g = paths[b]
            if g.num_arcs() == 0:
                continue
            sc[b] = np.sum(g.weights_to_numpy(), dtype=np.float32)
            fa = np.asarray(g.labels_to_list(True), np.int32) - 1  # the arc of every frame, -1 on blank frames
            t = np.arange(len(fa))
            first = (fa >= 0) & (fa != np.concatenate([[-2], fa[:-1]]))
            last = (fa >= 0) & (fa != np.concatenate([fa[1:], [-2]]))
            k = int(first.sum())
            rows[0, b, :k] = fa[first]
            rows[1, b, :k] = lats[b][0][fa[first], 2]
            rows[2, b, :k] = t[first]
            rows[3, b, :k] = t[last] + 1
        return torch.from_numpy(sc).to(em.device), torch.from_numpy(rows).to(em.device)

    # the two routes give the same scores (ties may part the paths: the tie rule is this project's own)
    out = align()
    bs, brows = built()
    torch.cuda.synchronize()
    s = out[0][:n].double()
    gap = ((s - bs.double()).abs() / s.abs().clamp(min=1.0)).max().item()
    same_paths = int(sum(bool((out[2][b] == brows[0, b]).all() and (out[4][b] == brows[2, b]).all()
                              and (out[5][b] == brows[3, b]).all()) for b in range(n)))
    times = {name: best_window(torch, fn, args.windows) for name, fn in
             (("align", align), ("paths_only", paths_only), ("score", score), ("built", built))}
    states = int((na_h + nn_h).max())
    rec = {
        "shape": {"B": B, "T": T, "C": C, "nodes": int(nn_h.max()), "arcs": int(na_h.max()), "states": states,
                  "max_states": MAX_STATES, "max_path": P},
        "device": torch.cuda.get_device_name(0),
        "built_route_utterances": n,
        "largest_relative_score_gap_between_the_routes": gap,
        "utterances_with_the_same_path_and_spans_in_both_routes": same_paths,
        "mean_path_len": float(out[1].float().mean().item()),
        "seconds": times,
        "lattices_per_second": {"align": B / times["align"], "paths_only": B / times["paths_only"],
                                "score": B / times["score"], "built": n / times["built"]},
        "align_over_score": times["align"] / times["score"],
        "paths_only_over_score": times["paths_only"] / times["score"],
        "microseconds_per_frame_and_utterance_wave": {"align": times["align"] / T * 1e6, "score": times["score"] / T * 1e6},
        "speedup_per_utterance_over_the_built_route": (times["built"] / n) / (times["align"] / B),
        "scratch_bytes_unsliced": 2 * T * MAX_STATES * B,
        "launches_per_call": -(-B // max(1, (256 << 20) // (2 * T * MAX_STATES))),
        "byte_model_bytes": byte_model(states, A, P, True),
        "byte_model_GBps_end_to_end": byte_model(states, A, P, True) / times["align"] / 1e9,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    # (the record is written first, so that a run that misses the gate still leaves its figures behind)
    assert gap <= 1e-4, f"the routes' scores differ by {gap}"


if __name__ == "__main__":
    main()
