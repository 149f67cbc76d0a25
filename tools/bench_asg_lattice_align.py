"""The best (lattice path, alignment) pair of word-piece lattices under the ASG criterion at the shape of
tools/bench_asg_lattice.py: B = 512 utterances, T = 1000, C = 512, transcripts of 100 units, every piece of up to 4
units, 101 nodes, 394 arcs (495 states for max_states = 512) and up to 1 536 edges per lattice, the same seeded
emissions, transitions and start scores.

  align        torch_loss.asg_lattice_align with token scores and frame arcs: one call
  paths_only   the same without the two optional outputs
  score        torch_loss.asg_lattice_score on the same inputs, in the same session: the sum-product sweep the max-plus
               one copies -- the difference is what the back-pointer stores and the walk add
  built        the route without the call, on the first `--built-utterances` utterances (default 16): the expanded graph
               of every lattice built on the host as a transducer (every arc into the node of lattice arc a reads a and
               writes its label), compose with Batch.linear, viterbi_path, the input labels read out of the path graphs,
               path arcs and spans derived with numpy, one upload
The tool asserts that the scores of the two routes agree within 1e-4 max(1, |score|) on those utterances, after it has
written its record.

    python tools/bench_asg_lattice_align.py [--out profiles/asg_lattice_align_c4.json] [--windows 3]
    python tools/bench_asg_lattice_align.py --new-only       (the new call alone: what a kernel trace is taken of)

Every figure is the best of `--windows` windows of at least half a second (at least three calls), timed with a host
clock around a closing synchronise after a warm-up of two calls.  No timing is promised.  Needs a GPU; without one it
fails.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))
from bench_asg_lattice import B, C, MAX_STATES, T, best_window, lattices  # noqa: E402


def transducer(gtn, np, arcs, K, trans, start):
    """bench_asg_lattice.expanded_graph as a transducer: node 0 starts, node 1 + a is arc a, and every arc into it reads
    a and writes the label of a"""
    src, dst, lab = (arcs[:, i].astype(np.int64) for i in range(3))
    A = len(arcs)
    g = gtn.Graph(False)
    g.add_nodes((np.arange(A + 1) == 0).tolist(), np.concatenate([[False], dst == K - 1]).tolist())
    first = np.nonzero(src == 0)[0]
    step = np.array([(p, a) for a in range(A) for p in np.nonzero(dst == src[a])[0]], dtype=np.int64).reshape(-1, 2)
    to = np.concatenate([np.arange(A), first, step[:, 1]])
    s = np.concatenate([1 + np.arange(A), np.zeros(first.size, np.int64), 1 + step[:, 0]])
    w = np.concatenate([trans[lab, lab], start[lab[first]], trans[lab[step[:, 1]], lab[step[:, 0]]]])
    g.add_arcs(s.astype(np.int32), (1 + to).astype(np.int32), to.astype(np.int32), lab[to].astype(np.int32),
               w.astype(np.float32))
    g.arc_sort(True)
    return g


def byte_model(arcs, edges, P, optional):
    """bytes of one call by DESIGN section 39.3 with the lattices' own arc and edge counts in the place of the bounds"""
    per = (6.0 * arcs + 4.0 * edges) * T + 2.0 * T + 12.0 * arcs + 12.0 + 8.0 + 16.0 * P
    return B * (per + ((4.0 * T + 4.0 * P) + 4.0 * T if optional else 0.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "asg_lattice_align_c4.json"))
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--built-utterances", type=int, default=16)
    ap.add_argument("--new-only", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    import gtn_amd as gtn
    from gtn_amd import torch_loss
    if not (torch.cuda.is_available() and gtn.device_count() > 0):
        raise SystemExit("bench_asg_lattice_align: needs a GPU")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    em = torch.randn((B, T, C), generator=gen, device="cuda", dtype=torch.float32)
    trans = (torch.randn((C, C), generator=gen, device="cuda") * 0.5).contiguous()
    start = (torch.randn((C,), generator=gen, device="cuda") * 0.5).contiguous()
    lats = lattices(gtn)
    arcs_h, na_h, nn_h, _ = gtn.pack_lattices(lats)
    arcs, na, nn_ = (torch.from_numpy(a).cuda() for a in (arcs_h, na_h, nn_h))
    P = int(nn_h.max()) - 1  # (a path has at most nodes - 1 arcs)

    def align():
        return torch_loss.asg_lattice_align(em, trans, arcs, na, nn_, None, start, None, MAX_STATES, None, P, True, True)

    def paths_only():
        return torch_loss.asg_lattice_align(em, trans, arcs, na, nn_, None, start, None, MAX_STATES, None, P)

    def score():
        return torch_loss.asg_lattice_score(em, trans, arcs, na, nn_, None, start, None, MAX_STATES)

    if args.new_only:
        for _ in range(10):
            align()
        torch.cuda.synchronize()
        return
    n = max(1, min(args.built_utterances, B))
    trans_h, start_h = trans.cpu().numpy(), start.cpu().numpy()
    graphs = gtn.Batch([transducer(gtn, np, lats[b][0], lats[b][1], trans_h, start_h) for b in range(n)])
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
            fa = np.asarray(g.labels_to_list(True), np.int32)  # the arc of every frame
            t = np.arange(len(fa))
            first = fa != np.concatenate([[-2], fa[:-1]])
            k = int(first.sum())
            rows[0, b, :k] = fa[first]
            rows[1, b, :k] = lats[b][0][fa[first], 2]
            rows[2, b, :k] = t[first]
            rows[3, b, :k] = np.concatenate([t[first][1:], [len(fa)]])
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
    edges = int(max(np.bincount(l[0][:, 1], minlength=l[1])[l[0][:, 0]].sum() for l in lats))
    rec = {
        "shape": {"B": B, "T": T, "C": C, "nodes": int(nn_h.max()), "arcs": int(na_h.max()), "edges": edges,
                  "max_states": MAX_STATES, "max_edges": min(8 * MAX_STATES, 1 << 21), "max_path": P},
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
        "speedup_per_utterance_over_the_built_route": (times["built"] / n) / (times["align"] / B),
        "scratch_bytes_unsliced": 2 * T * MAX_STATES * B,
        "launches_per_call": -(-B // max(1, (256 << 20) // (2 * T * MAX_STATES))),
        "byte_model_bytes": byte_model(int(na_h.max()), edges, P, True),
        "byte_model_GBps_end_to_end": byte_model(int(na_h.max()), edges, P, True) / times["align"] / 1e9,
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
