"""ASG scores of word-piece lattices, and their gradients, at BASELINE config C4's shape: B = 512 utterances, T = 1000,
C = 512, transcripts of 100 units over a 26-letter alphabet, every piece of up to 4 units in the inventory (labels 0 ..
511 by a fixed hash of the piece), so each lattice has 101 nodes and 394 arcs (495 states for max_states = 512) and
up to 1 536 edges (max_edges at its default, 4096).  Emissions, transitions and start scores are seeded normal
tensors: ASG takes any scores.

  score           torch_loss.asg_lattice_score without requires_grad: one launch
  score+grads     the same with emissions, transitions, start and learned arc weights requiring gradients, and
                  .backward(g): the forward launch and the one gradient call (alpha, backward and table launches per
                  slice of utterances)
  built           the route the parent commit offers for the same numbers: the expanded graph of every lattice built as a
                  Graph (a start node plus one node per arc; start, step and self-loop arcs carrying the table's entries),
                  composed with Batch.linear through the built-lattice path, forward_score on the result
  built+grad      ... and backward() with the emission gradients written out
The built route composes every product, so it runs on the first `--built-utterances` utterances only (default 16) and
the record gives both routes per utterance as well.  The tool asserts that the two routes agree within the gate of the
tests on those utterances: scores within 1e-4 max(1, |score|), emission gradients within 1e-4.

    python tools/bench_asg_lattice.py [--out profiles/asg_lattice_c4.json] [--windows 3] [--built-utterances 16]
    python tools/bench_asg_lattice.py --new-only          (the new route alone: what a kernel trace is taken of)

Every figure is the best of `--windows` windows of at least half a second (at least three calls), timed with a host
clock around a closing synchronise after a warm-up of two calls.  No timing is promised.  Needs a GPU; without one it
fails.
"""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, C = 512, 1000, 512
UNITS, LONGEST, MAX_STATES = 100, 4, 512
WINDOW_S = 0.5


def lattices(gtn):
    rng = np.random.default_rng(1234)
    out = []
    for _ in range(B):
        units = "".join(chr(97 + int(c)) for c in rng.integers(0, 26, UNITS))
        pieces = {units[i:j]: zlib.crc32(units[i:j].encode()) % C
                  for i in range(UNITS) for j in range(i + 1, min(UNITS, i + LONGEST) + 1)}
        out.append(gtn.decomposition_lattice(units, pieces))
    return out


def expanded_graph(gtn, arcs, K, trans, start):
    """the ASG alignment graph of a lattice without arc weights as a Graph: node 0 starts, node 1 + a is arc a"""
    src, dst, lab = (arcs[:, i].astype(np.int64) for i in range(3))
    A = len(arcs)
    g = gtn.Graph(False)
    g.add_nodes((np.arange(A + 1) == 0).tolist(), np.concatenate([[False], dst == K - 1]).tolist())
    first = np.nonzero(src == 0)[0]
    step = np.array([(p, a) for a in range(A) for p in np.nonzero(dst == src[a])[0]], dtype=np.int64).reshape(-1, 2)
    tok = 1 + np.arange(A)
    s = np.concatenate([tok, np.zeros(first.size, np.int64), 1 + step[:, 0]])
    d = np.concatenate([tok, 1 + first, 1 + step[:, 1]])
    l = np.concatenate([lab, lab[first], lab[step[:, 1]]])
    w = np.concatenate([trans[lab, lab], start[lab[first]], trans[lab[step[:, 1]], lab[step[:, 0]]]])
    g.add_arcs(s.astype(np.int32), d.astype(np.int32), l.astype(np.int32), l.astype(np.int32), w.astype(np.float32))
    g.arc_sort()
    return g


def best_window(torch, fn, windows):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    best = None
    for _ in range(windows):
        n, t0 = 0, time.perf_counter()
        while True:
            fn()
            n += 1
            if n >= 3 and time.perf_counter() - t0 >= WINDOW_S:
                break
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / n
        best = dt if best is None else min(best, dt)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "asg_lattice_c4.json"))
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--built-utterances", type=int, default=16)
    ap.add_argument("--new-only", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    import gtn_amd as gtn
    from gtn_amd import torch_loss
    if not (torch.cuda.is_available() and gtn.device_count() > 0):
        raise SystemExit("bench_asg_lattice: needs a GPU")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    em = torch.randn((B, T, C), generator=gen, device="cuda", dtype=torch.float32)
    trans = (torch.randn((C, C), generator=gen, device="cuda") * 0.5).contiguous()
    start = (torch.randn((C,), generator=gen, device="cuda") * 0.5).contiguous()
    lats = lattices(gtn)
    arcs_h, na_h, nn_h, _ = gtn.pack_lattices(lats)
    arcs, na, nn_ = (torch.from_numpy(a).cuda() for a in (arcs_h, na_h, nn_h))
    A = arcs.shape[1]
    gout = torch.rand(B, generator=gen, device="cuda") * 2.0 - 1.0
    w = (torch.randn((B, A), generator=gen, device="cuda") * 0.5).requires_grad_(True)
    x = em.clone().requires_grad_(True)
    tr = trans.clone().requires_grad_(True)
    st = start.clone().requires_grad_(True)

    def score():
        return torch_loss.asg_lattice_score(em, trans, arcs, na, nn_, None, start, None, MAX_STATES)

    def score_grad_em():
        x.grad = None
        torch_loss.asg_lattice_score(x, trans, arcs, na, nn_, None, start, None, MAX_STATES).backward(gout)

    def score_grads():
        x.grad = tr.grad = st.grad = w.grad = None
        torch_loss.asg_lattice_score(x, tr, arcs, na, nn_, w, st, None, MAX_STATES).backward(gout)

    new = (("score", score), ("score+grad", score_grad_em), ("score+grads", score_grads))
    if args.new_only:
        for _, fn in new:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        return
    n = max(1, min(args.built_utterances, B))
    trans_h, start_h = trans.cpu().numpy(), start.cpu().numpy()
    built_graphs = [expanded_graph(gtn, lats[b][0], lats[b][1], trans_h, start_h) for b in range(n)]
    product_arcs = sum(g.num_arcs() for g in built_graphs) * T
    graphs = gtn.Batch(built_graphs)
    xb = em[:n].clone().contiguous()
    out_b = torch.empty(n, dtype=torch.float32, device="cuda")
    grad_b = torch.empty(n, T, C, dtype=torch.float32, device="cuda")

    def built(grad=False):
        ems = gtn.Batch.linear(n, T, C, xb, calc_grad=grad, borrow=True)
        fs = gtn.forward_score(gtn.compose(ems, graphs))
        fs.items_to_device(out_b)
        if grad:
            gtn.backward(fs)
            ems.grads_to_device(grad_b, [b * T * C for b in range(n)])
        gtn.synchronize()

    # the two routes give the same numbers
    s = score()[:n].double()
    score_grad_em()  # (gout weights the new route's gradient; the built route's is unweighted)
    built(True)
    torch.cuda.synchronize()
    gap = ((s - out_b.double()).abs() / s.abs().clamp(min=1.0)).max().item()
    ggap = (x.grad[:n] - gout[:n, None, None] * grad_b).abs().max().item()
    largest_score = s.abs().max().item()

    times = {name: best_window(torch, fn, args.windows) for name, fn in new}
    times["built"] = best_window(torch, built, args.windows)
    times["built+grad"] = best_window(torch, lambda: built(True), args.windows)
    K = int(nn_h.max())
    indeg = [np.bincount(l[0][:, 1], minlength=l[1])[l[0][:, 0]].sum() for l in lats]
    max_edges = min(8 * MAX_STATES, 1 << 21)
    rec = {
        "shape": {"B": B, "T": T, "C": C, "units": UNITS, "longest_piece": LONGEST, "nodes": K, "arcs": int(na_h.max()),
                  "edges": int(max(indeg)), "max_states": MAX_STATES, "max_edges": max_edges},
        "device": torch.cuda.get_device_name(0),
        "built_route_utterances": n,
        "built_route_product_arcs": int(product_arcs),
        "largest_relative_score_gap_between_the_routes": gap,
        "largest_gradient_gap_between_the_routes": ggap,
        "largest_absolute_score": largest_score,
        "seconds": times,
        "scores_per_second": {"score": B / times["score"], "score+grad": B / times["score+grad"],
                              "score+grads": B / times["score+grads"], "built": n / times["built"],
                              "built+grad": n / times["built+grad"]},
        "speedup_forward_per_utterance": (times["built"] / n) / (times["score"] / B),
        "speedup_forward_backward_per_utterance": (times["built+grad"] / n) / (times["score+grad"] / B),
        "scratch_bytes_per_utterance": 4.0 * (T * MAX_STATES + max_edges + 5 * MAX_STATES),
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    # (the record is written first, so that a run that misses the gate still leaves its figures behind)
    assert gap <= 1e-4, f"the routes' scores differ by {gap}"
    assert ggap <= 1e-4, f"the routes' gradients differ by {ggap}"


if __name__ == "__main__":
    main()
