"""CTC scores of word-piece lattices, and their gradients, at BASELINE config C3's shape: B = 512 utterances, T = 1000,
C = 256, transcripts of 100 units over a 26-letter alphabet, every piece of up to 4 units in the inventory (labels 1 ..
255 by a fixed hash of the piece), so each lattice has 101 nodes, 394 arcs and 495 states; max_states = 512.  The
emissions are a seeded log-softmax tensor with the blank ahead in seven of eight blocks of eight frames, as in
tools/bench_ctc_score.py.

  score         torch_loss.ctc_lattice_score without requires_grad: one launch
  score+grad    the same with requires_grad and .backward(g): the forward launch and the one gradient call
  score+grad+w  ... with learned arc weights that require a gradient as well
  built         the route the parent commit offers for the same numbers: the alignment graph of every lattice built as a
                Graph (one blank state per node, one token state per arc), intersected with Batch.linear through the
                built-lattice path, forward_score on the result
  built+grad    ... and backward() with the emission gradients written out
The built route composes every product (about 2 800 arcs per lattice times T frames), so it runs on the first
`--built-utterances` utterances only (default 16) and the record gives both routes per utterance as well.  The tool
asserts that the two routes agree within the gate of the tests on those utterances: scores within 1e-4 max(1, |score|),
gradients within 1e-4.

    python tools/bench_ctc_lattice.py [--out profiles/ctc_lattice_c3.json] [--windows 3] [--built-utterances 16]
    python tools/bench_ctc_lattice.py --new-only          (the new route alone: what a kernel trace is taken of)
    python tools/bench_ctc_lattice.py --kernel-stats X.csv  (adds the ctc_lattice rows of a rocprofv3 --kernel-trace
                                                             --stats run of --new-only to the record; no GPU needed)

Every figure is the best of `--windows` windows of at least half a second (at least three calls), timed with a host
clock around a closing synchronise after a warm-up of two calls.  The rates are the byte models of DESIGN section 35
over those times.  Needs a GPU; without one it fails.
"""
import argparse
import csv
import json
import os
import sys
import time
import zlib

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, C = 512, 1000, 256
BLANK, UNITS, LONGEST, MAX_STATES = 0, 100, 4, 512
WINDOW_S = 0.5


def lattices(gtn):
    rng = np.random.default_rng(1234)
    out = []
    for _ in range(B):
        units = "".join(chr(97 + int(c)) for c in rng.integers(0, 26, UNITS))
        pieces = {units[i:j]: 1 + zlib.crc32(units[i:j].encode()) % (C - 1)
                  for i in range(UNITS) for j in range(i + 1, min(UNITS, i + LONGEST) + 1)}
        out.append(gtn.decomposition_lattice(units, pieces))
    return out


def alignment_graph(gtn, arcs, K):
    """the CTC alignment graph of a lattice without weights as a Graph"""
    src, dst, lab = (arcs[:, i].astype(np.int64) for i in range(3))
    A = len(arcs)
    g = gtn.Graph(False)
    start = np.arange(K + A) == 0  # (the start node's blank alone: frame 0 stays there or enters an arc that leaves it)
    accept = np.concatenate([np.arange(K) == K - 1, dst == K - 1])
    g.add_nodes(start.tolist(), accept.tolist())
    tok = K + np.arange(A)
    follow = [(K + p, K + a, lab[a]) for a in range(A) for p in np.nonzero((dst == src[a]) & (lab != lab[a]))[0]]
    f = np.array(follow, dtype=np.int64).reshape(-1, 3)
    s = np.concatenate([np.arange(K), tok, src, tok, f[:, 0]])
    d = np.concatenate([np.arange(K), tok, tok, dst, f[:, 1]])
    l = np.concatenate([np.full(K, BLANK), lab, lab, np.full(A, BLANK), f[:, 2]])
    g.add_arcs(s.astype(np.int32), d.astype(np.int32), l.astype(np.int32))
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


def merge_kernel_stats(out, path):
    with open(out) as f:
        rec = json.load(f)
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if "ctc_lattice" in r.get("Name", "")]
    rec["kernel_stats"] = [{"name": r["Name"], "calls": int(r["Calls"]),
                            "average_ns": float(r["AverageNs"]), "total_ns": float(r["TotalDurationNs"])} for r in rows]
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["kernel_stats"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ctc_lattice_c3.json"))
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--built-utterances", type=int, default=16)
    ap.add_argument("--new-only", action="store_true")
    ap.add_argument("--kernel-stats")
    args = ap.parse_args()
    if args.kernel_stats:
        return merge_kernel_stats(args.out, args.kernel_stats)
    sys.path.insert(0, HERE)
    import torch
    import gtn_amd as gtn
    from gtn_amd import torch_loss
    if not (torch.cuda.is_available() and gtn.device_count() > 0):
        raise SystemExit("bench_ctc_lattice: needs a GPU")
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
    gout = torch.rand(B, generator=gen, device="cuda") * 2.0 - 1.0
    w = (torch.randn((B, A), generator=gen, device="cuda") * 0.5).requires_grad_(True)
    x = em.clone().requires_grad_(True)

    def score():
        return torch_loss.ctc_lattice_score(em, arcs, na, nn_, None, BLANK, None, MAX_STATES)

    def score_grad():
        x.grad = None
        torch_loss.ctc_lattice_score(x, arcs, na, nn_, None, BLANK, None, MAX_STATES).backward(gout)

    def score_grad_w():
        x.grad = w.grad = None
        torch_loss.ctc_lattice_score(x, arcs, na, nn_, w, BLANK, None, MAX_STATES).backward(gout)

    new = (("score", score), ("score+grad", score_grad), ("score+grad+w", score_grad_w))
    if args.new_only:
        for _, fn in new:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        return
    n = max(1, min(args.built_utterances, B))
    built_graphs = [alignment_graph(gtn, lats[b][0], lats[b][1]) for b in range(n)]
    product_arcs = sum(g.num_arcs() for g in built_graphs) * T
    graphs = gtn.Batch(built_graphs)
    xb = em[:n].clone().contiguous()
    out_b = torch.empty(n, dtype=torch.float32, device="cuda")
    grad_b = torch.empty(n, T, C, dtype=torch.float32, device="cuda")

    def built(grad=False):
        ems = gtn.Batch.linear(n, T, C, xb, calc_grad=grad, borrow=True)
        fs = gtn.forward_score(gtn.intersect(graphs, ems))
        fs.items_to_device(out_b)
        if grad:
            gtn.backward(fs)
            ems.grads_to_device(grad_b, [b * T * C for b in range(n)])
        gtn.synchronize()

    # the two routes give the same numbers
    s = score()[:n].double()
    score_grad()  # (gout weights the new route's gradient; the built route's is unweighted)
    built(True)
    torch.cuda.synchronize()
    gap = ((s - out_b.double()).abs() / s.abs().clamp(min=1.0)).max().item()
    ggap = (x.grad[:n] - gout[:n, None, None] * grad_b).abs().max().item()
    largest_score = s.abs().max().item()

    times = {name: best_window(torch, fn, args.windows) for name, fn in new}
    times["built"] = best_window(torch, built, args.windows)
    times["built+grad"] = best_window(torch, lambda: built(True), args.windows)
    K, S = int(nn_h.max()), int((na_h + nn_h).max())
    lattice_bytes = 12.0 * A + 12.0
    fwd_bytes = B * (4.0 * S * T + lattice_bytes)
    grad_bytes = 2.0 * fwd_bytes + 3.0 * fwd_bytes + 4.0 * B * T * C
    grad_call = times["score+grad"] - times["score"]
    rec = {
        "shape": {"B": B, "T": T, "C": C, "units": UNITS, "longest_piece": LONGEST, "nodes": K, "arcs": int(na_h.max()),
                  "states": S, "max_states": MAX_STATES},
        "device": torch.cuda.get_device_name(0),
        "built_route_utterances": n,
        "built_route_product_arcs": int(product_arcs),
        "largest_relative_score_gap_between_the_routes": gap,
        "largest_gradient_gap_between_the_routes": ggap,
        "largest_absolute_score": largest_score,
        "seconds": times,
        "losses_per_second": {"score": B / times["score"], "score+grad": B / times["score+grad"],
                              "score+grad+w": B / times["score+grad+w"], "built": n / times["built"],
                              "built+grad": n / times["built+grad"]},
        "speedup_forward_per_utterance": (times["built"] / n) / (times["score"] / B),
        "speedup_forward_backward_per_utterance": (times["built+grad"] / n) / (times["score+grad"] / B),
        "byte_model": {"ctc_lattice_bytes": fwd_bytes, "ctc_lattice_GBps": fwd_bytes / times["score"] / 1e9,
                       "gradient_call_bytes": grad_bytes, "gradient_call_seconds": grad_call,
                       "gradient_call_GBps": grad_bytes / grad_call / 1e9 if grad_call > 0 else None,
                       "fraction_of_8_TBps": fwd_bytes / times["score"] / 8e12},
        "scratch_bytes_unsliced": 4.0 * T * MAX_STATES * B,
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
