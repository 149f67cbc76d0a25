"""ASG force-align scores of device-resident N-best hypotheses, and their gradients, at the shape of BASELINE config C4:
B = 512 utterances, T = 1000, C = 512 labels, four hypotheses per utterance of 192 .. 256 labels (seeded: a random label
sequence and three copies of it with one label in twenty replaced), emissions, transitions and start scores N(0, 1).

  score       torch_loss.asg_score without requires_grad: one launch
  score+grad  the same with requires_grad on emissions, transitions and start, and .backward(weights): the forward
              launch and the one gradient call (per slice an alpha, a backward and a scatter launch, then the table launch)
  graph       the route the parent commit offers for the same scores: tokens and lengths .tolist() (a download and a
              wait), then per k Batch.asg_force_align o Batch.linear -> forward_score, the items copied to the device
  graph+grad  ... each followed by backward() with unit seeds -- that route has no per-hypothesis weights -- and the
              emission gradients copied out

    python tools/bench_asg_score.py [--out profiles/asg_score_c4.json] [--windows 3]

Every figure is the best of `--windows` windows of at least half a second (at least three calls), timed with a host
clock around a closing synchronise after a warm-up of two calls.  The rates are the byte models of DESIGN section 25
over those times: `score` is one kernel; the gradient call is `score+grad` minus `score`.  A route that raises is
recorded with its message instead of a time, and nothing is run after it.  Needs a GPU; without one it fails.
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, C = 512, 1000, 512
NBEST, MIN_LENGTH, MAX_LENGTH = 4, 192, 256
WINDOW_S = 0.5


def inputs(torch):
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    em = torch.randn((B, T, C), generator=g, device="cuda", dtype=torch.float32)
    trans = torch.randn((C, C), generator=g, device="cuda", dtype=torch.float32)
    start = torch.randn((C,), generator=g, device="cuda", dtype=torch.float32)
    lengths = torch.randint(MIN_LENGTH, MAX_LENGTH + 1, (B, 1), generator=g, device="cuda").expand(B, NBEST)
    first = torch.randint(0, C, (B, 1, MAX_LENGTH), generator=g, device="cuda")
    other = torch.randint(0, C, (B, NBEST, MAX_LENGTH), generator=g, device="cuda")
    swap = torch.rand((B, NBEST, MAX_LENGTH), generator=g, device="cuda") < 0.05
    swap[:, 0] = False
    tokens = torch.where(swap, other, first.expand(B, NBEST, MAX_LENGTH)).to(torch.int32).contiguous()
    weights = torch.rand((B, NBEST), generator=g, device="cuda") * 2.0 - 1.0
    torch.cuda.synchronize()
    return em, trans, start, tokens, lengths.to(torch.int32).contiguous(), weights


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
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "asg_score_c4.json"))
    ap.add_argument("--windows", type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    import gtn_amd as gtn
    from gtn_amd import torch_loss
    if not (torch.cuda.is_available() and gtn.device_count() > 0):
        raise SystemExit("bench_asg_score: needs a GPU")
    em, trans, start, tokens, lengths, weights = inputs(torch)
    pairs = B * NBEST

    def score():
        return torch_loss.asg_score(em, trans, tokens, lengths, start=start, max_length=MAX_LENGTH)

    x = em.clone().requires_grad_(True)
    tr = trans.clone().requires_grad_(True)
    st = start.clone().requires_grad_(True)

    def score_grad():
        x.grad = tr.grad = st.grad = None
        torch_loss.asg_score(x, tr, tokens, lengths, start=st, max_length=MAX_LENGTH).backward(weights)

    table = torch_loss._asg_weights(start, trans)
    graphs = {False: torch_loss._asg_transitions_graph(C, table), True: torch_loss._asg_transitions_graph(C, table)}
    graphs[True].calc_grad = True
    out = torch.empty(NBEST, B, dtype=torch.float32, device="cuda")
    gbuf = torch.empty(B, T, C, dtype=torch.float32, device="cuda")
    offsets = np.arange(B, dtype=np.int64) * T * C

    def graph_route(grad):
        tk, lh = tokens.tolist(), lengths.tolist()  # (the download and the wait)
        torch_loss._engine_stream(em.device)
        for k in range(NBEST):
            ems = gtn.Batch.linear(B, T, C, em, calc_grad=grad, borrow=True)
            fals = gtn.Batch.asg_force_align([tk[b][k][:lh[b][k]] for b in range(B)], graphs[grad], C)
            sc = gtn.forward_score(gtn.compose(ems, fals))
            sc.items_to_device(out[k])
            if grad:
                gtn.backward(sc)
                ems.grads_to_device(gbuf, offsets)
        gtn.synchronize()

    times, errors = {}, {}
    for name, fn in (("score", score), ("score+grad", score_grad), ("graph", lambda: graph_route(False)),
                     ("graph+grad", lambda: graph_route(True))):
        try:
            times[name] = best_window(torch, fn, args.windows)
        except Exception as e:  # (recorded: the figures from here on are missing, not the record)
            errors[name] = f"{type(e).__name__}: {e}"[:300]
            break
    gap = None
    if "graph" in times and not errors:  # the two routes give the same numbers
        s = score().double()
        gap = ((s - out.t().double()).abs() / s.abs().clamp(min=1.0)).max().item()
    U = MAX_LENGTH
    fwd_bytes = pairs * (4.0 * U * T + 12.0 * U + 8.0)
    grad_bytes = 2.0 * fwd_bytes + 4.0 * fwd_bytes + 8.0 * U * pairs + 3.0 * fwd_bytes + 4.0 * B * T * C
    table_bytes = (4.0 * U * (C + 1) + 8.0 * U + 12.0) * pairs + 4.0 * C * (C + 1)
    rec = {
        "shape": {"B": B, "T": T, "C": C, "nbest": NBEST, "max_length": MAX_LENGTH},
        "device": torch.cuda.get_device_name(0),
        "hypothesis_lengths": {"mean": float(lengths.float().mean().item()), "max": int(lengths.max().item())},
        "largest_relative_gap_to_the_graph_route": gap,
        "seconds": times,
        "errors": errors,
        "speedup_forward": times["graph"] / times["score"] if "graph" in times and "score" in times else None,
        "speedup_forward_backward": (times["graph+grad"] / times["score+grad"]
                                     if "graph+grad" in times and "score+grad" in times else None),
        "scratch_bytes_unsliced": 4.0 * T * U * pairs,
    }
    if "score" in times:
        rec["byte_model"] = {"asg_score_bytes": fwd_bytes, "asg_score_GBps": fwd_bytes / times["score"] / 1e9}
        if "score+grad" in times:
            grad_call = times["score+grad"] - times["score"]
            rec["byte_model"].update({"gradient_call_bytes": grad_bytes + table_bytes,
                                      "gradient_call_seconds": grad_call,
                                      "gradient_call_GBps": (grad_bytes + table_bytes) / grad_call / 1e9
                                      if grad_call > 0 else None})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
