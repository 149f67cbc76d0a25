"""Exact CTC scores of device-resident N-best hypotheses, and their gradient, at BASELINE config C3's shape: B = 512
utterances, T = 1000, C = 256, hypotheses from `ctc_beam_decode` (beam_size 16, cutoff_top_n 16, nbest 4) on a seeded
log-softmax tensor made as the bench tensor of tools/bench_ctc_beam.py is, with blank ahead in seven of eight blocks of
eight frames instead of every other one, which shortens the hypotheses: 243 labels on average and 321 at most, so 609
of the 2048 are still above the max_length of 256 this tool runs with and score -inf without being swept (the loss
route sweeps them all; the record counts them).

  score       torch_loss.ctc_score without requires_grad: one launch
  score+grad  the same with requires_grad and .backward(weights): the forward launch and the one gradient call
  loss        the route the parent commit offers for the same numbers: tokens and lengths .tolist() (a download and a
              wait), then nbest calls of ctc_loss on the same tensor, one hypothesis per utterance each
  loss+grad   ... each followed by .backward(weights[:, k]), the gradients summed by autograd

    python tools/bench_ctc_score.py [--out profiles/ctc_score_c3.json] [--windows 3]

Every figure is the best of `--windows` windows of at least half a second (at least three calls), timed with a host
clock around a closing synchronise after a warm-up of two calls.  The rates are the byte models of DESIGN section 22.4
over those times: `score` is one kernel; the gradient call is `score+grad` minus `score` and runs two kernels per slice.
Needs a GPU; without one it fails.
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, C = 512, 1000, 256
BLANK, BEAM, TOPN, NBEST, MAX_LENGTH = 0, 16, 16, 4, 256
WINDOW_S = 0.5


def inputs(torch, torch_loss):
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    em = torch.randn((B, T, C), generator=g, device="cuda", dtype=torch.float32) * 3.0
    em[:, :, BLANK] += (torch.rand((B, T // 8 + 1, 1), generator=g, device="cuda") < 0.875).repeat_interleave(
        8, dim=1)[:, :T, 0] * 12.0
    em = torch.log_softmax(em, dim=2).contiguous()
    tokens, lengths, beam = torch_loss.ctc_beam_decode(em, BLANK, None, BEAM, TOPN, NBEST)
    weights = torch.rand((B, NBEST), generator=g, device="cuda") * 2.0 - 1.0
    torch.cuda.synchronize()
    return em, tokens, lengths, beam, weights


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
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ctc_score_c3.json"))
    ap.add_argument("--windows", type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    import gtn_amd as gtn
    from gtn_amd import torch_loss
    if not (torch.cuda.is_available() and gtn.device_count() > 0):
        raise SystemExit("bench_ctc_score: needs a GPU")
    em, tokens, lengths, beam, weights = inputs(torch, torch_loss)
    pairs = B * NBEST
    ln = lengths.clamp(0, T)
    too_long = int((ln > MAX_LENGTH).sum().item())

    def score():
        return torch_loss.ctc_score(em, tokens, lengths, BLANK, None, MAX_LENGTH)

    x = em.clone().requires_grad_(True)

    def score_grad():
        x.grad = None
        torch_loss.ctc_score(x, tokens, lengths, BLANK, None, MAX_LENGTH).backward(weights)

    def host_targets():
        tk, lh = tokens.tolist(), lengths.tolist()  # (the download and the wait)
        return [[tk[b][k][:lh[b][k]] for b in range(B)] for k in range(NBEST)]

    def loss():
        return [torch_loss.ctc_loss(em, tg, BLANK) for tg in host_targets()]

    def loss_grad():
        x.grad = None
        for k, tg in enumerate(host_targets()):
            torch_loss.ctc_loss(x, tg, BLANK).backward(weights[:, k])

    # the two routes give the same numbers: score == forwardScore(x) - loss
    s = score()
    norm = torch.logsumexp(em.double(), dim=2).sum(dim=1)
    via_loss = norm[:, None] - torch.stack(loss(), dim=1).double()
    ok = ln <= MAX_LENGTH
    gap = ((s.double() - via_loss).abs() / s.double().abs().clamp(min=1.0))[ok]
    gap = gap.max().item() if gap.numel() else None

    times = {name: best_window(torch, fn, args.windows) for name, fn in
             (("score", score), ("score+grad", score_grad), ("loss", loss), ("loss+grad", loss_grad))}
    SM = 2 * MAX_LENGTH + 1
    fwd_bytes = pairs * (4.0 * SM * T + 4.0 * MAX_LENGTH + 8.0)
    grad_bytes = 2.0 * fwd_bytes + 4.0 * fwd_bytes + 4.0 * B * T * C
    grad_call = times["score+grad"] - times["score"]
    rec = {
        "shape": {"B": B, "T": T, "C": C, "beam_size": BEAM, "cutoff_top_n": TOPN, "nbest": NBEST,
                  "max_length": MAX_LENGTH},
        "device": torch.cuda.get_device_name(0),
        "hypothesis_lengths": {"mean": float(ln.float().mean().item()), "max": int(ln.max().item()),
                               "above_max_length": too_long},
        "largest_relative_gap_to_the_loss_route": gap,
        "seconds": times,
        "speedup_forward": times["loss"] / times["score"],
        "speedup_forward_backward": times["loss+grad"] / times["score+grad"],
        "byte_model": {"ctc_score_bytes": fwd_bytes, "ctc_score_GBps": fwd_bytes / times["score"] / 1e9,
                       "gradient_call_bytes": grad_bytes, "gradient_call_seconds": grad_call,
                       "gradient_call_GBps": grad_bytes / grad_call / 1e9 if grad_call > 0 else None},
        "scratch_bytes_unsliced": 4.0 * T * SM * pairs,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
