"""Times the pruned (banded) transducer score (gtn_amd/csrc/transducer_pruned.hip) at B 32, T 400, U 100,
S 5, C 1024, normalised, full lengths, the ranges on the diagonal: the score call, score plus gradient with the rows plane
kept (torch_loss's route) and without it (the stateless gradient call), the kernels, and the sweep's time per step.

Call timings are a host clock around a closing synchronise over windows of at least 0.5 s.  Kernel means are the engine's
own event timings (gtn_amd.prof_*, the GTNX_PROF scopes transducer_pruned_rows / _sweep / _grad) over a few steps after
the timed windows; the sweep walks T + U steps at this shape (k = t + u up to (T - 1) + U).  The baseline is the only
route a caller had before, in the same session: scatter the band into a [B, T, U + 1, C] tensor of -inf in torch,
torch_loss.transducer_loss on it, backward through the scatter; its time and its peak allocation are recorded and the
values are asserted to agree after the record is written.  Every figure is printed as soon as it exists.  Writes
profiles/transducer_pruned.json (or --out).

    python tools/bench_transducer_pruned.py [--out PATH]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, T, U, S, C = 32, 400, 100, 5, 1024


def window(fn, sync, least=0.5):
    """seconds per call of fn over a window of at least `least` seconds, closed by one synchronise"""
    fn(), sync()
    calls, t0 = 0, time.perf_counter()
    while True:
        fn()
        calls += 1
        sync()
        dt = time.perf_counter() - t0
        if dt >= least:
            return dt / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transducer_pruned.json"))
    a = ap.parse_args()
    import torch
    import gtn_amd
    import gtn_amd.torch_loss as tl
    assert torch.cuda.is_available(), "the benchmark measures the GPU and has no other route"
    sync = torch.cuda.synchronize
    rec = {"tool": "tools/bench_transducer_pruned.py", "shape": {"B": B, "T": T, "U": U, "S": S, "C": C},
           "timing": "calls: host clock, windows >= 0.5 s; kernels: the engine's event timings"}

    def fig(key, v):
        rec[key] = v
        print("FIG " + json.dumps([key, v]), flush=True)

    g = torch.Generator(device="cuda:0").manual_seed(1)
    blank = 0
    y = torch.randint(1, C, (B, U), device="cuda:0", generator=g, dtype=torch.int32)
    ranges = ((torch.arange(T, device="cuda:0") * (U + 1 - S)) // (T - 1)).to(torch.int32)[None].repeat(B, 1).contiguous()
    idx = ranges[:, :, None].long() + torch.arange(S, device="cuda:0")            # u of every band node, all <= U
    x = torch.randn(B, T, S, C, device="cuda:0", generator=g)
    x[..., blank] += 3 + 6.93  # (peaked as the tests' cases are, so that |score| stays small)
    tok = torch.gather(y.long(), 1, idx.clamp(max=U - 1).reshape(B, -1)).reshape(B, T, S, 1)
    x.scatter_add_(3, tok, (idx < U)[..., None] * torch.full((B, T, S, 1), 9.93, device="cuda:0"))
    frames = torch.full((B,), T, device="cuda:0", dtype=torch.int32)
    tlens = torch.full((B,), U, device="cuda:0", dtype=torch.int32)
    w = torch.linspace(0.5, 1.5, B, device="cuda:0")
    grad, scores = torch.empty_like(x), torch.empty(B, device="cuda:0")
    gtn_amd.set_stream(None)

    def score():
        gtn_amd.transducer_pruned_score(x, ranges, y, frames, tlens, scores, None, blank)

    def stateless():
        score()
        gtn_amd.transducer_pruned_score_grad(x, ranges, y, frames, tlens, w, grad, None, blank)

    def with_rows():
        xr = x.detach().requires_grad_(True)
        tl.transducer_pruned_score(xr, ranges, y, frames, tlens, blank).backward(w)
        return xr.grad

    def scattered():
        xr = x.detach().requires_grad_(True)
        full = torch.full((B, T, U + 1, C), float("-inf"), device="cuda:0")
        full = full.scatter(2, idx[..., None].expand(-1, -1, -1, C), xr)
        out = tl.transducer_score(full, y, frames, tlens, blank)
        out.backward(w)
        return out.detach(), xr.grad

    esync = lambda: (gtn_amd.synchronize(), sync())
    fig("score_ms", 1e3 * window(score, esync))
    fig("score_grad_stateless_ms", 1e3 * window(stateless, esync))
    fig("score_grad_with_rows_ms", 1e3 * window(with_rows, esync))

    def peak(fn):
        esync()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        esync()
        return torch.cuda.max_memory_allocated() - base

    # (torch's allocator only: the engine's pooled scratch is added from the contract)
    fig("peak_torch_bytes_above_inputs", peak(with_rows))
    fig("engine_scratch_bytes", 8 * B * T * S + 4 * B)
    fig("scatter_route", {"score_grad_ms": 1e3 * window(scattered, esync),
                          "peak_torch_bytes_above_inputs": peak(scattered),
                          "engine_scratch_bytes": 8 * B * T * (U + 1) + 4 * B})
    fig("scatter_over_pruned", rec["scatter_route"]["score_grad_ms"] / rec["score_grad_with_rows_ms"])

    gtn_amd.prof_enable(True)
    gtn_amd.prof_reset()
    for _ in range(3):
        score()
    esync()
    alpha_only = gtn_amd.prof_get("transducer_pruned_sweep")
    gtn_amd.prof_reset()
    for _ in range(3):  # (the stateless gradient call: rows, alpha and beta side by side, gradient)
        gtn_amd.transducer_pruned_score_grad(x, ranges, y, frames, tlens, w, grad, None, blank)
    esync()
    names = ("transducer_pruned_rows", "transducer_pruned_sweep", "transducer_pruned_grad")
    prof = {k: gtn_amd.prof_get(k) for k in names}
    gtn_amd.prof_enable(False)
    ms = {k: v["total_ms"] / max(v["launches"], 1) for k, v in prof.items()}
    fig("kernel_mean_ms", ms)
    steps = T + U
    fig("sweep", {"steps": steps,
                  "alpha_only_us_per_step": 1e3 * alpha_only["total_ms"] / max(alpha_only["launches"], 1) / steps,
                  "alpha_and_beta_us_per_step": 1e3 * ms["transducer_pruned_sweep"] / steps,
                  "full_lattice_us_per_step_DESIGN_42": 0.62})
    for k in ("transducer_pruned_rows", "transducer_pruned_grad"):
        if ms[k]:
            per = prof[k]["algorithmic_bytes"] / max(prof[k]["launches"], 1)
            fig(k + "_rates", {"model_bytes": per, "model_GBps": per / ms[k] / 1e6})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    want, want_g = scattered()
    stateless(), esync()
    err = (scores - want).abs().max().item()
    gerr = (grad - want_g).abs().max().item()
    print("agreement with the scatter route: score", err, "gradient", gerr, flush=True)
    rec["agreement_with_scatter_route"] = {"score_abs": err, "gradient_abs": gerr}
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    assert err <= 1e-4 * max(1.0, want.abs().max().item()) and gerr <= 1e-4, (err, gerr)


if __name__ == "__main__":
    main()
