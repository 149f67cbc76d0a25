"""Times the transducer score under an additive joint (gtn_amd/csrc/transducer_add.hip) at B 32, T 400,
U 100, C 1024, full lengths: the score call, score plus gradient with the rows plane kept (torch_loss's route) and without
it (the stateless gradient call), and the kernels.

Call timings are a host clock around a closing synchronise over windows of at least 0.5 s.  Kernel means are the engine's
own event timings (gtn_amd.prof_*, the GTNX_PROF scopes transducer_add_max / _norm / _grad and transducer_sweep) over a
few steps after the timed windows.  For the two MFMA kernels: the float32 matrix rate (2 B T (U + 1) C flop per product;
norm has one product, grad two) and the bytes of the engine's own model over the kernel's time.  The baseline is the
route a caller had before, in the same session: am[:, :, None] + lm[:, None] in torch, torch_loss.transducer_loss, backward
through the broadcast; both times and both peak allocations are recorded and the values are asserted to agree after the
record is written.  Every figure is printed as soon as it exists.  Writes profiles/transducer_add.json (or --out).

    python tools/bench_transducer_add.py [--out PATH]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, T, U, C = 32, 400, 100, 1024


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transducer_add.json"))
    a = ap.parse_args()
    import torch
    import gtn_amd
    import gtn_amd.torch_loss as tl
    assert torch.cuda.is_available(), "the benchmark measures the GPU and has no other route"
    sync = torch.cuda.synchronize
    rec = {"tool": "tools/bench_transducer_add.py", "shape": {"B": B, "T": T, "U": U, "C": C},
           "timing": "calls: host clock, windows >= 0.5 s; kernels: the engine's event timings"}

    def fig(key, v):
        rec[key] = v
        print("FIG " + json.dumps([key, v]), flush=True)

    g = torch.Generator(device="cuda:0").manual_seed(1)
    blank = 0
    y = torch.randint(1, C, (B, U), device="cuda:0", generator=g, dtype=torch.int32)
    am = torch.randn(B, T, C, device="cuda:0", generator=g)
    lm = torch.randn(B, U + 1, C, device="cuda:0", generator=g)
    am[..., blank] += 3 + 6.93  # (peaked as the tests' cases are, so that |score| stays small)
    lm[:, :U].scatter_add_(2, y.long()[:, :, None], torch.full((B, U, 1), 9.93, device="cuda:0"))
    frames = torch.full((B,), T, device="cuda:0", dtype=torch.int32)
    tlens = torch.full((B,), U, device="cuda:0", dtype=torch.int32)
    w = torch.linspace(0.5, 1.5, B, device="cuda:0")
    ga, gl, scores = torch.empty_like(am), torch.empty_like(lm), torch.empty(B, device="cuda:0")
    gtn_amd.set_stream(None)

    def score():
        gtn_amd.transducer_add_score(am, lm, y, frames, tlens, scores, None, blank)

    def stateless():
        score()
        gtn_amd.transducer_add_score_grad(am, lm, y, frames, tlens, w, ga, gl, None, blank)

    def with_rows():
        ar, lr = am.detach().requires_grad_(True), lm.detach().requires_grad_(True)
        tl.transducer_add_score(ar, lr, y, frames, tlens, blank).backward(w)
        return ar.grad, lr.grad

    def materialised():
        ar, lr = am.detach().requires_grad_(True), lm.detach().requires_grad_(True)
        out = tl.transducer_score(ar[:, :, None] + lr[:, None], y, frames, tlens, blank)
        out.backward(w)
        return out.detach(), ar.grad, lr.grad

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

    # (torch's allocator only: the engine's pooled scratch, 20 bytes per node, is added from the contract)
    fig("peak_torch_bytes_above_inputs", peak(with_rows))
    fig("engine_scratch_bytes", 20 * B * T * (U + 1) + 4 * B * (T + U + 1))
    fig("materialised_route", {"score_grad_ms": 1e3 * window(materialised, esync),
                               "peak_torch_bytes_above_inputs": peak(materialised),
                               "engine_scratch_bytes": 8 * B * T * (U + 1)})
    fig("materialised_over_additive", rec["materialised_route"]["score_grad_ms"] / rec["score_grad_with_rows_ms"])

    gtn_amd.prof_enable(True)
    gtn_amd.prof_reset()
    for _ in range(3):
        score()
        with_rows()
    esync()
    names = ("transducer_add_max", "transducer_add_norm", "transducer_sweep", "transducer_add_grad")
    prof = {k: gtn_amd.prof_get(k) for k in names}
    gtn_amd.prof_enable(False)
    ms = {k: v["total_ms"] / max(v["launches"], 1) for k, v in prof.items()}
    fig("kernel_mean_ms", ms)
    flop = 2.0 * B * T * (U + 1) * C
    for k, products in (("transducer_add_norm", 1), ("transducer_add_grad", 2)):
        if ms[k]:
            fig(k + "_rates", {"matrix_TFLOPs": products * flop / ms[k] / 1e9,
                               "model_bytes": prof[k]["algorithmic_bytes"] / max(prof[k]["launches"], 1),
                               "model_GBps": prof[k]["algorithmic_bytes"] / max(prof[k]["launches"], 1) / ms[k] / 1e6})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    want, want_ga, want_gl = materialised()
    stateless(), esync()
    err = (scores - want).abs().max().item()
    gerr = max(((ga - want_ga).abs() / want_ga.abs().clamp(min=1)).max().item(),
               ((gl - want_gl).abs() / want_gl.abs().clamp(min=1)).max().item())
    print("agreement with the materialised route: score", err, "gradients over max(1, |want|)", gerr, flush=True)
    assert err <= 1e-4 * max(1.0, want.abs().max().item()) and gerr <= 1e-4, (err, gerr)


if __name__ == "__main__":
    main()
