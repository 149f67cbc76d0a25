"""Times the batched transducer (RNN-T) score (gtn_amd/csrc/transducer.hip) at B 32, T 400, U 100,
C 1024, normalised, full lengths: the score call, score plus gradient with the rows plane kept (torch_loss's route) and
without it (the stateless gradient call), and the three kernels.

Call timings are a host clock around a closing synchronise over windows of at least 0.5 s.  Kernel means are the
engine's own event timings (gtn_amd.prof_*, the GTNX_PROF scopes transducer_rows / _sweep / _grad) over a few steps after
the timed windows.  From them: the rows and gradient kernels' rates on their byte models (4 N and 8 N bytes for N live
logits) beside linear_decode_rows on the same tensor seen as [B, T (U + 1), C] in the same session, and the sweep's
microseconds per step (T + U / K steps).  The same computation in plain torch (log_softmax, gathers, an anti-diagonal
logaddexp loop, autograd) runs on the same tensors in the same session: its time and peak memory are a stated baseline,
not a target, and the values are asserted to agree after the record is written.  Every figure is printed as soon as it
exists.  Writes profiles/transducer.json (or --out).

    python tools/bench_transducer.py [--out PATH] [--skip-torch]
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


def torch_route(x, y, blank):
    """log P(y | x) of full-length utterances in plain torch: one logaddexp per anti-diagonal"""
    import torch
    lp = torch.log_softmax(x, -1)
    lpb = lp[..., blank]                                                      # [B, T, U + 1]
    lpl = torch.gather(lp[:, :, :-1], 3, y.long()[:, None, :, None].expand(-1, lp.shape[1], -1, 1))[..., 0]
    Bn, Tn, U1 = lpb.shape
    neg = torch.full((Bn, 1), float("-inf"), device=x.device)
    diag = torch.zeros(Bn, 1, device=x.device)  # alpha on the anti-diagonal t + u = d, indexed by u from lo
    lo = 0
    for d in range(1, Tn + U1 - 1):
        nlo, nhi = max(0, d - Tn + 1), min(d, U1 - 1)
        u = torch.arange(nlo, nhi + 1, device=x.device)
        t = d - u
        prev = torch.cat([neg, diag, neg], 1)  # prev[:, 1 + (u' - lo)] = alpha[d - 1 - u', u']
        up_ok, left_ok = t >= 1, u >= 1
        up = prev[:, (u - lo + 1).clamp(0, prev.shape[1] - 1)] + lpb[:, (t - 1).clamp(min=0), u]
        left = prev[:, (u - 1 - lo + 1).clamp(0, prev.shape[1] - 1)] + lpl[:, t, (u - 1).clamp(min=0)]
        diag = torch.logaddexp(torch.where(up_ok, up, neg), torch.where(left_ok, left, neg))
        lo = nlo
    return diag[:, 0] + lpb[:, Tn - 1, U1 - 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transducer.json"))
    ap.add_argument("--skip-torch", action="store_true")
    a = ap.parse_args()
    import torch
    import gtn_amd
    import gtn_amd.torch_loss as tl
    assert torch.cuda.is_available(), "the benchmark measures the GPU and has no other route"
    sync = torch.cuda.synchronize
    rec = {"tool": "tools/bench_transducer.py", "shape": {"B": B, "T": T, "U": U, "C": C, "normalize": True},
           "timing": "calls: host clock, windows >= 0.5 s; kernels: the engine's event timings"}

    def fig(key, v):
        rec[key] = v
        print("FIG " + json.dumps([key, v]), flush=True)

    g = torch.Generator(device="cuda:0").manual_seed(1)
    blank = 0
    y = torch.randint(1, C, (B, U), device="cuda:0", generator=g, dtype=torch.int32)
    x = torch.randn(B, T, U + 1, C, device="cuda:0", generator=g)
    x[..., blank] += 3 + 6.93  # (peaked as the tests' cases are, so that |score| stays small)
    x[:, :, :U].scatter_add_(3, y.long()[:, None, :, None].expand(-1, T, -1, 1), torch.full((B, T, U, 1), 9.93, device="cuda:0"))
    frames = torch.full((B,), T, device="cuda:0", dtype=torch.int32)
    tlens = torch.full((B,), U, device="cuda:0", dtype=torch.int32)
    w = torch.linspace(0.5, 1.5, B, device="cuda:0")
    N = float(B) * T * (U + 1) * C  # live logits
    grad = torch.empty_like(x)
    scores = torch.empty(B, device="cuda:0")
    gtn_amd.set_stream(None)

    def score():
        gtn_amd.transducer_score(x, y, frames, tlens, scores, None, blank, True)

    def stateless():
        score()
        gtn_amd.transducer_score_grad(x, y, frames, tlens, w, grad, None, blank, True)

    def with_rows():
        xr = x.detach().requires_grad_(True)
        tl.transducer_score(xr, y, frames, tlens, blank).backward(w)

    esync = lambda: (gtn_amd.synchronize(), sync())
    fig("score_ms", 1e3 * window(score, esync))
    fig("score_grad_stateless_ms", 1e3 * window(stateless, esync))
    fig("score_grad_with_rows_ms", 1e3 * window(with_rows, esync))

    gtn_amd.prof_enable(True)
    gtn_amd.prof_reset()
    for _ in range(3):
        score()
        with_rows()
    try:
        tl.ctc_decode(x.view(B, T * (U + 1), C))
        tl.ctc_decode(x.view(B, T * (U + 1), C))
    except Exception as e:
        fig("linear_decode_rows", "failed: " + str(e).splitlines()[0])
    esync()
    prof = {k: gtn_amd.prof_get(k) for k in ("transducer_rows", "transducer_sweep", "transducer_grad", "linear_decode_rows")}
    gtn_amd.prof_enable(False)
    ms = {k: v["total_ms"] / max(v["launches"], 1) for k, v in prof.items()}
    fig("kernel_mean_ms", ms)
    if ms["transducer_rows"] and ms["transducer_grad"]:
        rates = {"rows_GBps_on_4N": 4 * N / ms["transducer_rows"] / 1e6, "grad_GBps_on_8N": 8 * N / ms["transducer_grad"] / 1e6}
        if ms["linear_decode_rows"]:
            rates["linear_decode_rows_GBps_on_4N"] = 4 * N / ms["linear_decode_rows"] / 1e6
            rates["rows_over_linear_decode_rows"] = rates["rows_GBps_on_4N"] / rates["linear_decode_rows_GBps_on_4N"]
            rates["grad_over_linear_decode_rows"] = rates["grad_GBps_on_8N"] / rates["linear_decode_rows_GBps_on_4N"]
        fig("stream_rates", rates)
        K = 2  # ceil(101 / 64)
        fig("sweep_us_per_step", 1e3 * ms["transducer_sweep"] / (T + U // K))

    if a.skip_torch:
        fig("torch_route", "not measured")
    else:
        def torch_step():
            xr = x.detach().requires_grad_(True)
            out = torch_route(xr, y, blank)
            out.backward(w)
            return out.detach(), xr.grad
        torch_step(), sync()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        want, want_grad = torch_step()
        sync()
        fig("torch_route", {"score_grad_ms": 1e3 * (time.perf_counter() - t0),
                            "peak_bytes_above_inputs": torch.cuda.max_memory_allocated() - base})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    if not a.skip_torch:
        stateless(), esync()
        err = (scores - want).abs().max().item()
        gerr = (grad - want_grad).abs().max().item()
        print("agreement with the torch route: score", err, "gradient", gerr, flush=True)
        assert err <= 1e-4 * max(1.0, want.abs().max().item()) and gerr <= 1e-4, (err, gerr)


if __name__ == "__main__":
    main()
