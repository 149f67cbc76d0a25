"""Times the batched token-and-duration transducer (TDT) score (gtn_amd/csrc/transducer_tdt.hip) at
B 32, T 400, U 100, full lengths, for C 1025 + D 5 (a row of 1030 entries: 4-byte loads) and C 1024 + D 4 (1028 entries:
16-byte loads): the score call, score plus gradient with the rows plane kept (torch_loss's route) and without it (the
stateless gradient call), and the three kernels.

Timing as tools/bench_transducer.py: a host clock around a closing synchronise over windows of at least 0.5 s for the
calls, the engine's own event timings (the GTNX_PROF scopes transducer_tdt_rows / _sweep / _grad) for the kernels.  From
them the rows and gradient kernels' rates on 4 N and 8 N bytes for N live logits and the sweep's microseconds per step
(T + U / K steps), beside the classical transducer_score on the first 1024 entries of the same rows in the same session.
The same computation in plain torch (two log_softmax, gathers, an anti-diagonal logsumexp loop over the 2 D - 1 arcs into
a node, autograd) runs on the same tensors in the same session: a stated baseline, not a target, and the values are
asserted to agree after the record is written.  Every figure is printed as soon as it exists.  Writes
profiles/transducer_tdt.json (or --out).

    python tools/bench_transducer_tdt.py [--out PATH] [--skip-torch]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_transducer import window  # noqa: E402

B, T, U = 32, 400, 100
SHAPES = [(1025, 5), (1024, 4)]  # (C, D)


def torch_route(x, y, blank, C):
    """the TDT log score of full-length utterances in plain torch: one logsumexp per anti-diagonal t + u = k"""
    import torch
    Bn, Tn, U1, CD = x.shape
    D = CD - C
    lt, ld = torch.log_softmax(x[..., :C], -1), torch.log_softmax(x[..., C:], -1)
    lpl = torch.gather(lt[:, :, :-1], 3, y.long()[:, None, :, None].expand(-1, Tn, -1, 1))[..., 0]
    neg = torch.full((), float("-inf"), device=x.device)
    wb = lt[..., blank, None] + ld                                              # [B, T, U + 1, D]
    wl = torch.cat([lpl, neg.expand(Bn, Tn, 1)], 2)[..., None] + ld
    diags, los = [torch.zeros(Bn, 1, device=x.device)], [0]  # alpha on the anti-diagonal, indexed by u from lo
    for k in range(1, Tn + U1 - 1):
        lo, hi = max(0, k - Tn + 1), min(k, U1 - 1)
        u = torch.arange(lo, hi + 1, device=x.device)
        t = k - u
        terms = []
        for d in range(D):
            for label in (False, True):
                ks = k - d - int(label)  # the source node's anti-diagonal
                if ks < 0 or (d == 0 and not label):
                    continue
                us, ts = u - int(label), t - d
                ok = (ts >= 0) & (us >= los[ks]) & (us < los[ks] + diags[ks].shape[1])
                src = diags[ks][:, (us - los[ks]).clamp(0, diags[ks].shape[1] - 1)]
                terms.append(torch.where(ok, src + (wl if label else wb)[:, ts.clamp(min=0), us.clamp(min=0), d], neg))
        diags.append(torch.logsumexp(torch.stack(terms, 0), 0))
        los.append(lo)
    ends = [diags[Tn - d + U1 - 1][:, U1 - 1 - los[Tn - d + U1 - 1]] + wb[:, Tn - d, U1 - 1, d]
            for d in range(1, min(D - 1, Tn) + 1)]
    return torch.logsumexp(torch.stack(ends, 0), 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transducer_tdt.json"))
    ap.add_argument("--skip-torch", action="store_true")
    a = ap.parse_args()
    import torch
    import gtn_amd
    import gtn_amd.torch_loss as tl
    assert torch.cuda.is_available(), "the benchmark measures the GPU and has no other route"
    sync = torch.cuda.synchronize
    esync = lambda: (gtn_amd.synchronize(), sync())
    rec = {"tool": "tools/bench_transducer_tdt.py", "shape": {"B": B, "T": T, "U": U, "C_D": SHAPES},
           "timing": "calls: host clock, windows >= 0.5 s; kernels: the engine's event timings"}

    def fig(key, v):
        rec[key] = v
        print("FIG " + json.dumps([key, v]), flush=True)

    def means(names):
        prof = {k: gtn_amd.prof_get(k) for k in names}
        return {k: v["total_ms"] / max(v["launches"], 1) for k, v in prof.items()}

    gtn_amd.set_stream(None)
    blank, K = 0, 2  # (K = ceil(101 / 64))
    frames = torch.full((B,), T, device="cuda:0", dtype=torch.int32)
    tlens = torch.full((B,), U, device="cuda:0", dtype=torch.int32)
    w = torch.linspace(0.5, 1.5, B, device="cuda:0")
    scores = torch.empty(B, device="cuda:0")
    checks = []
    for C, D in SHAPES:
        tag = f"C{C}_D{D}"
        g = torch.Generator(device="cuda:0").manual_seed(1)
        y = torch.randint(1, C, (B, U), device="cuda:0", generator=g, dtype=torch.int32)
        x = torch.randn(B, T, U + 1, C + D, device="cuda:0", generator=g)
        x[..., blank] += 3 + 6.93  # (peaked as the tests' cases are, so that |score| stays small)
        x[:, :, :U].scatter_add_(3, y.long()[:, None, :, None].expand(-1, T, -1, 1),
                                 torch.full((B, T, U, 1), 9.93, device="cuda:0"))
        N = float(B) * T * (U + 1) * (C + D)  # live logits
        grad = torch.empty_like(x)

        def score():
            gtn_amd.transducer_tdt_score(x, y, frames, tlens, scores, D, None, blank)

        def stateless():
            score()
            gtn_amd.transducer_tdt_score_grad(x, y, frames, tlens, w, grad, D, None, blank)

        def with_rows():
            xr = x.detach().requires_grad_(True)
            tl.transducer_tdt_score(xr, y, frames, tlens, D, blank).backward(w)

        fig(tag + "_score_ms", 1e3 * window(score, esync))
        fig(tag + "_score_grad_stateless_ms", 1e3 * window(stateless, esync))
        fig(tag + "_score_grad_with_rows_ms", 1e3 * window(with_rows, esync))
        gtn_amd.prof_enable(True)
        gtn_amd.prof_reset()
        for _ in range(3):
            score()
            with_rows()
        esync()
        ms = means(("transducer_tdt_rows", "transducer_tdt_sweep", "transducer_tdt_grad"))
        gtn_amd.prof_enable(False)
        fig(tag + "_kernel_mean_ms", ms)
        fig(tag + "_rates", {"rows_GBps_on_4N": 4 * N / ms["transducer_tdt_rows"] / 1e6,
                             "grad_GBps_on_8N": 8 * N / ms["transducer_tdt_grad"] / 1e6,
                             "sweep_us_per_step": 1e3 * ms["transducer_tdt_sweep"] / (T + U // K)})
        if not a.skip_torch:
            def torch_step():
                xr = x.detach().requires_grad_(True)
                out = torch_route(xr, y, blank, C)
                out.backward(w)
                return out.detach(), xr.grad
            import time
            torch_step(), sync()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            want, want_grad = torch_step()
            sync()
            fig(tag + "_torch_route", {"score_grad_ms": 1e3 * (time.perf_counter() - t0),
                                       "peak_bytes_above_inputs": torch.cuda.max_memory_allocated() - base})
            stateless(), esync()
            checks.append((tag, (scores - want).abs().max().item(), want.abs().max().item(),
                           (grad - want_grad).abs().max().item()))
            fig(tag + "_agreement", {"score": checks[-1][1], "gradient": checks[-1][3]})
            del want, want_grad
        if (C, D) == SHAPES[-1]:  # section 42's kernels on the first 1024 entries of the same rows, same session
            xc = x[..., :1024].contiguous()
            gtn_amd.prof_enable(True)
            gtn_amd.prof_reset()
            for _ in range(3):
                gtn_amd.transducer_score(xc, y, frames, tlens, scores, None, blank, True)
                tl.transducer_score(xc.detach().requires_grad_(True), y, frames, tlens, blank).backward(w)
            esync()
            ms = means(("transducer_rows", "transducer_sweep", "transducer_grad"))
            gtn_amd.prof_enable(False)
            n = float(B) * T * (U + 1) * 1024
            fig("classical_C1024_kernel_mean_ms", ms)
            fig("classical_C1024_rates", {"rows_GBps_on_4N": 4 * n / ms["transducer_rows"] / 1e6,
                                          "grad_GBps_on_8N": 8 * n / ms["transducer_grad"] / 1e6,
                                          "sweep_us_per_step": 1e3 * ms["transducer_sweep"] / (T + U // K)})
            del xc
        del x, grad
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    for tag, err, top, gerr in checks:
        assert err <= 1e-4 * max(1.0, top) and gerr <= 1e-4, (tag, err, gerr)


if __name__ == "__main__":
    main()
