"""CTC posterior sampling with the results on the device at BASELINE config C3's shape (B = 512, T = 1000, C = 256),
N = 4 and N = 16 samples per utterance: the two ways.

  torch   what a caller had before Batch.ctc_sample: torch.distributions.Categorical(logits=x).sample((N,)) on the
          device (a softmax of [B, T, C] is materialised, the draw is a multinomial over it), the [N, B, T] labels
          brought to the host, merge-repeats / drop-blank there (numpy), one upload of tokens / lengths.  No logq (the
          caller would gather and sum log_softmax as well: this route is given that for free)
  sample  Batch.ctc_sample: two launches, tokens / lengths / logq written into the caller's tensors, no copy back

    python tools/bench_ctc_sample.py [--out profiles/ctc_sample_c3.json]
        alternates `torch` and `sample`, three samples each per N, every sample a process of its own that warms its
        shapes up and then times windows of at least half a second with a host clock around a closing synchronise.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_ctc_sample.py --worker trace4
        (and trace16) a few calls of `sample`, for the mean times of the two kernels;
    python tools/bench_ctc_sample.py --merge-stats DIR/.../kernel_stats.csv --n 4 [--out ...]
        adds those means, and the rows kernel's rate on its own byte model beside the stream-rate floor and beside
        linear_decode_rows_kernel on the same tensor, to the record.

Needs a GPU; a measurement path that finds none fails.
"""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_GBS = 6300.0  # the achievable HBM stream rate the floor is derived from
LINEAR_DECODE_ROWS_MS = 0.119  # linear_decode_rows_kernel on the same tensor
B, T, C = 512, 1000, 256
BLANK = 0
WINDOW_S = 0.5
SEED = 1234


def inputs(torch):
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    em = torch.rand((B, T, C), generator=g, device="cuda", dtype=torch.float32) * 10 - 5
    # a blank that holds most of the mass of about half of the frames, in runs: the collapse has work of both kinds
    em[:, :, BLANK] += (torch.rand((B, T // 8 + 1, 1), generator=g, device="cuda") < 0.5).repeat_interleave(
        8, dim=1)[:, :T, 0] * 12.0
    return torch.log_softmax(em, dim=2).contiguous()


def byte_model(N):
    """rows kernel: 4 C T read, 8 N T written (label and term); collapse kernel: 8 N T read back, 4 N T tokens, 8 N"""
    return float(B) * T * (4.0 * C + 8.0 * N), float(B) * N * (8.0 * T + 4.0 * T + 8.0)


def host_collapse(np, lab, out_tok, out_len):
    """lab [P, T] -> tokens [P, T] (-1 filled), lengths [P]"""
    prev = np.empty_like(lab)
    prev[:, 0] = -1
    prev[:, 1:] = lab[:, :-1]
    keep = (lab != prev) & (lab != BLANK)
    out_tok.fill(-1)
    for p in range(lab.shape[0]):
        idx = np.nonzero(keep[p])[0]
        out_tok[p, :idx.size] = lab[p, idx]
        out_len[p] = idx.size


def worker(kind):
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    import gtn_amd as gtn
    assert torch.cuda.is_available() and gtn.device_count() > 0, "bench_ctc_sample needs a GPU"
    N = int(kind.lstrip("abcdefghijklmnopqrstuvwxyz"))
    kind = kind.rstrip("0123456789")
    em = inputs(torch)
    tokens = torch.empty((B, N, T), dtype=torch.int32, device="cuda")
    lengths = torch.empty((B, N), dtype=torch.int32, device="cuda")
    logq = torch.empty((B, N), dtype=torch.float32, device="cuda")
    dev = torch.empty((B * N * T + B * N,), dtype=torch.int32, device="cuda")  # the torch route's one upload
    host = torch.full((B * N * T + B * N,), -1, dtype=torch.int32).pin_memory()
    h = host.numpy()
    h_tok, h_len = h[:B * N * T].reshape(B * N, T), h[B * N * T:]
    calls = [0]

    def torch_step():
        lab = torch.distributions.Categorical(logits=em).sample((N,))  # [N, B, T] int64
        lab = lab.permute(1, 0, 2).reshape(B * N, T).to(torch.int32).cpu().numpy()
        host_collapse(np, lab, h_tok, h_len)
        dev.copy_(host, non_blocking=True)

    def sample_step():
        calls[0] += 1
        ems = gtn.Batch.linear(B, T, C, em, False, True)
        ems.ctc_sample(tokens, lengths, logq, None, None, BLANK, N, SEED + calls[0], 1.0)

    def sync():
        gtn.synchronize()
        torch.cuda.synchronize()

    def timed(step):
        for _ in range(3):
            step()
        sync()
        n, t0 = 0, time.perf_counter()
        while True:
            step()
            sync()
            n += 1
            dt = time.perf_counter() - t0
            if dt >= WINDOW_S:
                return dt / n * 1e3, n

    if kind == "trace":
        for _ in range(5):
            sample_step()
            sync()
        print(json.dumps({"trace": "done"}))
        return
    c0, u0 = gtn.debug_ctc_sample_stats()
    ms, n = timed(sample_step if kind == "sample" else torch_step)
    sync()
    c1, u1 = gtn.debug_ctc_sample_stats()
    mean_len = float(lengths.float().mean().item()) if kind == "sample" else float(h_len.mean())
    rows_bytes, col_bytes = byte_model(N)
    print(json.dumps({"kind": kind, "N": N, "utterances": B, "ms_per_batch": ms, "iters": n, "mean_length": mean_len,
                      "rows_bytes": rows_bytes, "collapse_bytes": col_bytes, "sampled_utterances": u1 - u0}))


def run_worker(kind):
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", kind], env=env,
                         stdout=subprocess.PIPE, timeout=500, check=True).stdout.decode()
    rec = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    print(f"[bench_ctc_sample] {kind}: {rec['ms_per_batch']:.3f} ms per batch of {rec['utterances']}", file=sys.stderr,
          flush=True)
    return rec


def spread(v):
    return {"samples": v, "min": min(v), "max": max(v), "median": sorted(v)[len(v) // 2]}


KERNELS = ("ctc_sample_rows_kernel", "ctc_sample_collapse_kernel")
WORKERS = [k + n for k in ("torch", "sample", "trace") for n in ("4", "16")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=WORKERS)
    ap.add_argument("--merge-stats")
    ap.add_argument("--n", type=int, choices=[4, 16])
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ctc_sample_c3.json"))
    a = ap.parse_args()
    if a.worker:
        worker(a.worker)
        return
    rec = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            rec = json.load(f)
    if a.merge_stats:
        assert a.n, "--merge-stats needs --n"
        tag = f"N={a.n}"
        means = {}
        with open(a.merge_stats) as f:
            for row in csv.DictReader(f):
                for key in KERNELS:
                    if key in row["Name"]:
                        means[key] = {"calls": int(row["Calls"]), "mean_ms": float(row["AverageNs"]) * 1e-6,
                                      "min_ms": float(row["MinNs"]) * 1e-6, "max_ms": float(row["MaxNs"]) * 1e-6}
        sec = rec.setdefault(tag, {})
        sec["kernels"] = means
        rows_bytes, col_bytes = byte_model(a.n)
        k = means.get("ctc_sample_rows_kernel")
        if k:
            gbs = rows_bytes / (k["mean_ms"] * 1e-3) / 1e9
            sec["rows_kernel_on_its_byte_model"] = {
                "achieved_GBs": gbs, "stream_rate_GBs": STREAM_GBS, "frac": gbs / STREAM_GBS,
                "floor_ms": rows_bytes / (STREAM_GBS * 1e9) * 1e3, "bytes": "(4 C + 8 N) T per utterance",
                "times_linear_decode_rows_kernel": k["mean_ms"] / LINEAR_DECODE_ROWS_MS,
                "linear_decode_rows_kernel_ms": LINEAR_DECODE_ROWS_MS}
        k = means.get("ctc_sample_collapse_kernel")
        if k:
            sec["collapse_kernel_on_its_byte_model"] = {
                "achieved_GBs": col_bytes / (k["mean_ms"] * 1e-3) / 1e9, "bytes": "N (12 T + 8) per utterance"}
    else:
        for n in (4, 16):
            to, sa, lens = [], [], []
            for _ in range(3):
                r = run_worker(f"torch{n}")
                to.append(r["ms_per_batch"])
                lens.append(r["mean_length"])
                r = run_worker(f"sample{n}")
                sa.append(r["ms_per_batch"])
                lens.append(r["mean_length"])
                assert r["sampled_utterances"] > 0, r
            sec = rec.setdefault(f"N={n}", {})
            sec.update({
                "torch_route": dict(spread(to), what="Categorical(logits=x).sample((N,)) on the device + .cpu() + host "
                                    "collapse + one upload (no logq)", utterances=B),
                "sample_route": dict(spread(sa), what="Batch.ctc_sample (tokens, lengths, logq)", utterances=B),
                "speedup_median": sorted(to)[1] / sorted(sa)[1],
                "slowest_new_not_slower_than_fastest_torch": max(sa) <= min(to),
                "mean_collapsed_length": {"min": min(lens), "max": max(lens)},
            })
        rec.update({"shape": {"B": B, "T": T, "C": C, "blank": BLANK},
                    "unit": "ms per batch, host clock around a closing synchronise, windows >= 0.5 s"})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
