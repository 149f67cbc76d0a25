#!/usr/bin/env python3
"""bench.py -- CTC forward+backward losses/sec (BASELINE.json metric).

One "step" = one pass of the hot path over one batch of synthetic utterances,
everything benchmarks/ctc.cpp:150-165 does per utterance: build the CTC target
graph, wrap the [T, C] emissions as a linear graph, intersect, two forwardScores,
subtract, backward (emission gradients populated).  Emissions are resident in HBM
when the timed region starts (the PyTorch use-case); inputs follow the reference
generator (uniform [-5, 5) emissions, uniform targets in [1, C-1], blank 0),
seeded.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

N > 1 is launched by the driver under torch.distributed.run, one rank per GPU;
utterances are independent, so each rank owns B utterances (weak scaling) and the
only collective is an all_gather of the B scalar losses over RCCL.

A plain run sets up, warms up, times the K steps and prints ONE JSON line: metric,
value (losses/s), unit, higher_is_better, dtype, ms_per_step (one timed step).
--dump-outputs DIR writes what the timed path computed in its last step (the losses and
a fixed, seeded sample of the emission gradients) as DIR/<name>.npy.
--full adds every side record to the line and to bench_out/last_full.json, among them
  roofline     -- forwardScore kernel: algorithmic bytes (8A + 8N per graph) /
                  hipEvent-timed launch duration vs the 8 TB/s HBM3E peak
  cpu_baseline -- the unmodified reference's parallelMap CTC pattern on all host
                  cores (oracle/_ref) on a bounded sample of the same workload
and the cold pass, the built-lattice step, the reference's API forms and programs,
BASELINE's other configurations and the in-run parity check against the reference.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.environ.get("GTN_BENCH_OUT") or os.path.join(ROOT, "bench_out")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)


LINE_LIMIT = 4096  # bytes of the final stdout line (the driver keeps a bounded tail of stdout)


def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d}


def _sig(x, n=6):
    """floats to n significant digits (the full record keeps every digit)"""
    if isinstance(x, float):
        return float("%.*g" % (n, x))
    if isinstance(x, dict):
        return {k: _sig(v, n) for k, v in x.items()}
    if isinstance(x, list):
        return [_sig(v, n) for v in x]
    return x


def compact_line(full, full_ref=None):
    """The ONE line the driver parses: the contract's keys, `roofline`, `cpu_baseline` and the in-run parity verdict,
    under LINE_LIMIT bytes.  Everything else of `full` (side configurations, API forms, per-rank reports, the
    built-lattice step) lives in the side file named by `full_record`."""
    line = _pick(full, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "priming_steps", "ms_per_step",
                        "ms_per_step_cold", "value_cold", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
                        "dry_run", "gather_ok"))
    line["config"] = _pick(full.get("config") or {}, ("workload", "global_batch", "composed_nodes", "composed_arcs",
                                                       "parallelism", "rccl_ranks", "value_reference_api", "host"))
    roof_keys = ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "ms_per_launch",
                 "algorithmic_bytes_per_launch")
    if full.get("roofline"):
        line["roofline"] = _pick(full["roofline"], roof_keys)
    if full.get("roofline_other"):
        line["roofline_other"] = {k: _pick(v, ("kernel", "frac", "ms_per_launch", "traffic"))
                                  for k, v in full["roofline_other"].items()}
    if full.get("cpu_baseline"):
        cb = _pick(full["cpu_baseline"], ("value", "unit", "cores", "kind", "sample"))
        if isinstance(cb.get("sample"), str) and len(cb["sample"]) > 240:
            cb["sample"] = cb["sample"][:237] + "..."
        line["cpu_baseline"] = cb
    if full.get("parity_in_run"):
        line["parity_in_run"] = _pick(full["parity_in_run"], ("ok", "n", "loss_max_rel", "loss_max_rel_vs_fp64",
                                                             "grad_max_abs_vs_fp64", "grad_max_abs_vs_reference",
                                                             "reference_grad_max_abs_vs_fp64",
                                                             "grad_elements_no_further_from_fp64_than_reference", "error"))
    if full.get("collectives"):
        line["collectives"] = full["collectives"][:160]
    if full.get("per_rank") and len(full["per_rank"]) > 1:
        line["rank_seconds"] = [r.get("seconds") for r in full["per_rank"]]
    if full_ref:
        line["full_record"] = full_ref
    line = _sig(line)
    text = json.dumps(line, separators=(",", ":"))
    # (never over the limit: shed the optional parts, largest first)
    for k in ("roofline_other", "rank_seconds", "collectives", "full_record"):
        if len(text) <= LINE_LIMIT:
            break
        line.pop(k, None)
        text = json.dumps(line, separators=(",", ":"))
    return text


def emit(full):
    """write the full record beside the script (bench_out/last_full.json; also under $GRAFT_REPO_ROOT/gpurun_out when
    that exists, so a gpurun call brings it home); returns the compact line for say_last()"""
    import hashlib
    text = json.dumps(full) + "\n"  # (sha256 and bytes below are those of the FILE: `sha256sum bench_out/last_full.json`)
    ref = None
    for d in (OUT_DIR, os.path.join(ROOT, "gpurun_out")):
        try:
            if d.endswith("gpurun_out") and (not os.path.isdir(d) or os.environ.get("GTN_BENCH_OUT")):
                continue  # (a child process with its own output directory does not touch the parent's copy)
            os.makedirs(d, exist_ok=True)
            with open(os.path.join(d, "last_full.json"), "w") as f:
                f.write(text)
            if ref is None:
                ref = {"path": os.path.relpath(os.path.join(d, "last_full.json"), ROOT), "sha256": hashlib.sha256(text.encode()).hexdigest(), "bytes": len(text)}
        except OSError:
            continue
    return compact_line(full, ref)


def flush_c_stdio():
    """RCCL prints its version banner with printf: into a pipe that is a BUFFERED write which would otherwise surface
    when the process exits, i.e. after the result line.  fflush(NULL) sends it on its way now."""
    try:
        C.CDLL(None).fflush(None)
    except Exception:
        pass


def say_last(text, world=1, rc=0):
    """The compact line as the LAST thing on stdout.  The caller has left the process group; whatever the C
    libraries still hold in their stdio buffers goes out first (RCCL's banner would otherwise surface when the
    process exits, after the line), and the other ranks -- which print nothing -- get a moment to finish.  The
    process then ends the ordinary way: a profiler attached to it (rocprofv3) writes its files at exit."""
    flush_c_stdio()
    if world > 1:
        time.sleep(1.0)
    sys.stdout.flush()
    sys.stderr.flush()
    print(text)
    sys.stdout.flush()
    if rc:
        sys.exit(rc)


def leave_quietly():
    """ranks that print no line: nothing of theirs may land after rank 0's"""
    flush_c_stdio()
    sys.stdout.flush()
    sys.stderr.flush()


def ctc_arrays(target, blank=0):
    """arc/node arrays of benchmarks/ctc.cpp:40-58's ctcGraph, vectorised"""
    U = len(target)
    L = 2 * U + 1
    l = np.arange(L)
    idx = (l - 1) // 2
    label = np.where(l % 2 == 1, target[np.clip(idx, 0, U - 1)], blank).astype(np.int32)
    prev = target[np.clip(idx - 1, 0, U - 1)]
    has_step = l > 0
    has_skip = (l % 2 == 1) & (l > 1) & (label != prev)
    n_arcs = 1 + has_step.astype(np.int64) + has_skip.astype(np.int64)
    off = np.concatenate([[0], np.cumsum(n_arcs)])
    A = int(off[-1])
    src = np.empty(A, np.int32)
    dst = np.empty(A, np.int32)
    lab = np.empty(A, np.int32)
    src[off[:-1]] = l
    dst[off[:-1]] = l
    lab[off[:-1]] = label
    s = off[:-1][has_step] + 1
    src[s] = l[has_step] - 1
    dst[s] = l[has_step]
    lab[s] = label[has_step]
    k = off[:-1][has_skip] + 2
    src[k] = l[has_skip] - 2
    dst[k] = l[has_skip]
    lab[k] = label[has_skip]
    start = (l == 0).astype(np.uint8)
    accept = ((l == L - 1) | (l == L - 2)).astype(np.uint8)
    return start, accept, src, dst, lab


def build_ctc_graphs(gtn, targets):
    out = []
    for t in targets:
        st, ac, s, d, lab = ctc_arrays(t)
        g = gtn.Graph()
        g.add_nodes(st, ac)
        g.add_arcs(s, d, lab)
        g.arc_sort()
        out.append(g)
    return out


def cpu_baseline(B, T, Cn, U, seed, budget_s=45.0):
    """reference CPU path timed on this host (rank 0, N=1 only), bounded sample"""
    import graphgen as gg
    cores = os.cpu_count() or 1
    path = os.path.join(ROOT, "oracle", "_ref", "libgtn_ref.so")
    if os.path.exists(path):
        lib = C.CDLL(path)
        lib.ref_ctc_batch.restype = C.c_double
        lib.ref_ctc_batch.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p, C.c_void_p]
        # batch >= 4 x cores so every thread has work, 3 timed iterations
        # (ref_ctc_batch returns the mean seconds per iteration); bounded to about 30 s of CPU work
        nb = int(max(cores * 4, 8))
        scale = (T * Cn * U) / (1000.0 * 256 * 100)
        if scale > 1.5:
            nb = int(max(cores, 8))
        em, tg = gg.ctc_inputs(seed, nb, T, Cn, U)
        losses = np.zeros(nb, np.float32)
        thr = C.c_int()
        t0 = time.time()
        secs = []
        while len(secs) < 3 and (not secs or time.time() - t0 + secs[-1] < budget_s):
            secs.append(lib.ref_ctc_batch(em.ctypes.data, tg.ctypes.data, nb, T, Cn, U, 0, 1, losses.ctypes.data, None,
                                          C.byref(thr)))
        iters = len(secs)
        sec = float(np.mean(secs))
        return {"value": nb / sec, "unit": "losses/s", "cores": int(thr.value), "kind": "reference",
                "sample": f"mean of {iters} timed iteration(s) of parallelMap(fwd)+parallelMap(bwd) "
                          f"over {nb} utterances (T={T}, C={Cn}, U={U}); per-iteration losses/s min "
                          f"{nb / max(secs):.1f} max {nb / min(secs):.1f}; {time.time() - t0:.1f}s wall; host has "
                          f"{cores} logical cores"}
    from oracle_lib import ctc_loss
    em, tg = gg.ctc_inputs(seed, 4, T, Cn, U)
    t0 = time.time()
    for b in range(4):
        ctc_loss(em[b], tg[b])
    sec = time.time() - t0
    return {"value": 4 / sec, "unit": "losses/s", "cores": 1, "kind": "port",
            "sample": f"4 utterances (T={T}, C={Cn}, U={U}) through the scalar C oracle"}


def parity_in_run(em, tg, losses, grads, T, Cn, U, n):
    """The first `n` utterances of the TIMED batch through the checker in this same process: the unmodified reference
    (oracle/_ref/libgtn_ref.so: ref_ctc_batch = parallelMap(fwd) + parallelMap(bwd), benchmarks/ctc.cpp:136-168) when it
    was built, else the C restatement (oracle/liboracle.so).  `losses` [B] and `grads` [B][T][C] (or None) are what the
    timed loop's last step left on the device."""
    n = int(min(n, len(tg)))
    path = os.path.join(ROOT, "oracle", "_ref", "libgtn_ref.so")
    want_l = np.zeros(n, np.float32)
    want_g = np.zeros((n, T, Cn), np.float32)
    e = np.ascontiguousarray(em[:n])
    t = np.ascontiguousarray(tg[:n])
    if os.path.exists(path):
        lib = C.CDLL(path)
        lib.ref_ctc_batch.restype = C.c_double
        lib.ref_ctc_batch.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p, C.c_void_p]
        thr = C.c_int()
        lib.ref_ctc_batch(e.ctypes.data, t.ctypes.data, n, T, Cn, U, 0, 1, want_l.ctypes.data, want_g.ctypes.data, C.byref(thr))
        checker = "reference (oracle/_ref/libgtn_ref.so: the unmodified gtn library compiled from /root/reference)"
    else:
        from oracle_lib import ctc_loss
        for b in range(n):
            want_l[b], g = ctc_loss(e[b], t[b])
            want_g[b] = g.reshape(T, Cn)
        checker = "port (oracle/liboracle.so: C restatement pinned to the reference, tests/test_oracle.py)"
    # third corner: the same loss and gradient in float64 (tests/ctc_fp64.py: the alpha-beta recursion of
    # shortest.cpp:86-170 / :33-62 over the product of compose.cpp:377-522 in numpy float64).  The float32 reference
    # keeps unnormalised scores of magnitude ~8.5 T, so ITS gradients carry ~8 eps |z| of rounding (1.4e-3 at
    # T = 1000); the gate is therefore the north star's 1e-4 against exact arithmetic, and "no further from exact
    # arithmetic than the reference itself is" per utterance -- both distances measured here, not assumed.
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from ctc_fp64 import ctc_loss_fp64
    got_l = np.asarray(losses[:n], np.float64)
    l64 = np.zeros(n)
    d_gpu = np.zeros(n)
    d_ref = np.zeros(n)
    d_gpu_ref = np.zeros(n)
    closer = 0.0
    for b in range(n):
        l64[b], g64, _ = ctc_loss_fp64(e[b], t[b])
        d_ref[b] = np.abs(want_g[b] - g64).max()
        if grads is not None:
            gb = np.asarray(grads[b], np.float64)
            d_gpu[b] = np.abs(gb - g64).max()
            d_gpu_ref[b] = np.abs(gb - want_g[b]).max()
            closer += float(np.mean(np.abs(gb - g64) <= np.abs(want_g[b] - g64)))
    out = {"n": n, "checker": checker,
           "loss_max_rel": float(np.max(np.abs(got_l - want_l) / np.maximum(np.abs(want_l), 1e-30))),
           "loss_max_rel_vs_fp64": float(np.max(np.abs(got_l - l64) / np.maximum(np.abs(l64), 1e-30))),
           "reference_loss_max_rel_vs_fp64": float(np.max(np.abs(want_l - l64) / np.maximum(np.abs(l64), 1e-30))),
           "tolerance": "GATED: losses <= 1e-4 relative against the reference AND against float64 (north_star); emission "
                        "gradients (posteriors in [-1, 1]): max |gpu - float64| <= 1e-4 (tests/ctc_fp64.py) AND max |gpu - "
                        "reference| <= 1e-2 (the float32 reference keeps unnormalised scores ~8.5 T and is itself ~1e-3 from "
                        "float64 at T = 1000: reference_grad_max_abs_vs_fp64).  REPORTED, not gated: the share of gradient "
                        "elements at which the gpu is no further from float64 than the reference is"}
    if grads is not None:
        out["grad_max_abs_vs_fp64"] = float(d_gpu.max())
        out["reference_grad_max_abs_vs_fp64"] = float(d_ref.max())
        out["grad_max_abs_vs_reference"] = float(d_gpu_ref.max())
        out["grad_elements_no_further_from_fp64_than_reference"] = closer / n
        out["utterances_no_further_from_fp64_than_reference"] = float(np.mean(d_gpu <= d_ref + 1e-6))
    out["ok"] = bool(out["loss_max_rel"] <= 1e-4 and out["loss_max_rel_vs_fp64"] <= 1e-4
                     and (grads is None or (d_gpu.max() <= 1e-4 and d_gpu_ref.max() <= 1e-2)))
    return out


def unmodified_caller(B):
    """The reference's own benchmark program, benchmarks/ctc.cpp:136-168, compiled UNMODIFIED against
    include/gtn and linked to libgtn_amd.so (oracle/dropin.mk): per-utterance graph functions called
    from parallelMap threads, which the engine gathers into batched launches (gtnx_parallel_enter).  Its
    own configuration (T=1000, U=100, alphabet 28), its own timing loop (5 + 100 iterations)."""
    import re
    import subprocess
    exe = os.path.join(ROOT, "oracle", "_ref", "dropin", "bm_ctc")
    if not os.path.exists(exe):
        return None
    try:
        r = subprocess.run([exe, str(B)], capture_output=True, text=True, timeout=240)
        times = {k: float(v) for k, v in re.findall(r"Timing (\w+) \.\.\.\s+([0-9.e+-]+) msec", r.stdout)}
        if "ctcBatched" not in times:
            return {"error": (r.stdout + r.stderr)[-300:]}
        out = {"program": "benchmarks/ctc.cpp (reference, unmodified) with batch size %d: T=1000, U=100, alphabet 28" % B,
               "ctcBatched_ms": times["ctcBatched"], "losses_per_s": B / (times["ctcBatched"] * 1e-3),
               "other_timings_ms": {k: v for k, v in times.items() if k != "ctcBatched"},
               "other_timings_note": "the program's own timers around calls on an asynchronous device: ctcBatched, ctcGrad and the "
                                     "ngram entries end in a value the host reads or in compose (which returns sizes); ctcLoss "
                                     "never looks at its result, so its figure is launch time only -- configs.C1 is the "
                                     "single-utterance latency with the loss read back",
               "reference_one_core_ms": {"ctcLoss": 94.4, "ngramCtcLoss": 4.1, "ngramCtcGrad": 0.41,
                                         "source": "BASELINE.md (measured in the build container, other hardware)"}}
        # benchmarks/functions.cpp, unmodified too: compose of two explicit graphs (100 x 20 arcs against
        # 50 x (500 + 500 self loops)), unsorted and sorted -- the reference on one core: 98.6 / 6.6 ms
        fexe = os.path.join(ROOT, "oracle", "_ref", "dropin", "bm_functions")
        if os.path.exists(fexe):
            rf = subprocess.run([fexe], capture_output=True, text=True, timeout=240)
            ft = {k: float(v) for k, v in re.findall(r"Timing (\w+) \.\.\.\s+([0-9.e+-]+) msec", rf.stdout)}
            # (only the compose entries: compose returns with its sizes, i.e. after the kernels; the program's
            # forwardScore loops never look at a result, so on an asynchronous device its timer sees launches only)
            out["functions_benchmark_ms"] = {k: ft[k] for k in ("composeForward", "composeForwardSorted") if k in ft}
            out["functions_benchmark_ms"]["reference_one_core"] = {"composeForward": 98.6, "composeForwardSorted": 6.6}
        return out
    except Exception as e:  # a diagnostic must not cost the bench line
        return {"error": str(e)[:300]}


def run_json(cmd, timeout, cpus=None, env=None):
    """one JSON line from a child process (the last line that parses); cpus: the child's CPU affinity"""
    import subprocess
    try:
        pre = (lambda: os.sched_setaffinity(0, cpus)) if cpus else None
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=ROOT, preexec_fn=pre,
                           env=dict(os.environ, **env) if env else None)
        for ln in reversed(r.stdout.strip().splitlines()):
            try:
                return json.loads(ln)
            except ValueError:
                continue
        return {"error": (r.stdout + r.stderr)[-400:]}
    except Exception as e:  # a sub-record must not cost the bench line
        return {"error": str(e)[:300]}


def reference_loop(B, Cn, mode):
    """tests/native/bm_ctc_c256.cpp: timeBatchedCtc of benchmarks/ctc.cpp:136-168 written with the reference's
    names only (ctcGraph via addNode / addArc / arcSort, linearGraph + setWeights per utterance, parallelMap(fwd)
    then parallelMap(bwd)) at this alphabet size; emissions in device memory (`device`) or host vectors (`host`)."""
    exe = os.path.join(ROOT, "tests", "dropin", "_bin", "bm_ctc_c256")
    if not os.path.exists(exe):
        return None
    # The program runs on the cores of the GPU's own NUMA node (what `numactl --cpunodebind` does for a one-GPU job on
    # a two-socket host): its 33 host threads build 512 graphs per step, and threads that wander to the other socket
    # cost 5 % and a spread of +-6 % (0.94-1.03 ms per batch unbound, 0.91-0.93 bound, same box).
    cpus, node = gpu_local_cpus(0)
    r = run_json([exe, str(B), str(Cn), "300", mode], 300, cpus)
    if isinstance(r, dict) and "error" not in r:
        r["placement"] = ("the %d logical CPUs of the GPU's NUMA node (%s)" % (len(cpus), node)) if cpus else "unbound"
    return r


def other_configs(args):
    """BASELINE.json configs[0], [1], [3], [4] (C3 is the line itself): short timed loops, each with its own roofline
    and cpu_baseline, run as child processes so that their memory is gone before the next one starts"""
    py = sys.executable
    out = {}
    # (host-bound children run on the cores of the GPU's NUMA node, like reference_loop(); the CPU baselines inside
    #  them use every core they are given -- `cores` in each cpu_baseline says how many)
    cpus, _ = gpu_local_cpus(0)
    out["C1"] = run_json([py, os.path.join(ROOT, "tools", "bench_configs.py"), "c1"], 300, cpus)
    out["C2"] = run_json([py, os.path.join(ROOT, "tools", "bench_configs.py"), "c2"], 300)
    out["C3_viterbi"] = run_json([py, os.path.join(ROOT, "tools", "bench_configs.py"), "c3v"], 600)
    out["C4"] = run_json([py, os.path.join(ROOT, "tools", "bench_c4.py"), "--steps", "4"], 600)
    c5 = run_json([py, os.path.join(ROOT, "bench.py"), "--full", "--config", "c5", "--steps", "10", "--warmup", "2", "--no-configs",
                   "--no-reference-api", "--no-unmodified-caller", "--no-built-lattice", "--cpu-baseline-seconds", "20"], 600,
                  env={"GTN_BENCH_OUT": os.path.join(OUT_DIR, "c5")})
    try:  # (the child's stdout line is the compact one; its full record is in its own side file)
        if "error" not in c5:
            c5 = json.load(open(os.path.join(OUT_DIR, "c5", "last_full.json")))
    except Exception as e:
        c5 = {"error": "C5 child: no full record (%s)" % str(e)[:200]}
    if "error" not in c5:
        c5 = {k: c5.get(k) for k in ("metric", "value", "unit", "ms_per_step", "config", "roofline", "roofline_other",
                                     "kernel_ms_per_step", "host_ms_last_step", "loss_mean", "cpu_baseline", "parity_in_run")}
        c5["note"] = ("one rank's shard of BASELINE config C5 (T=2000, C=1024, U=200, 4096 utterances over 8 GPUs = 512 "
                      "per GPU), timed on one MI355X")
    out["C5_shard"] = c5
    return out


def gpu_local_cpus(local_rank):
    """(logical CPUs of the NUMA node GPU `local_rank` hangs off, that node's number) from sysfs; (None, None) if unknown"""
    import glob
    bases = []
    try:
        import torch
        props = torch.cuda.get_device_properties(local_rank)
        bdf = getattr(props, "pci_bus_id", None)
        if isinstance(bdf, str) and bdf:
            bases.append("/sys/bus/pci/devices/" + bdf.lower())
        elif isinstance(bdf, int):  # (this torch: three integers)
            bases.append("/sys/bus/pci/devices/%04x:%02x:%02x.0" % (int(getattr(props, "pci_domain_id", 0)), bdf,
                                                                      int(getattr(props, "pci_device_id", 0))))
    except Exception:
        pass
    # (no bus id from torch, or a sysfs layout that does not list it: the DRM render devices in order)
    cards = sorted(os.path.dirname(p) for p in glob.glob("/sys/class/drm/card[0-9]*/device/local_cpulist"))
    if local_rank < len(cards):
        bases.append(cards[local_rank])
    for base in bases:
        try:
            cpus = set()
            for part in open(base + "/local_cpulist").read().strip().split(","):
                lo, _, hi = part.partition("-")
                cpus.update(range(int(lo), int(hi or lo) + 1))
            cpus &= os.sched_getaffinity(0)
            if not cpus:
                continue
            try:
                node = int(open(base + "/numa_node").read())
            except Exception:
                node = None
            return cpus, node
        except Exception:
            continue
    return None, None


def pin_to_gpu_numa_node(local_rank):
    """One process per GPU: keep this rank's host threads (the engine's worker pool inherits the mask)
    on the cores of the NUMA node its GPU hangs off.  Returns what it did, for the per-rank report."""
    cpus, node = gpu_local_cpus(local_rank)
    if not cpus:
        return None
    try:
        os.sched_setaffinity(0, cpus)
        return {"numa_node": node, "cpus": len(cpus)}
    except Exception:
        return None


def per_rank_report(dist, torch, world, dev, host_ms, dt):
    """every rank's host phases, wall time and host-thread budget, gathered on rank 0: what makes a
    scaling run diagnosable (a slow rank, a starved host)"""
    mine = [float(dt)] + [float(host_ms.get(k, 0.0)) for k in ("target_graphs", "emission_graphs", "intersect",
                                                                   "forward_scores", "backward")] + \
           [float(len(os.sched_getaffinity(0)))]
    t = torch.tensor(mine, dtype=torch.float64, device=dev)
    if world > 1 or (dist.is_initialized() and os.environ.get("GTN_AMD_FORCE_COLLECTIVES") == "1"):
        parts = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(parts, t)
    else:
        parts = [t]
    out = []
    for r, p in enumerate(parts):
        v = p.cpu().tolist()
        out.append({"rank": r, "seconds": v[0], "host_ms_last_step": {"target_graphs": v[1], "emission_graphs": v[2],
                    "intersect": v[3], "forward_scores": v[4], "backward": v[5]}, "host_threads": int(v[6])})
    return out


class LossGather:
    """The step's one collective -- all_gather of every rank's losses -- kept OFF the step's critical path: the gather of
    step s is enqueued asynchronously behind the step's kernels (torch's process group runs it on its own stream) and
    is waited for when step s + 1 has been enqueued, so it overlaps the next step's sweeps and the ranks are coupled one
    step apart instead of at every step.  Two loss / result buffers alternate.  (The synchronous form put the
    collective's latency -- and the slowest rank's jitter -- into every step of every rank.)"""

    def __init__(self, dist, torch, world, B, dev, active):
        self.dist, self.active = dist, active
        self.loss = [torch.empty(B, dtype=torch.float32, device=dev) for _ in range(2 if active else 1)]
        self.out = [torch.empty(world * B, dtype=torch.float32, device=dev) for _ in range(2)] if active else None
        self.work, self.i, self.last = None, 0, 0

    def buffer(self):  # where the step about to run writes its losses
        return self.loss[self.i]

    def post(self):  # the step has been enqueued: start its gather, wait (on the stream) for the one before
        self.last = self.i
        if not self.active:
            return
        if self.work is not None:
            self.work.wait()
        self.work = self.dist.all_gather_into_tensor(self.out[self.i], self.loss[self.i], async_op=True)
        self.i ^= 1

    def drain(self):
        if self.work is not None:
            self.work.wait()
            self.work = None

    def last_losses(self):
        return self.loss[self.last]

    def last_gathered(self):
        return self.out[self.last] if self.active else None


def dry_run(args, dist, torch, world, rank, dev):
    """--dry-run-cpu: the collective / timing skeleton of main() over gloo, with a stand-in for the step
    (losses = rank-tagged constants).  Nothing is measured; the line says so."""
    from gtn_amd.distributed import max_over_ranks
    B = args.batch
    lg = LossGather(dist, torch, world, B, dev, world > 1)

    def step():
        lg.buffer().fill_(float(rank))
        lg.post()

    def fence():
        lg.drain()
        if world > 1:
            dist.barrier()

    for _ in range(args.warmup):
        step()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    dt_local = time.perf_counter() - t0
    dt = max_over_ranks(dt_local, dev)
    ranks = per_rank_report(dist, torch, world, dev, {}, dt_local)
    line = None
    if rank == 0:
        gathered = lg.last_gathered()
        ok = gathered is None or all(float(gathered[r * B]) == float(r) for r in range(world))
        line = emit({"metric": "CTC forward+backward losses/sec (T=%d, C=%d)" % (args.T, args.C), "value": None,
                          "unit": "losses/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": dt / max(args.steps, 1) * 1e3, "higher_is_better": True, "scaling": "weak",
                          "dry_run": True, "data": "none (stand-in step: collectives and timing skeleton only)",
                          "config": {"workload": "dry run (no kernel)", "global_batch": world * B,
                                     "parallelism": f"dp{world} (utterance sharding, all_gather of losses)",
                                     "rccl_ranks": world if world > 1 else 0, "value_reference_api": None},
                          "gather_ok": bool(ok), "per_rank": ranks})
    if world > 1:
        dist.destroy_process_group()
    if line is not None:
        say_last(line, world)
    elif world > 1:
        leave_quietly()


def headline(args, world, world_dist, forced, native, B, T, Cn, U, dt, priming_steps):
    """the record of the timed loop: what a plain run prints, and what --full adds its side records to"""
    return {
        "metric": "CTC forward+backward losses/sec (T=1000, C=256)" if (T, Cn) == (1000, 256)
        else f"CTC forward+backward losses/sec (T={T}, C={Cn})",
        "value": world * B * args.steps / dt,
        "unit": "losses/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup, "priming_steps": priming_steps,
        "ms_per_step": dt / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": {"workload": f"{'BASELINE config C3' if (B, T, Cn, U) == (512, 1000, 256, 100) else 'CTC'}: compose(ctc_target, emissions)+forwardScore CTC loss "
                               f"fwd+bwd, T={T}, C={Cn}, U={U}, batch={B} per GPU",
                   "global_batch": world * B,
                   "parallelism": f"dp{world} (utterance sharding, all_gather of losses)",
                   # (in `config` so that the driver's parsed record keeps it:) ranks in the RCCL process group
                   # of THIS run (0: no process group)
                   "rccl_ranks": world if world_dist else 0,
                   "host": "python (gtn_amd/api.py)" if native is None else "C++ (include/gtn/, bench_native/ctc_step.cpp)"},
        "collectives": ("RCCL (nccl backend): all_gather of the losses per step (asynchronous, overlapping the next step), "
                        "barrier + all_reduce(MAX) around the timed region" + (" -- forced at world size 1 (GTN_BENCH_FORCE_DIST=1)" if forced and world == 1 else ""))
        if world_dist else None,
    }


DUMP_GRAD_FLOATS = 8 << 20  # emission-gradient elements --dump-outputs writes at most (32 MB of float32)


def dump_outputs(d, lg, grad_dev, keep, stream, B, T, Cn):
    """--dump-outputs: what the timed path computed in its last step, as float32 .npy files in `d` -- the losses a
    caller receives (this rank's; every rank's too when the step gathers them) and the emission gradients of a fixed,
    seeded choice of utterances (all of them when they fit in DUMP_GRAD_FLOATS), in utterance order.  The inputs are
    seeded (graphgen.ctc_inputs): the same arguments give the same inputs on every run."""
    import torch
    os.makedirs(d, exist_ok=True)
    k = max(1, min(B, DUMP_GRAD_FLOATS // max(T * Cn, 1)))
    pick = np.arange(B) if k == B else np.sort(np.random.default_rng(0).choice(B, k, replace=False))
    rows = max(1, min(T, DUMP_GRAD_FLOATS // (k * Cn)))  # (one utterance larger than the budget: its first frames)
    with torch.cuda.stream(stream):
        losses = lg.last_losses().cpu()
        gathered = lg.last_gathered()
        gathered = gathered.cpu() if gathered is not None else None
        if grad_dev is not None:  # the C++ host: the step's gradients land in this [B, T, C] tensor
            grads = grad_dev[torch.from_numpy(pick).to(grad_dev.device), :rows].cpu().numpy()
        else:  # the Python host: the step returned its emission graphs
            ems = keep[0]
            grads = np.stack([np.asarray(ems[int(b)].grad().weights_to_numpy(), np.float32).reshape(T, Cn)[:rows]
                              for b in pick])
    stream.synchronize()
    np.save(os.path.join(d, "losses.npy"), losses.numpy().astype(np.float32))
    if gathered is not None:
        np.save(os.path.join(d, "losses_all_ranks.npy"), gathered.numpy().astype(np.float32))
    np.save(os.path.join(d, "emission_grads.npy"), np.ascontiguousarray(grads, np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=512, help="utterances per GPU (C3: 512)")
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--C", type=int, default=256)
    ap.add_argument("--U", type=int, default=100)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--built-lattice", action="store_true", default=True,
                    help="(default) also run the step with every lattice built (compose -> forwardScore kernel -> fused "
                         "backward) and report its kernels as built_lattice_path")
    ap.add_argument("--no-built-lattice", dest="built_lattice", action="store_false")
    ap.add_argument("--no-configs", action="store_true",
                    help="skip the sub-records of BASELINE.json's other configurations (C1, C2, C4, C5 shard)")
    ap.add_argument("--no-reference-api", action="store_true",
                    help="skip timing the same step through the vector overloads and through the reference's own loop")
    ap.add_argument("--cpu-baseline-seconds", type=float, default=45.0, help="bound of the cpu_baseline leg")
    ap.add_argument("--dry-run-cpu", action="store_true",
                    help="no GPU: drive this script's multi-rank branch (rendezvous, all_gather of the losses, barrier, "
                         "max-over-ranks timing, per-rank report) over gloo with a stand-in step -- tests/test_distributed_cpu.py")
    ap.add_argument("--config", choices=["c3", "c5"], default=None,
                    help="BASELINE.json configs: c3 = T 1000, C 256, U 100 (default); c5 = T 2000, C 1024, U 200")
    ap.add_argument("--no-unmodified-caller", action="store_true",
                    help="skip timing the reference's own benchmarks/ctc.cpp (built unmodified against include/gtn)")
    ap.add_argument("--parity-n", type=int, default=0,
                    help="utterances of the timed batch checked against the reference in this run (default 64; 16 at C5)")
    ap.add_argument("--python-host", action="store_true",
                    help="drive the step through the Python interface instead of the C++ one")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path computed in its last step: losses.npy "
                         "(float32 [B]; losses_all_ranks.npy [N*B] when N > 1) and emission_grads.npy (float32, a fixed "
                         "seeded sample of the utterances' [T, C] gradients, at most 32 MB)")
    ap.add_argument("--full", action="store_true",
                    help="also every side record (cold pass, per-kernel rooflines from a profiled pass, built-lattice "
                         "step, reference API forms and programs, BASELINE's other configurations, CPU baseline, in-run "
                         "parity against the reference) and the full record bench_out/last_full.json; the --no-* "
                         "options above select among them")
    args = ap.parse_args()
    if args.config == "c5":
        args.T, args.C, args.U = 2000, 1024, 200

    import torch
    import torch.distributed as dist
    import gtn_amd as gtn

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dry = args.dry_run_cpu
    # GTN_BENCH_FORCE_DIST=1: take the multi-rank branch (RCCL process group, all_gather of the losses, barrier,
    # max over ranks) with whatever world size the environment gives -- ONE on a single-GPU box, so that the
    # first 8-GPU run is not also the first time these calls execute (tests/test_distributed_gpu.py)
    forced = os.environ.get("GTN_BENCH_FORCE_DIST") == "1"
    if forced:
        os.environ["GTN_AMD_FORCE_COLLECTIVES"] = "1"
        os.environ.setdefault("MASTER_PORT", str(29500 + os.getpid() % 2000))
    world_dist = world > 1 or forced
    numa = pin_to_gpu_numa_node(local) if (world_dist and not dry) else None
    if world_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if dry:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            torch.cuda.set_device(local)
            gtn.set_device(local)
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
    elif not dry:
        torch.cuda.set_device(0)
    dev = torch.device("cpu") if dry else torch.device("cuda", local if world > 1 else 0)
    B, T, Cn, U = args.batch, args.T, args.C, args.U
    if dry:
        return dry_run(args, dist, torch, world, rank, dev)

    import graphgen as gg
    em, tg = gg.ctc_inputs(1234 + rank, B, T, Cn, U)
    stream = torch.cuda.Stream(device=dev)
    gtn.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        em_dev = torch.from_numpy(em).to(dev)
        # ONE flat [world * B] result tensor per gather: all_gather_into_tensor writes the ranks' blocks in place (the
        # list form of all_gather copies world tensors around the collective, host work on every step)
        lg = LossGather(dist, torch, world, B, dev, world_dist)

    native = None
    if not args.python_host:
        native = C.CDLL(os.path.join(ROOT, "bench_native", "libgtn_bench.so"))
        native.gtn_bench_ctc_step.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_void_p]
        native.gtn_bench_ctc_step.restype = C.c_int
        native.gtn_bench_ctc_step_vector.argtypes = native.gtn_bench_ctc_step.argtypes
        native.gtn_bench_ctc_step_vector.restype = C.c_int
        with torch.cuda.stream(stream):
            grad_dev = torch.empty(B, T, Cn, dtype=torch.float32, device=dev)

    def native_step():
        # the step as a gtn user's C++ host code (bench_native/ctc_step.cpp): target
        # graphs built with parallelMap on host threads, graph functions batched
        with torch.cuda.stream(stream):
            rc = native.gtn_bench_ctc_step(em_dev.data_ptr(), tg.ctypes.data, B, T, Cn, U, lg.buffer().data_ptr(),
                                           grad_dev.data_ptr())
            if rc != 0:
                native.gtn_bench_last_error.restype = C.c_char_p
                raise RuntimeError("native step failed: " + native.gtn_bench_last_error().decode())
            lg.post()
        return None

    def vector_step():
        # the same step through the vector overloads of the per-graph functions (bench_native: gtn_bench_ctc_step_vector)
        with torch.cuda.stream(stream):
            if native.gtn_bench_ctc_step_vector(em_dev.data_ptr(), tg.ctypes.data, B, T, Cn, U, loss_dev.data_ptr(),
                                                grad_dev.data_ptr()) != 0:
                native.gtn_bench_last_error.restype = C.c_char_p
                raise RuntimeError("vector step failed: " + native.gtn_bench_last_error().decode())

    def step():
        if native is not None:
            return native_step()
        with torch.cuda.stream(stream):
            ctcs = build_ctc_graphs(gtn, tg)
            ems = gtn.linear_graph_n(B, T, Cn, em_dev)
            comp = gtn.intersect(ctcs, ems)
            loss = gtn.subtract(gtn.forward_score(ems), gtn.forward_score(comp))  # Python: left to right
            gtn.backward(loss)
            gtn.items_to_device(loss, lg.buffer())
            lg.post()
        return ems, comp

    def fence():
        if world_dist:
            with torch.cuda.stream(stream):
                lg.drain()
            dist.barrier()
        torch.cuda.synchronize()

    # one-time priming, outside the W warm-up steps the contract asks for: the first few
    # steps grow the engine's device / pinned pools (hipMalloc, hipHostMalloc), load each
    # kernel's code object and start the host worker pool; nothing of it recurs
    for _ in range(3):
        step()
    fence()
    from gtn_amd.distributed import max_over_ranks
    dt_cold = None
    if args.full:
        # ---- COLD pass: W warm-up + K timed steps exactly as the flags ask, on a GPU that has been busy for a few
        # milliseconds only (its clocks are still on their way up): reported as ms_per_step_cold / value_cold
        for _ in range(args.warmup):
            step()
        fence()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        fence()
        dt_cold = max_over_ranks(time.perf_counter() - t0, dev)
    # ---- PRIMED pass (`value`): the GPU leaves its idle clocks some tens of milliseconds after work arrives; with
    # W = 5 and K = 20 the whole measurement is 17 ms long and would be taken on the way up (0.668 ms per step
    # against 0.630 over 300 steps).  PRIME_STEPS more untimed steps (about 0.2 s at C3; the same count on every
    # rank -- a step may hold a collective) come first, EXTRA to the W warm-up steps and reported as `priming_steps`.
    PRIME_STEPS = 300
    for i in range(PRIME_STEPS):
        step()
        if i % 16 == 15:
            fence()  # (bounds what is queued ahead of the device)
    priming_steps = PRIME_STEPS
    fence()
    flush_c_stdio()  # (RCCL's banner, printed at the first collective, leaves the stdio buffer now -- not at exit)
    for _ in range(args.warmup):
        step()
    fence()
    t0 = time.perf_counter()
    keep = None
    for _ in range(args.steps):
        keep = step()
    fence()
    dt = dt_local = time.perf_counter() - t0
    dt = max_over_ranks(dt, dev)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, lg, grad_dev if native is not None else None, keep, stream, B, T, Cn)
    if not args.full:
        # a plain run: the headline figure only -- no side records, no side file
        line = compact_line(headline(args, world, world_dist, forced, native, B, T, Cn, U, dt, priming_steps)) \
            if rank == 0 else None
        del keep
        gtn.set_stream(None)
        gtn.synchronize()
        gtn.empty_cache()
        if world_dist:
            dist.destroy_process_group()
        if line is not None:
            say_last(line, world)
        elif world_dist:
            leave_quietly()
        return

    host_ms = None
    if native is not None:
        try:  # host phases of the timed loop's last step (bench_native/ctc_step.cpp)
            buf = (C.c_double * 5)()
            native.gtn_bench_last_host_ms(buf)
            host_ms = dict(zip(("target_graphs", "emission_graphs", "intersect", "forward_scores", "backward"),
                               [round(float(x), 3) for x in buf]))
        except Exception:
            host_ms = None
    losses_timed = lg.last_losses().cpu().numpy().copy()  # of the timed loop's last step
    grad_timed = None
    if native is not None:
        try:
            with torch.cuda.stream(stream):
                grad_timed = grad_dev.clone()
            stream.synchronize()
        except Exception:
            grad_timed = None
    # ---- PROFILED pass: K more steps with the engine's hipEvent pairs around each kernel family, for the per-kernel
    # figures below (kernel_ms_per_step, roofline); the timed loop above runs without them
    gtn.prof_reset()
    gtn.prof_enable(True)
    for _ in range(args.steps):
        keep = step()
    fence()
    gtn.prof_enable(False)
    prof = {n: gtn.prof_get(n) for n in gtn.prof_names()}
    loss_dev = lg.last_losses()  # (what the side legs below write into and read from)
    # composed-lattice size of utterance 0 (one extra untimed intersect)
    e0 = gtn.linear_graph_n(1, T, Cn, em_dev)
    comp = gtn.intersect(build_ctc_graphs(gtn, tg[:1]), e0)
    ems = e0
    n_nodes, n_arcs = comp[0].num_nodes(), comp[0].num_arcs()

    # ---- roofline of every profiled kernel family of the timed loop, against HBM peak.
    # Algorithmic bytes per launch (DESIGN.md section 3 / SURVEY.md section 8d):
    #   band_forward_score            4TC + 4(T+1)NS per utterance (emissions in, alpha out; NS = N rounded up to 4)
    #   band_forward_score_grad       8TC + 4(T+1)NS + 4A          (emissions in, gradient out, alpha in, G's gradient)
    #   linear_forward / _grad        4TC  /  12TC                 (rows in; rows in + gradient read-modify-write)
    #   intersect                     24A + 8N: what the chain-product variant of compose_kernel writes -- dst, w, gi1, gi2
    #                                 in arc order, in_src and in_w in in-row order (six 4-byte arrays per arc; src, il,
    #                                 ol, in_list are derivable and left out: DESIGN.md section 2) + in_off, pair_of per
    #                                 node.  (Rounds 2-5 priced it at 20A + 8N, one array short: the WRITE_SIZE counter
    #                                 -- 6.13 GB per launch at B = 512 -- agrees with 24A + 8N = 6.27 GB, there is no
    #                                 write amplification.)
    #   forward_score                 8A + 8N (reported by the engine)
    #   forward_score_grad            20A + 12N + 4TC (in-rows, arc gradients, node rows, emission gradient)
    # measured = the engine's hipEvent pairs around each family on the launch stream.
    KERNEL_OF = {  # family -> kernel (template arguments depend on the shape: matched by prefix in the PMC table)
        "band_forward_score": "band_forward_kernel",
        "band_forward_score_grad": "band_backward_kernel",
        "lazy_pair_forward_score": "lazy_pair_forward_kernel",
        "lazy_pair_forward_score_grad": "lazy_pair_backward_kernel",
        "linear_forward": "linear_rows_kernel<false>",
        "linear_forward_grad": "linear_rows_kernel<true>",
        "forward_score": "sd_forward_narrow_kernel<true>",
        "forward_score_grad": "sd_backward_narrow_kernel<true>",
        "intersect": "compose_kernel<3, false, true, true, true, 256>",
    }
    import glob

    def newest_pmc(tag):
        files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_%s_pmc_hbm.json" % tag)))
        return (json.load(open(files[-1])), files[-1]) if files else ({}, None)

    # the committed counter passes per workload: the timed loop at C3, the built-lattice step at B = 512 (its
    # compose / forwardScore / fused-backward launches), the C5-shaped launches (tools/profile_round4.sh)
    if (B, T, Cn, U) == (512, 1000, 256, 100):
        pmc, pmc_file = newest_pmc("c3")
        pmc_built, pmc_built_file = newest_pmc("built")
    elif (B, T, Cn, U) == (512, 2000, 1024, 200):
        pmc, pmc_file = newest_pmc("c5")
        pmc_built, pmc_built_file = {}, None
    else:
        pmc, pmc_file, pmc_built, pmc_built_file = {}, None, {}, None

    def rooflines(pr, pmc=pmc, pmc_file=pmc_file):
        fixed = {"linear_forward": B * 4.0 * T * Cn, "linear_forward_grad": B * 12.0 * T * Cn,
                 "intersect": B * (24.0 * n_arcs + 8.0 * n_nodes),
                 "forward_score_grad": B * (20.0 * n_arcs + 12.0 * n_nodes + 4.0 * T * Cn)}
        out = {}
        for name, e in pr.items():
            if not e["launches"] or name not in KERNEL_OF:
                continue
            per = fixed.get(name, e["algorithmic_bytes"] / e["launches"])
            ms = e["total_ms"] / e["launches"]
            if per <= 0 or ms <= 0:
                continue
            k = next((v for kk, v in pmc.items() if kk.startswith(KERNEL_OF[name])), None)
            # HBM bytes per launch from the PMC passes of this same command (rocprofv3 --pmc FETCH_SIZE /
            # WRITE_SIZE, separate passes; newest profiles/r*_c3_pmc_hbm.json).  Calibrated on
            # linear_rows_kernel<false>, whose bytes are known exactly: FETCH_SIZE reads half the
            # fetched KiB on gfx950, WRITE_SIZE is exact (profiles/README.md)
            traffic = (2 * k["FETCH_SIZE"]["mean_per_launch"] + k["WRITE_SIZE"]["mean_per_launch"]) * 1024 if k else None
            # (NOT measured by this run: read from the committed PMC passes of the same command and kernel)
            src = ("profiles/" + os.path.basename(pmc_file) + " (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of "
                   "`python bench.py`, tools/profile_gpu.sh / tools/profile_round4.sh; 2*FETCH_SIZE + WRITE_SIZE KiB per launch)") if k else None
            gbs = per / (ms * 1e-3) / 1e9
            out[name] = {"bound": "hbm", "kernel": KERNEL_OF[name], "achieved": gbs, "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": src, "ms_per_launch": ms,
                         "algorithmic_bytes_per_launch": per}
        return out

    roofs = rooflines(prof)
    dominant = max(roofs, key=lambda k: roofs[k]["ms_per_launch"]) if roofs else None
    roof = roofs.get(dominant)

    # ---- the same step with every lattice BUILT (the path graphs that are not CTC-shaped take, and what
    # GTNX_LAZY_COMPOSE=0 selects; through the vector overloads -- a batch record's product is symbolic by
    # construction): untimed for `value`, profiled for its kernels (compose_kernel, the forwardScore kernel over the
    # built lattices, its fused backward)
    built = None
    if native is not None and args.built_lattice and not os.environ.get("GTNX_LAZY_COMPOSE"):
        os.environ["GTNX_LAZY_COMPOSE"] = "0"
        try:
            for _ in range(3):
                vector_step()
            fence()
            gtn.prof_reset()
            gtn.prof_enable(True)
            dt_built = None
            for _ in range(3):  # (the best of three timed loops of five steps; the profiler sees all fifteen)
                t1 = time.perf_counter()
                for _ in range(5):
                    vector_step()
                fence()
                d = (time.perf_counter() - t1) / 5
                dt_built = d if dt_built is None else min(dt_built, d)
            gtn.prof_enable(False)
            pb = {n: gtn.prof_get(n) for n in gtn.prof_names()}
            lb = loss_dev.cpu().numpy()
            try:
                with torch.cuda.stream(stream):
                    gdiff = float((grad_dev - grad_timed).abs().max().item())
            except Exception:  # a diagnostic must not cost the bench line
                gdiff = None
            built = {"ms_per_step": dt_built * 1e3, "losses_per_s": B / dt_built, "roofline": rooflines(pb, pmc_built or pmc, pmc_built_file or pmc_file),
                     "loss_mean": float(np.mean(lb)),
                     # the two paths on the same batch: largest relative difference of a per-utterance loss
                     "max_rel_diff_vs_timed_path": float(np.max(np.abs(lb - losses_timed) / np.maximum(np.abs(lb), 1e-30))),
                     # ... and largest absolute difference of an emission-gradient element (posteriors in [-1, 1])
                     "max_abs_grad_diff_vs_timed_path": gdiff}
        finally:
            os.environ.pop("GTNX_LAZY_COMPOSE", None)
    # ---- the SAME step through the reference's own API forms, same inputs, same device tensors (world == 1):
    #   batch_records    gtn::Batch (the timed loop above: `value`)
    #   vector_overloads gtn::batched::* on std::vector<Graph> (bench_native: gtn_bench_ctc_step_vector)
    #   reference_loop   parallelMap(fwd) + parallelMap(bwd) over per-utterance lambdas, reference names only
    #                    (tests/native/bm_ctc_c256.cpp; its per-graph calls are deferred to the join: region.cpp)
    reference_api = None
    if world == 1 and native is not None and not args.no_reference_api:
        reference_api = {"batch_records": {"losses_per_s": B * args.steps / dt, "ms_per_batch": dt / args.steps * 1e3,
                                           "host": "bench_native/ctc_step.cpp over gtn::Batch (include/gtn/batch.h)"}}
        try:
            vstep = vector_step
            for _ in range(3):
                vstep()
            fence()
            nv = max(5, min(args.steps, 30))
            dv = None
            for _ in range(3):  # (a side figure: the best of three timed loops -- one host hiccup is not the path's speed)
                t1 = time.perf_counter()
                for _ in range(nv):
                    vstep()
                fence()
                d = (time.perf_counter() - t1) / nv
                dv = d if dv is None else min(dv, d)
            lv = loss_dev.cpu().numpy()
            reference_api["vector_overloads"] = {
                "losses_per_s": B / dv, "ms_per_batch": dv * 1e3,
                "max_rel_diff_vs_batch_records": float(np.max(np.abs(lv - losses_timed) / np.maximum(np.abs(losses_timed), 1e-30))),
                "host": "bench_native/ctc_step.cpp: gtn_bench_ctc_step_vector (gtn::batched on vectors of graphs)"}
        except Exception as e:  # a diagnostic must not cost the bench line
            reference_api["vector_overloads"] = {"error": str(e)[:300]}
        reference_api["reference_loop"] = reference_loop(B, Cn, "device")
        reference_api["reference_loop_host_emissions"] = reference_loop(B, Cn, "host")
    ranks = per_rank_report(dist, torch, world, dev, host_ms or {}, dt_local)
    parity = None
    if rank == 0:
        # the timed batch against the checker, in this run: 64 utterances (16 at C5's size: 8 MB of emissions each)
        # through ref_ctc_batch on all host cores + the float64 restatement
        try:
            npar = args.parity_n or (64 if T * Cn <= 1000 * 256 else 16)
            gpar = grad_timed[:npar].cpu().numpy() if grad_timed is not None else None
            parity = parity_in_run(em, tg, losses_timed, gpar, T, Cn, U, npar)
        except Exception as e:  # reported, and fails the run below
            parity = {"error": str(e)[:300], "ok": False}
    if rank == 0:
        losses = losses_timed
        out = headline(args, world, world_dist, forced, native, B, T, Cn, U, dt, priming_steps)
        # the same K steps after the same W warm-up steps WITHOUT the priming steps in front (clocks rising)
        out["ms_per_step_cold"], out["value_cold"] = dt_cold / args.steps * 1e3, world * B * args.steps / dt_cold
        out["config"]["composed_nodes"], out["config"]["composed_arcs"] = n_nodes, n_arcs
        # the same step through the reference's own API (parallelMap over per-utterance lambdas,
        # tests/native/bm_ctc_c256.cpp) beside `value`
        out["config"]["value_reference_api"] = ((reference_api or {}).get("reference_loop") or {}).get("losses_per_s")
        out.update({
            "roofline": roof,
            # every other kernel family of the timed loop against the same 8 TB/s
            "roofline_other": {k: v for k, v in roofs.items() if k != dominant},
            # the step with the lattices built (compose -> forwardScore kernel -> fused backward)
            "built_lattice_path": built,
            # where a step's wall time goes on the host thread (ms, last timed step) next to the GPU work below:
            # with the sweep kernels the step is host-bound
            "host_ms_last_step": host_ms,
            "kernel_ms_per_step": {k: v["total_ms"] / args.steps for k, v in prof.items()},
            # one entry per rank: its own wall time, host phases and host-thread budget (NUMA-pinned when N > 1)
            "per_rank": ranks,
            "numa": numa,
            "loss_mean": float(np.mean(losses)),
            # the first utterances of the timed batch, losses and emission gradients, against the reference in this run
            "parity_in_run": parity,
        })
        if world == 1 and not args.no_unmodified_caller:
            out["unmodified_caller"] = unmodified_caller(B)
        if world == 1 and native is not None and not args.no_reference_api:
            out["reference_api"] = reference_api
            # the same step written with the REFERENCE'S OWN API (parallelMap over per-utterance lambdas calling the
            # per-graph functions: tests/native/bm_ctc_c256.cpp = benchmarks/ctc.cpp:136-168 at C = 256; one process,
            # same GPU, emissions in device memory; item() returns with the loss and the clock stops after a device
            # synchronisation) next to `value` (gtn::Batch, an API the reference does not have)
            rl = (reference_api or {}).get("reference_loop") or {}
            if "losses_per_s" in rl:
                out["value_reference_api"] = rl["losses_per_s"]
                out["ms_per_step_reference_api"] = rl.get("ctcBatched_ms")
        if world == 1 and not args.no_configs and (B, T, Cn, U) == (512, 1000, 256, 100):
            # the children (other processes on the same GPU) get the memory this process's pools still hold
            gtn.synchronize()
            gtn.empty_cache()
            torch.cuda.empty_cache()
            out["configs"] = other_configs(args)
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(B, T, Cn, U, 1234, args.cpu_baseline_seconds)
        line = emit(out)
    else:
        line = None
    # orderly teardown: drop every graph, return pooled memory, leave the process group -- and only then the line
    # (RCCL writes to stdout when a group is destroyed; the driver reads the LAST line)
    del keep, ems, comp, e0
    gtn.set_stream(None)
    gtn.synchronize()
    gtn.empty_cache()
    if world_dist:
        dist.destroy_process_group()
    if line is not None:
        bad = parity is not None and not parity.get("ok", False)
        if bad:
            print("bench.py: the timed batch does NOT match the checker: " + json.dumps(parity), file=sys.stderr)
        say_last(line, world, 3 if bad else 0)
    elif world_dist:
        leave_quietly()


if __name__ == "__main__":
    main()
