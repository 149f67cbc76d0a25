"""ASG prefix beam search with N-best output on the device at BASELINE config C4's shape (B = 512, T = 1000, C = 512),
beam_size 16, cutoff_top_n 16, nbest 4, beside the CTC prefix beam search with a bigram table on the same tensor, the
same table and the same parameters.

  asg     Batch.asg_beam_decode: two launches (asg_beam_rows_kernel, asg_beam_search_kernel), tokens / lengths / scores
          written into the caller's tensors, no copy back
  ctc_lm  Batch.ctc_beam_decode(lm=table, lm_weight=1, insertion_bonus=0, blank=0) in a process of its own: the
          yardstick -- the searches share their structure (top-K row stream, prefix list in LDS, trie in scratch, keys,
          bitonic sort), ASG keeps one score per prefix where CTC keeps two

There is no route for the ASG call on the previous commit, so no speed-up is claimed.

    python tools/bench_asg_beam.py [--out profiles/asg_beam_c4.json]
        three samples of each, alternating, every sample a process of its own that warms its shapes up and then times
        windows of at least half a second with a host clock around a closing synchronise
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_asg_beam.py --worker trace
        a few calls of both, for the mean times of the four kernels (a run of its own: no counters, no other tracing)
    python tools/bench_asg_beam.py --merge-stats DIR/.../kernel_stats.csv [--out ...]
        adds those means to the record: the rows kernels on their byte model (4 C in, 8 K + 4 out per row; K + 1 for
        CTC) at the stream rate, the search kernels per batch and per frame, ASG over CTC.

    python tools/bench_asg_beam.py --graph [--parent TREE] [--out profiles/asg_beam_graph_c4.json]
        the same tensor and table with a compiled LM graph fused in (Batch.asg_beam_decode(lm=gtn_amd.LmGraph(...));
        DESIGN section 31) beside the call without one: the table's own bigram spelled as a graph (a start state and a
        state per label, C + C * C arcs, every state dense) and the synthetic back-off trigram of
        tools/bench_ctc_beam.py --graph over this alphabet, at that tool's weight and bonus.  Three samples of each,
        alternating, every sample a process of its own.  With --parent, the call without a graph is also run from
        TREE -- a built tree of the commit to compare with -- alternating with this tree's, and the record gets both
        and the run-to-run spread.

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
B, T, C = 512, 1000, 512
BLANK, BEAM, TOPN, NBEST = 0, 16, 16, 4
WINDOW_S = 0.5


def inputs(torch):
    """log-softmax of seeded normals in which one label per stretch of 8 frames is lifted: runs, as a model emits them"""
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    em = torch.randn((B, T, C), generator=g, device="cuda", dtype=torch.float32) * 3.0
    lifted = torch.randint(0, C, (B, T // 8 + 1), generator=g, device="cuda").repeat_interleave(8, dim=1)[:, :T]
    em.scatter_add_(2, lifted.unsqueeze(2), torch.full((B, T, 1), 12.0, device="cuda"))
    return torch.log_softmax(em, dim=2).contiguous()


def table_of(torch):
    """a seeded table [C + C * C]: normal(0, 1)"""
    g = torch.Generator(device="cuda")
    g.manual_seed(4321)
    return torch.randn((C + C * C,), generator=g, device="cuda", dtype=torch.float32).contiguous()


def byte_model():
    """(ASG rows, ASG search, CTC rows): 4 C in and 8 K + 4 out per row; those back in, one gather per (prefix, member
    of the set), at most a trie node and a self-transition per prefix and frame, the output rows"""
    rows = float(B) * T * (4.0 * C + 8.0 * TOPN + 4.0)
    search = float(B) * (T * (8.0 * TOPN + 4.0 + 12.0 * BEAM + 4.0 * BEAM * TOPN) + NBEST * (4.0 * T + 8.0))
    ctc_rows = float(B) * T * (4.0 * C + 8.0 * (TOPN + 1) + 4.0)
    return rows, search, ctc_rows


def worker(kind):
    sys.path.insert(0, HERE)
    import torch
    import gtn_amd as gtn
    assert torch.cuda.is_available() and gtn.device_count() > 0, "bench_asg_beam needs a GPU"
    em = inputs(torch)
    table = table_of(torch)
    tokens = torch.empty((B, NBEST, T), dtype=torch.int32, device="cuda")
    lengths = torch.empty((B, NBEST), dtype=torch.int32, device="cuda")
    scores = torch.empty((B, NBEST), dtype=torch.float32, device="cuda")

    def asg_step():
        ems = gtn.Batch.linear(B, T, C, em, False, True)
        ems.asg_beam_decode(tokens, lengths, scores, None, table, BEAM, TOPN, NBEST)

    lmg = None
    if kind in ("asg_bigram", "asg_trigram"):
        # the graph generators of tools/bench_ctc_beam.py, over this tool's alphabet
        import numpy as np
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        import bench_ctc_beam as cb
        lmg = gtn.LmGraph(cb.bigram_graph(gtn, np, table.cpu().numpy(), C=C) if kind == "asg_bigram"
                          else cb.trigram_graph(gtn, np, C=C))
        # (a full bigram has a state per label and the start; the trigram a unigram state, C bigram states and more)
        states = lmg.info()["num_states"]
        assert states == 1 + C if kind == "asg_bigram" else states > 1 + C, states
        am_scores = torch.empty((B, NBEST), dtype=torch.float32, device="cuda")

    def asg_graph_step():
        ems = gtn.Batch.linear(B, T, C, em, False, True)
        ems.asg_beam_decode(tokens, lengths, scores, None, table, BEAM, TOPN, NBEST, lm=lmg, lm_weight=cb.LM_WEIGHT,
                            insertion_bonus=cb.LM_BONUS, am_scores_out=am_scores)

    def ctc_lm_step():
        ems = gtn.Batch.linear(B, T, C, em, False, True)
        ems.ctc_beam_decode(tokens, lengths, scores, None, BLANK, BEAM, TOPN, NBEST, lm=table, lm_weight=1.0,
                            insertion_bonus=0.0)

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
            asg_step()
            ctc_lm_step()
            sync()
        print(json.dumps({"trace": "done"}))
        return
    c0 = gtn.debug_asg_beam_stats()
    ms, n = timed({"asg": asg_step, "ctc_lm": ctc_lm_step, "asg_bigram": asg_graph_step,
                   "asg_trigram": asg_graph_step}[kind])
    sync()
    c1 = gtn.debug_asg_beam_stats()
    rec = {"kind": kind, "utterances": B, "ms_per_batch": ms, "iters": n, "asg_beam_utterances": c1[1] - c0[1],
           "mean_length": float(lengths.float().mean().item()), "mean_score": float(scores.mean().item()),
           "slots_with_a_hypothesis": int(torch.isfinite(scores).sum().item())}
    if lmg is not None:
        rec["graph"] = lmg.info()
        rec["mean_am_score"] = float(am_scores.mean().item())
        rec["lm_weight"], rec["insertion_bonus"] = cb.LM_WEIGHT, cb.LM_BONUS
    if kind == "asg":
        first = scores.clone()
        asg_step()
        sync()
        rec["second_run_has_the_same_bits"] = bool(torch.equal(first.view(torch.int32), scores.view(torch.int32)))
    print(json.dumps(rec))


def run_worker(kind, tree=None):
    """a sample in a process of its own; `tree`: run this tool's copy in that built tree instead (the commit to
    compare with)"""
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    script = os.path.abspath(__file__) if tree is None else os.path.join(os.path.abspath(tree), "tools",
                                                                         os.path.basename(__file__))
    out = subprocess.run([sys.executable, script, "--worker", kind], env=env,
                         stdout=subprocess.PIPE, timeout=500, check=True).stdout.decode()
    rec = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    print(f"[bench_asg_beam] {kind}{'' if tree is None else ' (parent tree)'}: {rec['ms_per_batch']:.3f} ms per batch "
          f"of {rec['utterances']}", file=sys.stderr, flush=True)
    return rec


def spread(v):
    return {"samples": v, "min": min(v), "max": max(v), "median": sorted(v)[len(v) // 2]}


# (the search kernel is a template since the graph instantiation; the trace worker launches the graph-less one only)
KERNELS = {"asg_beam_rows_kernel": ("asg_beam_rows_kernel",), "asg_beam_search_kernel": ("asg_beam_search_kernel",),
           "ctc_beam_rows_kernel": ("ctc_beam_rows_kernel",),
           "ctc_beam_search_kernel<true>": ("ctc_beam_search_kernel<true>", "ctc_beam_search_kernelILb1E")}


def main_graph(a):
    """the --graph record: end to end without a graph (from this tree and, with --parent, from that one), with the
    bigram graph and with the trigram graph"""
    kinds = ("asg", "asg_bigram", "asg_trigram")
    samples, last, parent = {k: [] for k in kinds}, {}, []
    for _ in range(3):
        if a.parent:
            parent.append(run_worker("asg", a.parent)["ms_per_batch"])
        for k in kinds:
            last[k] = run_worker(k)
            assert last[k]["asg_beam_utterances"] > 0, last[k]
            samples[k].append(last[k]["ms_per_batch"])
    med = {k: sorted(v)[1] for k, v in samples.items()}
    rec = {"shape": {"B": B, "T": T, "C": C, "beam_size": BEAM, "cutoff_top_n": TOPN, "nbest": NBEST,
                     "table": "normal(0, 1), seeded, C + C * C float32", "lm_weight": last["asg_bigram"]["lm_weight"],
                     "insertion_bonus": last["asg_bigram"]["insertion_bonus"]},
           "unit": "ms per batch, host clock around a closing synchronise, windows >= 0.5 s",
           "asg": dict(spread(samples["asg"]), what="Batch.asg_beam_decode without a graph, this tree", utterances=B,
                       mean_length=last["asg"]["mean_length"], mean_score=last["asg"]["mean_score"]),
           "asg_bigram": dict(spread(samples["asg_bigram"]), what="lm = the table's own bigram as an LmGraph",
                              utterances=B, graph=last["asg_bigram"]["graph"],
                              mean_length=last["asg_bigram"]["mean_length"]),
           "asg_trigram": dict(spread(samples["asg_trigram"]), what="lm = a synthetic back-off trigram LmGraph",
                               utterances=B, graph=last["asg_trigram"]["graph"],
                               mean_length=last["asg_trigram"]["mean_length"]),
           "asg_bigram_over_asg": med["asg_bigram"] / med["asg"],
           "asg_trigram_over_asg": med["asg_trigram"] / med["asg"],
           "walks_per_frame_at_most": BEAM * TOPN}
    if a.parent:
        both = samples["asg"] + parent
        rec["asg_parent"] = dict(spread(parent), what="Batch.asg_beam_decode, the parent commit's tree, alternating "
                                 "with this tree's samples", utterances=B)
        rec["run_to_run_spread_ms"] = max(max(parent) - min(parent), max(samples["asg"]) - min(samples["asg"]))
        rec["asg_median_minus_parent_median_ms"] = med["asg"] - sorted(parent)[1]
        rec["all_six_samples_range_ms"] = max(both) - min(both)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=["asg", "ctc_lm", "asg_bigram", "asg_trigram", "trace"])
    ap.add_argument("--merge-stats")
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--parent")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.worker:
        worker(a.worker)
        return
    if not a.out:
        a.out = os.path.join(HERE, "profiles", "asg_beam_graph_c4.json" if a.graph else "asg_beam_c4.json")
    if a.graph:
        main_graph(a)
        return
    rec = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            rec = json.load(f)
    rows_bytes, search_bytes, ctc_rows_bytes = byte_model()
    if a.merge_stats:
        means = {}
        with open(a.merge_stats) as f:
            for row in csv.DictReader(f):
                for key, names in KERNELS.items():
                    if any(n in row["Name"] for n in names):
                        ms = float(row["AverageNs"]) * 1e-6
                        means[key] = {"calls": int(row["Calls"]), "mean_ms": ms, "us_per_frame_of_the_batch": ms * 1e3 / T,
                                      "min_ms": float(row["MinNs"]) * 1e-6, "max_ms": float(row["MaxNs"]) * 1e-6}
        assert len(means) == len(KERNELS), means
        rec["kernels"] = means
        for key, nbytes in (("asg_beam_rows_kernel", rows_bytes), ("ctc_beam_rows_kernel", ctc_rows_bytes)):
            gbs = nbytes / (means[key]["mean_ms"] * 1e-3) / 1e9
            rec[key + "_on_its_byte_model"] = {"achieved_GBs": gbs, "stream_rate_GBs": STREAM_GBS,
                                               "frac": gbs / STREAM_GBS, "floor_ms": nbytes / (STREAM_GBS * 1e9) * 1e3}
        rec["asg_search_over_ctc_search_with_table"] = (means["asg_beam_search_kernel"]["mean_ms"]
                                                        / means["ctc_beam_search_kernel<true>"]["mean_ms"])
        rec["asg_rows_over_ctc_rows"] = means["asg_beam_rows_kernel"]["mean_ms"] / means["ctc_beam_rows_kernel"]["mean_ms"]
    else:
        asg, ctc, last, last_ctc = [], [], None, None
        for _ in range(3):
            last = run_worker("asg")
            assert last["asg_beam_utterances"] > 0 and last["second_run_has_the_same_bits"], last
            asg.append(last["ms_per_batch"])
            last_ctc = run_worker("ctc_lm")
            ctc.append(last_ctc["ms_per_batch"])
        rec.update({"shape": {"B": B, "T": T, "C": C, "beam_size": BEAM, "cutoff_top_n": TOPN, "nbest": NBEST,
                              "table": "normal(0, 1), seeded, C + C * C float32"},
                    "unit": "ms per batch, host clock around a closing synchronise, windows >= 0.5 s",
                    "asg": dict(spread(asg), what="Batch.asg_beam_decode (tokens, lengths, scores)", utterances=B,
                                mean_length=last["mean_length"], mean_score=last["mean_score"],
                                slots_with_a_hypothesis=last["slots_with_a_hypothesis"]),
                    "ctc_lm": dict(spread(ctc), what="Batch.ctc_beam_decode(lm=table, lm_weight=1, insertion_bonus=0, "
                                   "blank=0) on the same tensor", utterances=B, mean_length=last_ctc["mean_length"]),
                    "asg_over_ctc_lm": sorted(asg)[1] / sorted(ctc)[1],
                    "rows_bytes": rows_bytes, "search_bytes": search_bytes})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
