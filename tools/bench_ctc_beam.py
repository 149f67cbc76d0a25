"""CTC prefix beam search with N-best output on the device at BASELINE config C3's shape (B = 512, T = 1000, C = 256),
beam_size 16, cutoff_top_n 16, nbest 1, beside the greedy decode of the same tensor.

  beam    Batch.ctc_beam_decode: two launches (ctc_beam_rows_kernel, ctc_beam_search_kernel), tokens / lengths /
          scores written into the caller's tensors, no copy back
  greedy  Batch.linear_decode on the same tensor in the same process: its row kernel is the pure stream the beam
          search's row kernel adds the top-K rounds to

There is no route for this call on the previous commit, so there is nothing to alternate with and no speed-up to
claim.

    python tools/bench_ctc_beam.py [--out profiles/ctc_beam_c3.json]
        three samples, every sample a process of its own that warms its shapes up and then times windows of at least
        half a second with a host clock around a closing synchronise, for `beam` and for `greedy`
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_ctc_beam.py --worker trace
        a few calls of both, for the mean times of the kernels (a run of its own: no counters, no other tracing);
        with --beam W --topn K the trace runs at another beam_size / cutoff_top_n (the search kernel's time against
        the number of candidates per frame: what a frame costs when there is next to nothing to rank);
    python tools/bench_ctc_beam.py --merge-stats DIR/.../kernel_stats.csv [--beam W --topn K] [--out ...]
        adds those means to the record: the row kernel beside linear_decode_rows_kernel and as a fraction of its own
        byte model (4 C in, 8 (K + 1) + 4 out per row) at the stream rate, the search kernel per batch and per frame.

    python tools/bench_ctc_beam.py --lm [--out profiles/ctc_beam_lm_c3.json]
        the same tensor with a seeded bigram table fused in (Batch.ctc_beam_decode(lm=...), lm_weight 0.8,
        insertion_bonus 0.5, am_scores written too) beside the call without one: three samples of each, alternating,
        every sample a process of its own.  `--worker trace --lm` and `--merge-stats CSV --lm` add the mean times of
        the two instantiations of the search kernel (ms per batch, us per frame) and the cost of the table over the
        call without it; with `--lm-weight 0 --lm-bonus 0` on both, the same at a weight and bonus of zero, where the
        two searches keep the same prefixes and only the table's code differs.

    python tools/bench_ctc_beam.py --graph [--out profiles/ctc_beam_graph_c3.json]
        the same tensor with a compiled LM graph fused in (Batch.ctc_beam_decode(lm=gtn_amd.LmGraph(...)); DESIGN
        section 30) beside the table: the SAME bigram spelled as a graph (a start state and a state per label, C + C * C
        arcs; every state has all 256 labels, so a lookup is the one-load form), and a synthetic back-off trigram over the same alphabet (a unigram
        state with every label, a bigram state per label with a quarter of the arcs, a trigram state for a tenth of the
        label pairs with a quarter of the arcs, epsilon arcs one order down).  Three samples of each, alternating, every
        sample a process of its own.  `--worker trace --graph bigram|trigram` and `--merge-stats CSV --graph
        bigram|trigram` add the mean times of the search kernel's instantiations in that trace (ms per batch, us per
        frame) and the graph's cost over the table's.

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
B, T, C = 512, 1000, 256
BLANK, BEAM, TOPN, NBEST = 0, 16, 16, 1
WINDOW_S = 0.5
LM_WEIGHT, LM_BONUS = 0.8, 0.5


def inputs(torch):
    """log-softmax of seeded normals with a blank that wins about half of the frames, in runs"""
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    em = torch.randn((B, T, C), generator=g, device="cuda", dtype=torch.float32) * 3.0
    em[:, :, BLANK] += (torch.rand((B, T // 8 + 1, 1), generator=g, device="cuda") < 0.5).repeat_interleave(
        8, dim=1)[:, :T, 0] * 12.0
    return torch.log_softmax(em, dim=2).contiguous()


def byte_model():
    """(rows kernel, search kernel): 4 C in and 8 (K + 1) + 4 out per row; those back in, at most a trie node per beam
    and frame, the output rows"""
    rows = float(B) * T * (4.0 * C + 8.0 * (TOPN + 1) + 4.0)
    search = float(B) * (T * (8.0 * (TOPN + 1) + 4.0 + 8.0 * BEAM) + NBEST * (4.0 * T + 8.0))
    return rows, search


def lm_table(torch):
    """a seeded bigram table [C + C * C]: normal(0, 2)"""
    g = torch.Generator(device="cuda")
    g.manual_seed(4321)
    return (torch.randn((C + C * C,), generator=g, device="cuda", dtype=torch.float32) * 2.0).contiguous()


def bigram_graph(gtn, np, table, C=C):
    """the table [C + C * C] as a graph: state 0 the start, state 1 + c after label c, every arc"""
    g = gtn.Graph(False)
    g.add_nodes(np.arange(1 + C) == 0, np.ones(1 + C, bool))
    lab = np.arange(C)
    i, j = np.meshgrid(lab, lab, indexing="ij")  # entry C + i * C + j: label j followed by label i
    g.add_arcs(np.concatenate([np.zeros(C, np.int64), 1 + j.ravel()]), np.concatenate([1 + lab, 1 + i.ravel()]),
               np.concatenate([lab, i.ravel()]), None, table)
    return g


def trigram_graph(gtn, np, seed=4321, arcs_share=0.25, pairs_share=0.1, C=C):
    """a seeded back-off trigram over C labels: state 0 the unigram state (every label) and the start, 1 + i the bigram
    state after i, then a trigram state per kept pair (j, i); a state has `arcs_share` of the labels and an epsilon arc
    one order down; an arc labelled k out of a state that ends in i leads to the trigram state (i, k) where that is
    kept, else to the bigram state k"""
    rng = np.random.default_rng(seed)
    kept = rng.random((C, C)) < pairs_share
    tri = np.full((C, C), -1, np.int64)
    tri[kept] = 1 + C + np.arange(int(kept.sum()))
    n = 1 + C + int(kept.sum())
    ends = np.concatenate([np.arange(C), np.nonzero(kept)[1]])  # the last label of states 1 ..
    have = rng.random((n - 1, C)) < arcs_share
    s, k = np.nonzero(have)
    i = ends[s]
    src = np.concatenate([np.zeros(C, np.int64), 1 + s, 1 + np.arange(n - 1)])
    dst = np.concatenate([1 + np.arange(C), np.where(tri[i, k] >= 0, tri[i, k], 1 + k),
                          np.concatenate([np.zeros(C, np.int64), 1 + ends[C:]])])
    lab = np.concatenate([np.arange(C), k, np.full(n - 1, -1)])
    wt = np.concatenate([rng.normal(0, 2, C + len(s)), rng.normal(-1, 0.5, n - 1)]).astype(np.float32)
    g = gtn.Graph(False)
    g.add_nodes(np.arange(n) == 0, np.ones(n, bool))
    g.add_arcs(src, dst, lab, None, wt)
    return g


def worker(kind, beam=BEAM, topn=TOPN, lm=False, lm_weight=LM_WEIGHT, lm_bonus=LM_BONUS, graph=None):
    sys.path.insert(0, HERE)
    import torch
    import gtn_amd as gtn
    assert torch.cuda.is_available() and gtn.device_count() > 0, "bench_ctc_beam needs a GPU"
    em = inputs(torch)
    tokens = torch.empty((B, NBEST, T), dtype=torch.int32, device="cuda")
    lengths = torch.empty((B, NBEST), dtype=torch.int32, device="cuda")
    scores = torch.empty((B, NBEST), dtype=torch.float32, device="cuda")
    labels = torch.empty((B, T), dtype=torch.int32, device="cuda")
    gtok = torch.empty((B, T), dtype=torch.int32, device="cuda")
    gsta = torch.empty((B, T), dtype=torch.int32, device="cuda")
    gsc = torch.empty((B,), dtype=torch.float32, device="cuda")
    glen = torch.empty((B,), dtype=torch.int32, device="cuda")
    table = lm_table(torch) if lm or graph or kind in ("beam_lm", "beam_bigram") else None
    if kind in ("beam_bigram", "beam_trigram"):
        graph = kind[5:]
    lmg = None
    if graph:
        import numpy as np
        lmg = gtn.LmGraph(bigram_graph(gtn, np, table.cpu().numpy()) if graph == "bigram" else trigram_graph(gtn, np))

    def beam_graph_step():
        ems = gtn.Batch.linear(B, T, C, em, False, True)
        ems.ctc_beam_decode(tokens, lengths, scores, None, BLANK, beam, topn, NBEST, lm=lmg, lm_weight=lm_weight,
                            insertion_bonus=lm_bonus, am_scores_out=am_scores)
    am_scores = torch.empty((B, NBEST), dtype=torch.float32, device="cuda")

    def beam_lm_step():
        ems = gtn.Batch.linear(B, T, C, em, False, True)
        ems.ctc_beam_decode(tokens, lengths, scores, None, BLANK, beam, topn, NBEST, lm=table, lm_weight=lm_weight,
                            insertion_bonus=lm_bonus, am_scores_out=am_scores)

    def beam_step():
        ems = gtn.Batch.linear(B, T, C, em, False, True)
        ems.ctc_beam_decode(tokens, lengths, scores, None, BLANK, beam, topn, NBEST)

    def greedy_step():
        ems = gtn.Batch.linear(B, T, C, em, False, True)
        ems.linear_decode(labels, gsc, None, BLANK, gtok, gsta, glen)

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
            beam_step()
            if graph:
                beam_lm_step()
                beam_graph_step()
            elif lm:
                beam_lm_step()
            else:
                greedy_step()
            sync()
        print(json.dumps({"trace": "done"}))
        return
    c0 = gtn.debug_ctc_beam_stats()
    ms, n = timed({"beam": beam_step, "beam_lm": beam_lm_step, "greedy": greedy_step, "beam_bigram": beam_graph_step,
                   "beam_trigram": beam_graph_step}[kind])
    sync()
    c1 = gtn.debug_ctc_beam_stats()
    rec = {"kind": kind, "utterances": B, "ms_per_batch": ms, "iters": n, "beam_utterances": c1[1] - c0[1]}
    if lmg is not None:
        rec["graph"] = lmg.info()
    if kind in ("beam_lm", "beam_bigram", "beam_trigram"):
        rec["mean_length"] = float(lengths.float().mean().item())
        rec["mean_score"] = float(scores.mean().item())
        rec["mean_am_score"] = float(am_scores.mean().item())
        first = tokens.clone()
        beam_step()
        sync()
        rec["utterances_whose_first_hypothesis_differs_from_the_call_without_a_table"] = int(
            (first != tokens).any(dim=2).any(dim=1).sum().item())
        if kind == "beam_bigram":  # (the same model: the same bytes)
            beam_lm_step()
            sync()
            rec["utterances_whose_first_hypothesis_differs_from_the_table"] = int(
                (first != tokens).any(dim=2).any(dim=1).sum().item())
    if kind == "beam":
        rec["mean_length"] = float(lengths.float().mean().item())
        rec["mean_score"] = float(scores.mean().item())
        beam_step()
        greedy_step()
        sync()
        # the summed score of the best label sequence is at least the score of the best alignment (up to rounding)
        rec["beam_score_minus_greedy_score_min"] = float((scores[:, 0] - gsc).min().item())
    print(json.dumps(rec))


def run_worker(kind):
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", kind], env=env,
                         stdout=subprocess.PIPE, timeout=500, check=True).stdout.decode()
    rec = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    print(f"[bench_ctc_beam] {kind}: {rec['ms_per_batch']:.3f} ms per batch of {rec['utterances']}", file=sys.stderr,
          flush=True)
    return rec


def spread(v):
    return {"samples": v, "min": min(v), "max": max(v), "median": sorted(v)[len(v) // 2]}


KERNELS = ("ctc_beam_rows_kernel", "ctc_beam_search_kernel", "linear_decode_rows_kernel",
           "linear_decode_collapse_kernel")


# (the template parameter was a bool before the graph instantiation: both spellings, so that a trace of the commit
#  before can be merged too)
LM_KERNELS = {"without_table": ("ctc_beam_search_kernel<false>", "ctc_beam_search_kernelILb0E",
                                "ctc_beam_search_kernel<0>", "ctc_beam_search_kernelILi0E"),
              "with_table": ("ctc_beam_search_kernel<true>", "ctc_beam_search_kernelILb1E",
                             "ctc_beam_search_kernel<1>", "ctc_beam_search_kernelILi1E")}
GRAPH_KERNEL = ("ctc_beam_search_kernel<2>", "ctc_beam_search_kernelILi2E")


def kernel_means(path, kernels):
    means = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for key, names in kernels.items():
                if any(n in row["Name"] for n in names):
                    ms = float(row["AverageNs"]) * 1e-6
                    means[key] = {"calls": int(row["Calls"]), "ms_per_batch": ms, "us_per_frame_of_the_batch": ms * 1e3 / T,
                                  "min_ms": float(row["MinNs"]) * 1e-6, "max_ms": float(row["MaxNs"]) * 1e-6}
    return means


def main_graph(a):
    """the --graph record: end to end with the table, the bigram graph and the trigram graph, or (--merge-stats) the
    search kernels' means of a trace with one of the graphs"""
    rec = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            rec = json.load(f)
    if a.merge_stats:
        means = kernel_means(a.merge_stats, dict(LM_KERNELS, with_graph=GRAPH_KERNEL))
        assert len(means) == 3, means
        rec["search_kernel_" + a.graph] = means
        rec[f"search_kernel_with_{a.graph}_graph_over_with_table"] = (means["with_graph"]["ms_per_batch"]
                                                                      / means["with_table"]["ms_per_batch"])
    else:
        kinds = ("beam_lm", "beam_bigram", "beam_trigram")
        samples, last = {k: [] for k in kinds}, {}
        for _ in range(3):
            for k in kinds:
                last[k] = run_worker(k)
                assert last[k]["beam_utterances"] > 0, last[k]
                samples[k].append(last[k]["ms_per_batch"])
        med = {k: sorted(v)[1] for k, v in samples.items()}
        rec.update({"shape": {"B": B, "T": T, "C": C, "blank": BLANK, "beam_size": BEAM, "cutoff_top_n": TOPN,
                              "nbest": NBEST, "lm_weight": LM_WEIGHT, "insertion_bonus": LM_BONUS},
                    "unit": "ms per batch, host clock around a closing synchronise, windows >= 0.5 s",
                    "beam_lm": dict(spread(samples["beam_lm"]), what="Batch.ctc_beam_decode(lm=table)", utterances=B),
                    "beam_bigram": dict(spread(samples["beam_bigram"]), what="the same bigram as an LmGraph",
                                        utterances=B, graph=last["beam_bigram"]["graph"]),
                    "beam_trigram": dict(spread(samples["beam_trigram"]), what="a synthetic back-off trigram LmGraph",
                                         utterances=B, graph=last["beam_trigram"]["graph"]),
                    "beam_bigram_over_beam_lm": med["beam_bigram"] / med["beam_lm"],
                    "beam_trigram_over_beam_lm": med["beam_trigram"] / med["beam_lm"],
                    "walks_per_frame_at_most": BEAM * TOPN,
                    "bigram_graph_first_hypotheses_that_differ_from_the_table":
                        last["beam_bigram"]["utterances_whose_first_hypothesis_differs_from_the_table"]})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


def main_lm(a):
    """the --lm record: end to end with and without the table, or (--merge-stats) the two search kernels' means"""
    rec = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            rec = json.load(f)
    if a.merge_stats:
        means = kernel_means(a.merge_stats, LM_KERNELS)
        assert len(means) == 2, means
        # (at weight = bonus = 0 the search is the one without a table, step for step: what the table's code costs)
        tag = "" if (a.lm_weight, a.lm_bonus) == (LM_WEIGHT, LM_BONUS) else f"_at_weight_{a.lm_weight:g}_bonus_{a.lm_bonus:g}"
        rec["search_kernel" + tag] = means
        rec["search_kernel_with_table_over_without" + tag] = (means["with_table"]["ms_per_batch"]
                                                              / means["without_table"]["ms_per_batch"])
    else:
        plain, fused, last = [], [], None
        for _ in range(3):
            plain.append(run_worker("beam")["ms_per_batch"])
            last = run_worker("beam_lm")
            assert last["beam_utterances"] > 0, last
            fused.append(last["ms_per_batch"])
        rec.update({"shape": {"B": B, "T": T, "C": C, "blank": BLANK, "beam_size": BEAM, "cutoff_top_n": TOPN,
                              "nbest": NBEST, "lm_weight": LM_WEIGHT, "insertion_bonus": LM_BONUS,
                              "table": "normal(0, 2), seeded, C + C * C float32"},
                    "unit": "ms per batch, host clock around a closing synchronise, windows >= 0.5 s",
                    "beam": dict(spread(plain), what="Batch.ctc_beam_decode without a table", utterances=B),
                    "beam_lm": dict(spread(fused), what="Batch.ctc_beam_decode(lm=...) with am_scores_out",
                                    utterances=B),
                    "beam_lm_over_beam": sorted(fused)[1] / sorted(plain)[1],
                    "gathers_per_frame_at_most": BEAM * (TOPN + 1),
                    "mean_length": last["mean_length"], "mean_score": last["mean_score"],
                    "mean_am_score": last["mean_am_score"],
                    "utterances_whose_first_hypothesis_differs_from_the_call_without_a_table":
                        last["utterances_whose_first_hypothesis_differs_from_the_call_without_a_table"]})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=["beam", "beam_lm", "beam_bigram", "beam_trigram", "greedy", "trace"])
    ap.add_argument("--lm", action="store_true")
    ap.add_argument("--graph", nargs="?", const="bigram", choices=["bigram", "trigram"])
    ap.add_argument("--lm-weight", type=float, default=LM_WEIGHT)
    ap.add_argument("--lm-bonus", type=float, default=LM_BONUS)
    ap.add_argument("--merge-stats")
    ap.add_argument("--beam", type=int, default=BEAM)
    ap.add_argument("--topn", type=int, default=TOPN)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.beam, a.topn, a.lm, a.lm_weight, a.lm_bonus, a.graph)
        return
    if not a.out:
        a.out = os.path.join(HERE, "profiles", "ctc_beam_graph_c3.json" if a.graph else
                             "ctc_beam_lm_c3.json" if a.lm else "ctc_beam_c3.json")
    if a.graph:
        main_graph(a)
        return
    if a.lm:
        main_lm(a)
        return
    rec = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            rec = json.load(f)
    rows_bytes, search_bytes = byte_model()
    if a.merge_stats and (a.beam, a.topn) != (BEAM, TOPN):
        with open(a.merge_stats) as f:
            for row in csv.DictReader(f):
                if "ctc_beam_search_kernel" in row["Name"]:
                    ms = float(row["AverageNs"]) * 1e-6
                    rec.setdefault("search_kernel_by_setting", {})[f"beam_size {a.beam}, cutoff_top_n {a.topn}"] = {
                        "ms_per_batch": ms, "us_per_frame_of_the_batch": ms * 1e3 / T,
                        "candidates_per_frame_at_most": a.beam + a.beam * a.topn}
                if "ctc_beam_rows_kernel" in row["Name"]:
                    rec.setdefault("rows_kernel_by_setting", {})[f"cutoff_top_n {a.topn}"] = float(row["AverageNs"]) * 1e-6
    elif a.merge_stats:
        means = {}
        with open(a.merge_stats) as f:
            for row in csv.DictReader(f):
                for key in KERNELS:
                    if key in row["Name"]:
                        means[key] = {"calls": int(row["Calls"]), "mean_ms": float(row["AverageNs"]) * 1e-6,
                                      "min_ms": float(row["MinNs"]) * 1e-6, "max_ms": float(row["MaxNs"]) * 1e-6}
        rec["kernels"] = means
        k, sib = means.get("ctc_beam_rows_kernel"), means.get("linear_decode_rows_kernel")
        if k:
            gbs = rows_bytes / (k["mean_ms"] * 1e-3) / 1e9
            rec["rows_kernel_on_its_byte_model"] = {
                "achieved_GBs": gbs, "stream_rate_GBs": STREAM_GBS, "frac": gbs / STREAM_GBS,
                "floor_ms": rows_bytes / (STREAM_GBS * 1e9) * 1e3, "bytes": "(4 C + 8 (K + 1) + 4) per row"}
            if sib:
                rec["rows_kernel_over_linear_decode_rows_kernel"] = k["mean_ms"] / sib["mean_ms"]
        k = means.get("ctc_beam_search_kernel")
        if k:
            rec["search_kernel"] = {"ms_per_batch": k["mean_ms"], "us_per_frame_of_the_batch": k["mean_ms"] * 1e3 / T,
                                    "workgroups": B, "achieved_GBs": search_bytes / (k["mean_ms"] * 1e-3) / 1e9}
    else:
        be, gr, last = [], [], None
        for _ in range(3):
            last = run_worker("beam")
            assert last["beam_utterances"] > 0, last
            be.append(last["ms_per_batch"])
            gr.append(run_worker("greedy")["ms_per_batch"])
        rec.update({"shape": {"B": B, "T": T, "C": C, "blank": BLANK, "beam_size": BEAM, "cutoff_top_n": TOPN,
                              "nbest": NBEST},
                    "unit": "ms per batch, host clock around a closing synchronise, windows >= 0.5 s",
                    "beam": dict(spread(be), what="Batch.ctc_beam_decode (tokens, lengths, scores)", utterances=B),
                    "greedy": dict(spread(gr), what="Batch.linear_decode on the same tensor (all five outputs)",
                                   utterances=B),
                    "rows_bytes": rows_bytes, "search_bytes": search_bytes,
                    "mean_length": last["mean_length"], "mean_score": last["mean_score"],
                    "beam_score_minus_greedy_score_min": last["beam_score_minus_greedy_score_min"]})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
