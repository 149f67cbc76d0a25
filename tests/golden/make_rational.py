"""tests/golden/rational.json: what the UNMODIFIED reference (oracle/_ref/libgtn_ref.so through
tests/refbackend/gtn_ref.py) builds for the small graphs of tests/rational_cases.py -- every result and probe of CASES
with at most SMALL_N nodes and SMALL_A arcs, in full -- and the arcs of its viterbi_path for TIE_CASES, whose paths all
tie exactly.  Run where that library exists (it is built where the reference's sources are); only the recorded results
are committed, and only this generator reads the reference.  tests/test_rational_cpu.py compares the yardstick of
tests/rational_fp.py with the result, so the yardstick stays pinned where the library is absent."""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "refbackend"))

import rational_cases as rc  # noqa: E402
import rational_fp as fp  # noqa: E402

SMALL_N, SMALL_A = 40, 80


def is_small(g):
    return fp.N(g) <= SMALL_N and fp.A(g) <= SMALL_A


def pack(g):
    """nodes as id lists, arcs as one flat list {src, dst, ilabel, olabel} x A, weights as float32 bit patterns"""
    return {"N": fp.N(g), "start": fp.start_list(g).tolist(), "accept": fp.accept_list(g).tolist(),
            "arcs": np.stack([g["src"], g["dst"], g["il"], g["ol"]], 1).reshape(-1).tolist(),
            "w_bits": g["w"].view(np.int32).tolist()}


def unpack(p):
    start, accept = np.zeros(p["N"], np.uint8), np.zeros(p["N"], np.uint8)
    start[p["start"]] = 1
    accept[p["accept"]] = 1
    a = np.asarray(p["arcs"], np.int32).reshape(-1, 4)
    return fp.graph(start, accept, a[:, 0], a[:, 1], a[:, 2], a[:, 3], np.asarray(p["w_bits"], np.int32).view(np.float32))


if __name__ == "__main__":
    import gtn_ref
    assert gtn_ref.backend() == "reference-cpu", gtn_ref.backend()
    graphs, ties = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, case in rc.CASES.items():
            ops = rc.ApiOps(gtn_ref, tmp)
            got = case(ops)
            for kind in ("results", "probes"):
                for key, h in got[kind].items():
                    g = ops.pull(h)
                    if is_small(g):
                        graphs["%s/%s/%s" % (name, kind, key)] = pack(g)
        for name, case in rc.TIE_CASES.items():
            ops = rc.ApiOps(gtn_ref, tmp)
            ties[name] = pack(ops.pull(case(ops)))
    with open(os.path.join(HERE, "rational.json"), "w") as f:
        json.dump({"source": "reference clone / concat / closure / union_ / remove / load / viterbiPath",
                   "small": [SMALL_N, SMALL_A], "graphs": graphs, "ties": ties}, f, separators=(",", ":"))
    print(len(graphs), "graphs,", len(ties), "tie paths,", os.path.getsize(os.path.join(HERE, "rational.json")), "bytes")
