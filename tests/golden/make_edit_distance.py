"""tests/golden/edit_distance.json: the UNMODIFIED reference's own edit distance, the form of its
examples/edit_distance.cpp -- -viterbiScore(compose(hyp, compose(edits, ref))) with an edits graph of alphabet^2 + 2 *
alphabet arcs -- on the seeded pairs of edit_distance_fp.GOLDEN_SPECS, through tests/refbackend/gtn_ref.py
(oracle/_ref/libgtn_ref.so).  Run where that library exists (it is built where the reference's sources are); only the
recorded numbers and the seeds are committed, and only this generator reads the reference.
test_edit_distance_cpu.py compares the yardstick of tests/edit_distance_fp.py with the result."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "refbackend"))

import edit_distance_fp as fp  # noqa: E402


def chain(gtn, tokens):
    g = gtn.Graph(False)
    g.add_node(True, len(tokens) == 0)
    for i, t in enumerate(tokens):
        g.add_node(False, i == len(tokens) - 1)
        g.add_arc(i, i + 1, int(t), int(t), 0.0)
    return g


def edits_graph(gtn, alphabet):
    g = gtn.Graph(False)
    g.add_node(True, True)
    for i in range(alphabet):
        for j in range(alphabet):
            g.add_arc(0, 0, i, j, -float(i != j))
        g.add_arc(0, 0, i, gtn.epsilon, -1.0)
        g.add_arc(0, 0, gtn.epsilon, i, -1.0)
    return g


def reference_distance(gtn, ref, hyp, alphabet):
    score = gtn.viterbi_score(gtn.compose(chain(gtn, hyp), gtn.compose(edits_graph(gtn, alphabet), chain(gtn, ref))))
    return int(round(-score.item()))


if __name__ == "__main__":
    import gtn_ref
    assert gtn_ref.backend() == "reference-cpu", gtn_ref.backend()
    out = []
    for seed, m, n, alphabet in fp.GOLDEN_SPECS:
        ref, hyp = fp.seeded_pair(seed, m, n, alphabet)
        out.append({"seed": seed, "len_ref": m, "len_hyp": n, "alphabet": alphabet,
                    "dist": reference_distance(gtn_ref, ref, hyp, alphabet)})
    with open(os.path.join(HERE, "edit_distance.json"), "w") as f:
        json.dump({"source": "reference -viterbiScore(compose(hyp, compose(edits, ref)))", "pairs": out}, f, indent=1)
    print(len(out), "pairs", [o["dist"] for o in out])
