"""The yardstick of the ASG prefix beam search tests: the recursion of DESIGN section 27 in numpy, parameterised by the
float type and by how log-add is spelled (the three host forms of tests/ctc_beam_fp.py, whose log-add, vetting rule and
emission generators are imported, not restated).

  hypotheses  label sequences without equal neighbours, each summed over all of its alignments under emissions o
              transitions: every frame labelling collapses to exactly one of them
  table       w [C + C*C] float32 in the arc order of asgTransitions: w[c] = start[c], w[C + i*C + j] = tr[i][j], label
              j followed by label i
  token set   S_t = the K best labels of row t (value descending, of equal values the smaller label; NaN and -inf are
              never chosen); no blank is appended; S_t restricts stays as well as extensions
  state       at most W distinct prefixes with ONE score a(p); the empty prefix with 0 to begin with, and it has no stay
  frame       stay (l = last(p) in S_t):       (a(p) + tr[l][l]) + x[l]
              extension by c in S_t, c != l:   s = (a(p) + w) + x[c], w = start[c] for the empty prefix, else tr[c][l]
              a w that is not finite drops its candidate, and so does a value that is not above -inf
              an extension that spells a prefix q of the list: stay(q) = logadd(stay(q), s), no candidate
              order: total descending, stays before extensions, parent's rank ascending, label ascending; the first W
  result      the first nbest of the final list: tokens, length, score; nothing where no candidate is left or T = 0

The form "f32" IS the contract; "f32log" (m + log(1 + exp(n - m)) in place of log1p) only widens err for the vetting.
`vet` (ctc_beam_fp) says whether a continuous case can be compared with == on tokens.

tests/test_asg_beam_cpu.py pins the float64 form to a brute-force enumeration, to the oracle's forwardScore and to
tests/asg_score_fp.py; tests/test_asg_beam_gpu.py judges the kernels by it.
"""
import functools
import itertools

import numpy as np

import ctc_beam_fp as cf
from ctc_beam_fp import FORMS, GAP_FACTOR, SCORE_FACTOR, case_err, logadd, vet  # noqa: F401  (the shared rules)
from ctc_beam_fp import continuous_case, dead_case, holes_case, integer_case  # noqa: F401  (the emission generators)


def token_set(row, K):
    """(labels, values) of S_t, in the order the K best are chosen"""
    x = np.asarray(row, np.float32)
    v = np.where(np.isnan(x), np.float32(-np.inf), x)
    order = np.argsort(-v, kind="stable")[:K]  # (stable: of equal values the smaller label first)
    order = order[v[order] > -np.inf]
    return order.astype(np.int64), x[order]


def beam_search(em, table, W, K, form="f64", frames=None, fresh_nodes=False, stats=None):
    """em [M, C], table [C + C*C] -> the final list [(tokens tuple, score)] (at most W entries, in order), the form's
    arithmetic.  fresh_nodes=True is NOT the contract: it numbers every kept extension anew and knows a prefix by that
    number alone, so a prefix that left the list and is created again is no longer recognised as the parent of its child
    that stayed (duplicate prefixes, split mass).  It exists to find and to certify the RECREATED_CASES below.
    stats["recreated"] counts the kept extensions whose prefix was in the trie already."""
    ft = cf._ft(form)
    em = np.asarray(em, np.float32)
    C = em.shape[1]
    tab = np.asarray(table, np.float32).astype(ft)
    T = em.shape[0] if frames is None else int(frames)
    if T == 0:
        return []
    NEG = ft(-np.inf)
    parent, label, child = [-1], [-1], {}  # the trie: node -> (parent, label); node 0 is the empty prefix
    node = np.array([0])
    a = np.array([0.0], ft)
    for t in range(T):
        n = len(node)
        if n == 0:
            break
        sl, sv = token_set(em[t], K)
        sv = sv.astype(ft)
        last = np.array([label[v] for v in node])
        col_of = {int(c): k for k, c in enumerate(sl)}
        with np.errstate(all="ignore"):
            # the stays
            lk = np.array([col_of.get(int(l), -1) for l in last])
            wself = np.where(last >= 0, tab[C + np.maximum(last, 0) * (C + 1)], NEG).astype(ft)
            xl = np.where(lk >= 0, sv[np.maximum(lk, 0)] if len(sv) else NEG, NEG).astype(ft)
            stay = ((a + wself).astype(ft) + xl).astype(ft)
            stay = np.where((lk >= 0) & np.isfinite(wself) & (stay > -np.inf), stay, NEG).astype(ft)
            # the extensions
            at = np.where(last[:, None] < 0, sl[None, :], C + sl[None, :] * C + np.maximum(last[:, None], 0))
            w = tab[at].reshape(n, len(sl))
            s = ((a[:, None] + w).astype(ft) + sv[None, :]).astype(ft)
            ok = (sl[None, :] != last[:, None]) & np.isfinite(w) & (s > -np.inf)
        rank_of = {int(v): i for i, v in enumerate(node)}
        for j in range(n):  # an extension that is a prefix of the list already joins that prefix
            i, k = rank_of.get(parent[node[j]]), int(lk[j])
            if i is not None and k >= 0 and ok[i, k]:
                stay[j] = logadd(stay[j:j + 1], s[i:i + 1, k], form)[0]
                ok[i, k] = False
        ei, ek = np.nonzero(ok)
        total = np.concatenate([stay, s[ei, ek]])
        kind = np.concatenate([np.zeros(n, np.int64), np.ones(len(ei), np.int64)])
        rank = np.concatenate([np.arange(n), ei])
        lab = np.concatenate([np.full(n, -1), sl[ek]])
        keep = total > -np.inf
        total, kind, rank, lab = total[keep], kind[keep], rank[keep], lab[keep]
        order = np.lexsort((lab, rank, kind, -total))[:W]
        new_node, new_a = [], []
        for o in order:
            i = int(rank[o])
            if kind[o] == 0:
                new_node.append(int(node[i]))
            else:
                key = (int(node[i]), int(lab[o]))
                if key in child and stats is not None:
                    stats["recreated"] = stats.get("recreated", 0) + 1
                if fresh_nodes or key not in child:
                    child[key] = len(parent)
                    parent.append(key[0])
                    label.append(key[1])
                new_node.append(child[key])
            new_a.append(total[o])
        node, a = np.array(new_node, np.int64), np.array(new_a, ft)
    out = []
    for v, sc in zip(node, a):
        toks = []
        while v > 0:
            toks.append(label[v])
            v = parent[v]
        out.append((tuple(reversed(toks)), sc))
    return out


def decode_batch(em, table, frames, W, K, nbest, form="f64"):
    """em [B, M, C] -> (tokens int32 [B, nbest, M], lengths int32 [B, nbest], scores [B, nbest] of the form's type):
    what the engine's call writes"""
    B, M, _ = em.shape
    return rows_of([beam_search(em[b], table, W, K, form, None if frames is None else frames[b]) for b in range(B)],
                   M, nbest, form)


def rows_of(hyps, M, nbest, form="f64"):
    """the final lists of a batch as the engine's call writes them"""
    B = len(hyps)
    tokens = np.full((B, nbest, M), -1, np.int32)
    lengths = np.zeros((B, nbest), np.int32)
    scores = np.full((B, nbest), -np.inf, cf._ft(form))
    for b, hyp in enumerate(hyps):
        for r, (toks, sc) in enumerate(hyp[:nbest]):
            tokens[b, r, :len(toks)] = toks
            lengths[b, r] = len(toks)
            scores[b, r] = sc
    return tokens, lengths, scores


def brute_force(em, table, frames=None):
    """{label sequence without equal neighbours: log-sum over the labellings that collapse to it}, float64, over all
    C^T labellings"""
    em = np.asarray(em, np.float64)
    T, C = em.shape if frames is None else (int(frames), em.shape[1])
    tab = np.asarray(table, np.float64)
    out = {}
    if T == 0:
        return out
    with np.errstate(all="ignore"):
        for path in itertools.product(range(C), repeat=T):
            s = tab[path[0]] + em[0, path[0]]
            for t in range(1, T):
                s += tab[C + path[t] * C + path[t - 1]] + em[t, path[t]]
            if not s > -np.inf:
                continue
            y = tuple(k for k, _ in itertools.groupby(path))
            out[y] = np.logaddexp(out.get(y, -np.inf), s)
    return out


# ---- the case generators ----
def table_case(seed, C, holes=0.0):
    """seeded normal(0, 1) table; with `holes` that share of its entries -inf (a seeded choice), with ("nan", share)
    that share NaN"""
    w = np.random.default_rng(seed + 100).normal(0.0, 1.0, C + C * C).astype(np.float32)
    if holes:
        fill, share = (np.nan, holes[1]) if isinstance(holes, tuple) else (-np.inf, holes)
        w[np.random.default_rng(seed + 15000).random(C + C * C) < share] = fill
    return w


_KINDS = {"continuous": continuous_case, "holes": holes_case, "dead": dead_case}


@functools.lru_cache(maxsize=None)
def case_results(kind, seed, B, T, C, W, K, frames=None, holes=0.0):
    """(em, table, {form: [final list per utterance]}, re-creations in the float64 form) of a generated case, computed
    once per process and left unchanged"""
    em = _KINDS[kind](seed, B, T, C)
    table = table_case(seed, C, holes)
    em.setflags(write=False)
    table.setflags(write=False)
    stats = {}
    res = {f: [beam_search(em[b], table, W, K, f, None if frames is None else frames[b],
                           stats=stats if f == "f64" else None) for b in range(B)] for f in FORMS}
    return em, table, res, stats.get("recreated", 0)


def results_of(case):
    """case_results of an entry of the case lists below (its nbest is not part of the computation)"""
    kind, seed, B, T, C, W, K, _, frames, holes = case
    return case_results(kind, seed, B, T, C, W, K, frames, holes)


def fresh_results(case):
    """the float64 final lists of the case under fresh_nodes=True: identity by node number, which is not the contract"""
    kind, seed, B, T, C, W, K, _, frames, holes = case
    em, table, _, _ = results_of(case)
    return [beam_search(em[b], table, W, K, "f64", None if frames is None else frames[b], fresh_nodes=True)
            for b in range(B)]


def fresh_differs(case):
    """does fresh_nodes=True get a compared hypothesis of the case wrong?"""
    nbest = case[7]
    _, _, res, _ = results_of(case)
    return any([p for p, _ in h[:nbest]] != [p for p, _ in g[:nbest]]
               or any(abs(float(x) - float(y)) > 1e-9 for (_, x), (_, y) in zip(h[:nbest], g[:nbest]))
               for h, g in zip(res["f64"], fresh_results(case)))


# The cases test_asg_beam_gpu.py runs: (kind, seed, B, T, C, W, K, nbest, frames, table holes).  Seeds found by host
# search with `python tests/asg_beam_fp.py` (the first that vets and, where a log-add is involved, has err > 0);
# test_asg_beam_cpu.py asserts that every one vets.  Continuous cases compare at most the first 4 hypotheses;
# nbest = W only at T <= 3.  The shapes follow ctc_beam_fp.SHAPE_CASES: C at every head, tail and lanes-per-row variant of
# the row kernel (1, 2, 3, 5, 29, 33, 64, 65, 256, 257, 300, 1000), C <= K, T at 1, 2, 3, 63, 64, 65, 128, 129,
# B = 1, 2, 65, W = 1, 2, 63, 64, K = 1, 32, nbest = 1, 2, 4.
SHAPE_CASES = [
    ("continuous", 1, 1, 1, 1, 1, 1, 1, None, 0.0),
    ("continuous", 1, 2, 1, 2, 2, 2, 2, None, 0.0),
    ("continuous", 1, 2, 2, 3, 4, 3, 4, None, 0.0),
    ("continuous", 1, 2, 3, 300, 2, 1, 2, None, 0.0),
    ("continuous", 1, 65, 3, 5, 4, 3, 4, None, 0.0),
    ("continuous", 1, 2, 63, 5, 1, 4, 1, None, 0.0),
    ("continuous", 1, 2, 64, 33, 2, 32, 2, None, 0.0),
    ("continuous", 1, 2, 65, 5, 4, 3, 2, None, 0.0),
    ("continuous", 1, 2, 129, 33, 8, 4, 4, None, 0.0),
    ("continuous", 2, 1, 128, 64, 64, 32, 4, None, 0.0),
    ("continuous", 1, 2, 40, 65, 63, 32, 4, None, 0.0),
    ("continuous", 1, 2, 33, 1000, 16, 32, 4, None, 0.0),
    ("continuous", 1, 2, 64, 256, 32, 16, 2, None, 0.0),
    ("continuous", 1, 2, 129, 257, 16, 8, 1, None, 0.0),
    ("continuous", 1, 3, 65, 29, 16, 16, 4, None, 0.0),
    ("continuous", 1, 2, 2, 3, 64, 3, 4, None, 0.0),
    ("continuous", 1, 2, 3, 2, 16, 16, 1, None, 0.0),
]
K1_CASE = ("continuous", 1, 3, 65, 29, 4, 1, 2, None, 0.0)  # one label per frame: no log-add anywhere
RAGGED_FRAMES = cf.RAGGED_FRAMES  # T, T - 1, 1 and 0 among them
RAGGED_CASE = ("continuous", 1, 7, 40, 29, 8, 6, 2, RAGGED_FRAMES, 0.0)
RAGGED_ROWS_CASE = ("continuous", 1, 6, 40, 29, 8, 6, 2, tuple(f for f in RAGGED_FRAMES if f > 0), 0.0)
HOLES_CASE = ("dead", 1, 4, 33, 9, 8, 4, 2, None, 0.0)  # -inf and NaN emissions; utterance 1 has an all--inf row
# about a fifth of the table -inf / NaN, a start entry among them; the search on the table without holes returns a
# forbidden first label and a forbidden bigram (`python tests/asg_beam_fp.py constrained` finds the seeds)
CONSTRAINED_CASE = ("continuous", 2, 3, 40, 12, 16, 8, 4, None, 0.2)
NAN_TABLE_CASE = ("continuous", 2, 3, 40, 12, 16, 8, 4, None, ("nan", 0.2))
REPEAT_CASE = ("continuous", 1, 3, 65, 29, 16, 8, 4, None, 0.0)
# (T <= 3, C <= 4, W = 64, K = C: at most 4 + 12 + 36 = 52 hypotheses)
UNPRUNED_CASES = [("continuous", 1, 2, 1, 2, 64, 2, 2, None, 0.0), ("continuous", 1, 2, 2, 3, 64, 3, 4, None, 0.0),
                  ("continuous", 1, 2, 3, 4, 64, 4, 4, None, 0.0), ("continuous", 1, 2, 3, 3, 64, 3, 4, None, 0.0)]
TORCH_CASES = [("continuous", 1, 4, 40, 12, 16, 16, 1, None, 0.0),
               ("continuous", 1, 3, 75, 29, 8, 5, 3, (75, 0, 41), 0.0),
               ("continuous", 1, 66, 5, 9, 4, 4, 2, None, 0.0)]
# A prefix leaves the list while its child stays, and is created again later from its own parent: the child must still
# be recognised as that prefix plus a label (exact identity, not the number a node happened to get).  Seeds found by
# host search over the shapes of ctc_beam_fp.RECREATED_CASES (`python tests/asg_beam_fp.py recreated`): they vet, a
# prefix is created again, and beam_search(fresh_nodes=True) -- identity by node number -- gets their compared
# hypotheses wrong (test_asg_beam_cpu.py asserts all three).
RECREATED_SHAPES = [(2, 40, 4, 4, 4, 2), (2, 100, 5, 8, 5, 2), (2, 65, 3, 4, 3, 4), (2, 129, 6, 16, 6, 2),
                    (1, 40, 4, 4, 4, 1)]
RECREATED_CASES = [("continuous", seed, B, T, C, W, K, nbest, None, 0.0)
                   for seed, (B, T, C, W, K, nbest) in zip((5, 3, 1, 1, 6), RECREATED_SHAPES)]
ALL_GPU_CASES = (SHAPE_CASES + [K1_CASE, RAGGED_CASE, RAGGED_ROWS_CASE, HOLES_CASE, CONSTRAINED_CASE, NAN_TABLE_CASE,
                                REPEAT_CASE]
                 + UNPRUNED_CASES + TORCH_CASES + RECREATED_CASES)


def forbidden_first(table, y):
    return len(y) > 0 and not np.isfinite(table[y[0]])


def forbidden_bigram(table, C, y):
    return any(not np.isfinite(table[C + b * C + a]) for a, b in zip(y, y[1:]))


def constraints_bite(case):
    """does the search on the case's table WITHOUT its holes return, among the compared hypotheses, a first label and a
    bigram that the holes forbid?"""
    kind, seed, B, T, C, W, K, nbest, frames, holes = case
    em, table, _, _ = results_of(case)
    free = [y for b in range(B) for y, _ in beam_search(em[b], table_case(seed, C), W, K)[:nbest]]
    return any(forbidden_first(table, y) for y in free) and any(forbidden_bigram(table, C, y) for y in free)


def find_seed(case, tries=400, recreated=False, constrained=False):
    kind, _, B, T, C, W, K, nbest, frames, holes = case
    for seed in range(1, tries):
        trial = (kind, seed, B, T, C, W, K, nbest, frames, holes)
        _, _, res, again = results_of(trial)
        ok, err, gap = vet(res, nbest)
        good = (ok and (err > 0 or T == 1 or K == 1 or C == 1) and (not recreated or (again > 0 and fresh_differs(trial)))
                and (not constrained or constraints_bite(trial)))
        case_results.cache_clear()
        if good:
            return seed, err, gap, again
    return None


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["recreated"]:
        for B, T, C, W, K, nbest in RECREATED_SHAPES:
            case = ("continuous", 0, B, T, C, W, K, nbest, None, 0.0)
            print(case, "->", find_seed(case, recreated=True), flush=True)
    elif sys.argv[1:] == ["constrained"]:
        for case in (CONSTRAINED_CASE, NAN_TABLE_CASE):
            print(case, "->", find_seed(case, constrained=True), flush=True)
    else:
        for case in ALL_GPU_CASES:
            print(case, "->", find_seed(case, recreated=case in RECREATED_CASES,
                                        constrained=case in (CONSTRAINED_CASE, NAN_TABLE_CASE)), flush=True)
