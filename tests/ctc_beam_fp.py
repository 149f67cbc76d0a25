"""The yardstick of the CTC prefix beam search tests: the recursion of DESIGN section 20 in numpy, parameterised by the
float type and by how log-add is spelled.

  token set   S_t = the K best labels of row t (value descending, of equal values the smaller label; NaN and -inf are
              never chosen) plus `blank` if its entry is above -inf and not there already
  log-add     b if a = -inf, a if b = -inf, else m + log1p(exp(n - m)), m the larger, n the smaller
  state       at most W distinct prefixes with (pb, pnb); the empty prefix with (0, -inf) to begin with
  frame       stay:       pb' = tot + x[blank] (blank in S_t), pnb' = pnb + x[last] (last in S_t, pnb > -inf)
              extension:  c in S_t, c != blank: s = (pb if c == last else tot) + x[c], skipped when that base is -inf;
                          it is the prefix of a beam j of the current list: pnb'_j = logadd(pnb'_j, s), no candidate
              order:      total descending, stays before extensions, parent's rank ascending, label ascending; the
                          first W whose total is above -inf
  result      the first nbest of the final list: tokens, length, total; nothing where no candidate is left or T = 0

Three host forms: float64, float32, and float32 with m + log(1 + exp(n - m)) in place of log1p.  `vet` says whether a
continuous case can be compared with == on tokens: the three forms agree on every compared hypothesis and the float64
totals of neighbours (the one past the cut included) are at least 64 err apart, err the largest distance of either
float32 form's scores from float64 on that case.

tests/test_ctc_beam_cpu.py pins the float64 form to a brute-force enumeration and to the oracle's forwardScore;
tests/test_ctc_beam_gpu.py judges the kernels by it.
"""
import functools

import numpy as np

FORMS = ("f64", "f32", "f32log")
GAP_FACTOR = 64.0   # neighbours at least this many err apart (vet)
SCORE_FACTOR = 8.0  # the device's scores within this many err of float64 (test_ctc_beam_gpu.py)


def _ft(form):
    return np.float64 if form == "f64" else np.float32


def logadd(a, b, form="f64"):
    """element-wise log-add of two arrays of the form's float type"""
    ft = _ft(form)
    a, b = np.asarray(a, ft), np.asarray(b, ft)
    m, n = np.maximum(a, b), np.minimum(a, b)
    both = n > -np.inf
    d = np.where(both, n - np.where(both, m, ft(0)), ft(0)).astype(ft)
    with np.errstate(all="ignore"):
        tail = np.log(ft(1) + np.exp(d)) if form == "f32log" else np.log1p(np.exp(d))
    return np.where(both, m + tail.astype(ft), m).astype(ft)


def token_set(row, K, blank):
    """(labels, values) of S_t, in the order the K best are chosen, blank last where it is appended"""
    x = np.asarray(row, np.float32)
    v = np.where(np.isnan(x), np.float32(-np.inf), x)
    order = np.argsort(-v, kind="stable")[:K]  # (stable: of equal values the smaller label first)
    order = order[v[order] > -np.inf]
    if blank not in order and v[blank] > -np.inf:
        order = np.append(order, blank)
    return order.astype(np.int64), x[order]


def beam_search(em, blank, W, K, form="f64", frames=None, fresh_nodes=False):
    """em [M, C] -> the final list [(tokens tuple, total)] (at most W entries, in order), the form's arithmetic.
    fresh_nodes=True is NOT the contract: it numbers every kept extension anew and knows a prefix by that number alone,
    so a prefix that left the list and is created again is no longer recognised as the parent of its child that stayed
    (duplicate prefixes, split mass).  It exists to find and to certify the RECREATED_CASES below."""
    ft = _ft(form)
    em = np.asarray(em, np.float32)
    T = em.shape[0] if frames is None else int(frames)
    if T == 0:
        return []
    NEG = ft(-np.inf)
    # the trie: node -> (parent, label); node 0 is the empty prefix
    parent, label, child = [-1], [-1], {}
    node = np.array([0])
    pb, pnb = np.array([0.0], ft), np.array([NEG], ft)
    for t in range(T):
        n = len(node)
        if n == 0:
            break
        sl, sv = token_set(em[t], K, blank)
        sv = sv.astype(ft)
        xs = dict(zip(sl.tolist(), sv.tolist()))
        last = np.array([label[v] for v in node])
        tot = logadd(pb, pnb, form)
        xb = ft(xs[blank]) if blank in xs else NEG
        with np.errstate(invalid="ignore"):
            spb = (tot + xb).astype(ft) if blank in xs else np.full(n, NEG, ft)
            xl = np.array([xs.get(int(c), -np.inf) for c in last], ft)
            spnb = np.where((pnb > -np.inf) & (xl > -np.inf), pnb + xl, NEG).astype(ft)
            ext = sl != blank
            el, ev = sl[ext], sv[ext]
            base = np.where(el[None, :] == last[:, None], pb[:, None], tot[:, None]).astype(ft)
            s = (base + ev[None, :]).astype(ft)
        ok = base > -np.inf
        rank_of = {int(v): i for i, v in enumerate(node)}
        col_of = {int(c): k for k, c in enumerate(el)}
        for j in range(n):  # an extension that is a beam of the list already joins that beam
            i, k = rank_of.get(parent[node[j]]), col_of.get(int(last[j]))
            if i is not None and k is not None and ok[i, k]:
                spnb[j] = logadd(spnb[j], s[i, k], form)
                ok[i, k] = False
        stot = logadd(spb, spnb, form)
        ei, ek = np.nonzero(ok)
        total = np.concatenate([stot, s[ei, ek]])
        kind = np.concatenate([np.zeros(n, np.int64), np.ones(len(ei), np.int64)])
        rank = np.concatenate([np.arange(n), ei])
        lab = np.concatenate([np.full(n, -1), el[ek]])
        keep = total > -np.inf
        total, kind, rank, lab = total[keep], kind[keep], rank[keep], lab[keep]
        order = np.lexsort((lab, rank, kind, -total))[:W]
        new_node, new_pb, new_pnb = [], [], []
        for o in order:
            i = int(rank[o])
            if kind[o] == 0:
                new_node.append(int(node[i]))
                new_pb.append(spb[i])
                new_pnb.append(spnb[i])
            else:
                key = (int(node[i]), int(lab[o]))
                if fresh_nodes or key not in child:
                    child[key] = len(parent)
                    parent.append(key[0])
                    label.append(key[1])
                new_node.append(child[key])
                new_pb.append(NEG)
                new_pnb.append(total[o])
        node, pb, pnb = np.array(new_node, np.int64), np.array(new_pb, ft), np.array(new_pnb, ft)
    out = []
    tot = logadd(pb, pnb, form) if len(node) else []
    for v, sc in zip(node, tot):
        toks = []
        while v > 0:
            toks.append(label[v])
            v = parent[v]
        out.append((tuple(reversed(toks)), sc))
    return out


def decode_batch(em, frames, blank, W, K, nbest, form="f64"):
    """em [B, M, C] -> (tokens int32 [B, nbest, M], lengths int32 [B, nbest], scores [B, nbest] of the form's type):
    what the engine's call writes"""
    B, M, _ = em.shape
    tokens = np.full((B, nbest, M), -1, np.int32)
    lengths = np.zeros((B, nbest), np.int32)
    scores = np.full((B, nbest), -np.inf, _ft(form))
    for b in range(B):
        hyp = beam_search(em[b], blank, W, K, form, None if frames is None else frames[b])
        for r, (toks, sc) in enumerate(hyp[:nbest]):
            tokens[b, r, :len(toks)] = toks
            lengths[b, r] = len(toks)
            scores[b, r] = sc
    return tokens, lengths, scores


# ---- the case generators ----
def continuous_case(seed, B, T, C):
    """log-softmax of seeded normals (float32)"""
    x = np.random.default_rng(seed).normal(0.0, 2.0, (B, T, C))
    x = x - x.max(axis=2, keepdims=True)
    return (x - np.log(np.exp(x).sum(axis=2, keepdims=True))).astype(np.float32)


def holes_case(seed, B, T, C, p=0.3):
    """a continuous case with -inf entries at random places (never a whole row)"""
    rng = np.random.default_rng(seed + 5000)
    em = continuous_case(seed, B, T, C).copy()
    holes = rng.random((B, T, C)) < p
    holes[np.arange(B)[:, None], np.arange(T)[None, :], rng.integers(0, C, (B, T))] = False
    em[holes] = -np.inf
    return em


def dead_case(seed, B, T, C):
    """a holes case with a few NaN entries as well, and one all--inf row in the middle of utterance 1"""
    rng = np.random.default_rng(seed + 7000)
    em = holes_case(seed, B, T, C)
    nan = (rng.random((B, T, C)) < 0.1) & np.isneginf(em)
    em[nan] = np.nan
    em[1, T // 2] = -np.inf
    return em


def integer_case(seed, B, T, C, lo=-3, hi=1):
    """integer-valued scores: exact ties in the top-K choice"""
    return np.random.default_rng(seed + 9000).integers(lo, hi, (B, T, C)).astype(np.float32)


# ---- vetting ----
@functools.lru_cache(maxsize=None)
def case_results(kind, seed, B, T, C, blank, W, K, frames=None):
    """(em, {form: [final list per utterance]}) of a generated case, computed once per process and left unchanged"""
    em = {"continuous": continuous_case, "holes": holes_case, "dead": dead_case}[kind](seed, B, T, C)
    em.setflags(write=False)
    res = {f: [beam_search(em[b], blank, W, K, f, None if frames is None else frames[b]) for b in range(B)]
           for f in FORMS}
    return em, res


def results_of(case):
    """case_results of an entry of the case lists below (its nbest is not part of the computation)"""
    kind, seed, B, T, C, blank, W, K, _, frames = case
    return case_results(kind, seed, B, T, C, blank, W, K, frames)


def case_err(res, ncmp):
    """the largest distance of either float32 form's scores from float64 over the compared hypotheses"""
    err = 0.0
    for f in ("f32", "f32log"):
        for h64, h in zip(res["f64"], res[f]):
            for (_, a), (_, b) in zip(h64[:ncmp], h[:ncmp]):
                err = max(err, abs(float(a) - float(b)))
    return err


def vet(res, ncmp):
    """the rule of the module docstring over the first `ncmp` hypotheses of every utterance: (ok, err, smallest gap)"""
    err = case_err(res, ncmp)
    gap = np.inf
    for b, h64 in enumerate(res["f64"]):
        for f in ("f32", "f32log"):
            h = res[f][b]
            if len(h) != len(h64) or [p for p, _ in h[:ncmp]] != [p for p, _ in h64[:ncmp]]:
                return False, err, 0.0
        sc = [float(s) for _, s in h64[:ncmp + 1]]  # (the pair at the cut to the next one included)
        for a, c in zip(sc, sc[1:]):
            gap = min(gap, a - c)
    return bool(gap >= GAP_FACTOR * err), err, gap


# The cases test_ctc_beam_gpu.py runs: (kind, seed, B, T, C, blank, W, K, nbest, frames).  Seeds found by host search
# with `python tests/ctc_beam_fp.py` (the first that vets and, where a log-add is involved, has err > 0);
# test_ctc_beam_cpu.py asserts that every one vets.  Continuous cases compare at most the first 4 hypotheses;
# nbest = W only at T <= 3.
SHAPE_CASES = [
    ("continuous", 1, 1, 1, 1, 0, 1, 1, 1, None),
    ("continuous", 1, 2, 1, 2, 0, 2, 2, 2, None),
    ("continuous", 1, 2, 2, 3, 0, 4, 3, 4, None),
    ("continuous", 1, 2, 3, 300, 299, 2, 1, 2, None),
    ("continuous", 1, 65, 3, 5, 0, 4, 3, 4, None),
    ("continuous", 1, 2, 63, 4, 0, 1, 4, 1, None),
    ("continuous", 1, 2, 64, 33, 32, 2, 32, 2, None),
    ("continuous", 1, 2, 65, 5, 0, 4, 3, 2, None),
    ("continuous", 7, 2, 129, 33, 0, 8, 4, 4, None),
    ("continuous", 1, 1, 128, 64, 0, 64, 32, 4, None),
    ("continuous", 2, 2, 40, 65, 7, 63, 32, 4, None),
    ("continuous", 1, 2, 33, 1000, 0, 16, 32, 4, None),
    ("continuous", 1, 2, 64, 256, 0, 32, 16, 2, None),
    ("continuous", 1, 2, 129, 257, 256, 16, 8, 1, None),
    ("continuous", 1, 3, 65, 29, 0, 16, 16, 4, None),
    ("continuous", 1, 2, 2, 3, 1, 64, 3, 4, None),
    ("continuous", 1, 2, 3, 2, 0, 16, 16, 1, None),
]
RAGGED_FRAMES = (40, 1, 0, 39, 33, 2, 40)  # T, T - 1, 1 and 0 among them
RAGGED_CASE = ("continuous", 1, 7, 40, 29, 0, 8, 6, 2, RAGGED_FRAMES)
RAGGED_ROWS_CASE = ("continuous", 1, 6, 40, 29, 0, 8, 6, 2, tuple(f for f in RAGGED_FRAMES if f > 0))
HOLES_CASE = ("dead", 1, 4, 33, 9, 0, 8, 4, 2, None)  # -inf and NaN entries; utterance 1 has an all--inf row
REPEAT_CASE = ("continuous", 1, 3, 65, 29, 28, 16, 8, 4, None)
UNPRUNED_CASES = [("continuous", 1, 2, 1, 2, 0, 64, 2, 2, None), ("continuous", 1, 2, 2, 3, 0, 64, 3, 4, None),
                  ("continuous", 1, 2, 3, 4, 0, 64, 4, 4, None), ("continuous", 1, 2, 3, 3, 2, 64, 3, 4, None)]
TORCH_CASES = [("continuous", 1, 4, 40, 12, 0, 16, 16, 1, None), ("continuous", 1, 3, 75, 29, 28, 8, 5, 3, (75, 0, 41)),
               ("continuous", 1, 66, 5, 9, 0, 4, 4, 2, None)]
# A prefix leaves the list while its child stays, and is created again later from its own parent: the child must still
# be recognised as that prefix plus a label (exact identity, not the number a node happened to get).  Seeds found by
# host search: they vet, and beam_search(fresh_nodes=True) -- identity by node number -- gets their compared
# hypotheses wrong (test_ctc_beam_cpu.py asserts both).
RECREATED_CASES = [("continuous", 9, 2, 40, 4, 0, 4, 4, 2, None), ("continuous", 18, 2, 100, 5, 0, 8, 5, 2, None),
                   ("continuous", 6, 2, 65, 3, 0, 4, 3, 4, None), ("continuous", 6, 2, 129, 6, 0, 16, 6, 2, None),
                   ("continuous", 13, 1, 40, 4, 0, 4, 4, 1, None)]
ALL_GPU_CASES = (SHAPE_CASES + [RAGGED_CASE, RAGGED_ROWS_CASE, HOLES_CASE, REPEAT_CASE] + UNPRUNED_CASES
                 + TORCH_CASES + RECREATED_CASES)


def find_seed(case, tries=400):
    kind, _, B, T, C, blank, W, K, nbest, frames = case
    for seed in range(1, tries):
        _, res = case_results(kind, seed, B, T, C, blank, W, K, frames)
        ok, err, gap = vet(res, nbest)
        case_results.cache_clear()
        if ok and (err > 0 or T == 1):
            return seed, err, gap
    return None


if __name__ == "__main__":
    for case in ALL_GPU_CASES:
        print(case, "->", find_seed(case), flush=True)
