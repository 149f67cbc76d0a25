"""The yardstick of the CTC prefix beam search with a bigram table fused in: the recursion of
tests/ctc_beam_fp.py with a language model score L per prefix, in numpy, in the same three float forms.

  table       w [C + C*C] float32 in the arc order of asgTransitions: w[c] scores c as first label, w[C + i*C + j] label
              j followed by label i
  L           L(()) = 0; L(y + c) = L(y) + inc, inc = alpha * w(last(y) -> c) + beta (a product rounded, then a sum
              rounded), all in the form's float type
  ranking     a stay by logadd(pb', pnb') + L(y), an extension by s + (L(y) + inc), s as in ctc_beam_fp; the same order;
              a candidate whose acoustic total is -inf is dropped, and so is an extension whose inc is not finite
  the rest    the token sets, (pb, pnb) and the merge of an extension into a beam of the list are purely acoustic
  result      the first nbest of the final list: (tokens, acoustic total + L, acoustic total)

`stats["recreated"]` counts the kept extensions that re-create a prefix which is in the trie but not in the current list
(an extension that spells a beam of the list is merged and is no candidate, so every kept extension whose trie node
exists already is one): such a prefix must get its L again bit for bit.

tests/test_ctc_beam_lm_cpu.py pins the float64 form to a brute-force enumeration and to ctc_beam_fp.beam_search at
alpha = beta = 0; tests/test_ctc_beam_lm_gpu.py judges the kernel by it.  `vet` is ctc_beam_fp.vet over the combined
totals; err is taken over both score kinds.
"""
import functools

import numpy as np

import ctc_beam_fp as fp
from ctc_beam_fp import GAP_FACTOR, SCORE_FACTOR, case_err, logadd, token_set, vet  # noqa: F401  (the shared rules)

ALPHA, BETA = 0.8, 0.5  # of the generated cases


def beam_search_lm(em, blank, W, K, w, alpha, beta, form="f64", frames=None, stats=None):
    """em [M, C], w [C + C*C] -> the final list [(tokens tuple, total, am_total)] (at most W entries, in order), the
    form's arithmetic"""
    ft = fp._ft(form)
    em = np.asarray(em, np.float32)
    C = em.shape[1]
    w = np.asarray(w, np.float32).astype(ft)
    alpha, beta = ft(np.float32(alpha)), ft(np.float32(beta))
    T = em.shape[0] if frames is None else int(frames)
    if T == 0:
        return []
    NEG = ft(-np.inf)
    parent, label, child, lm = [-1], [-1], {}, [ft(0)]  # the trie: node -> (parent, label, L); node 0 the empty prefix
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
        L = np.array([lm[v] for v in node], ft)
        tot = logadd(pb, pnb, form)
        xb = ft(xs[blank]) if blank in xs else NEG
        with np.errstate(all="ignore"):
            spb = (tot + xb).astype(ft) if blank in xs else np.full(n, NEG, ft)
            xl = np.array([xs.get(int(c), -np.inf) for c in last], ft)
            spnb = np.where((pnb > -np.inf) & (xl > -np.inf), pnb + xl, NEG).astype(ft)
            ext = sl != blank
            el, ev = sl[ext], sv[ext]
            base = np.where(el[None, :] == last[:, None], pb[:, None], tot[:, None]).astype(ft)
            s = (base + ev[None, :]).astype(ft)
            # the table entry of (beam, label): the start score for the empty prefix
            at = np.where(last[:, None] < 0, el[None, :], C + el[None, :] * C + np.maximum(last[:, None], 0))
            inc = ((alpha * w[at]).astype(ft) + beta).astype(ft).reshape(n, len(el))
            Lnew = (L[:, None] + inc).astype(ft)
            stotal = (s + Lnew).astype(ft)
        ok = base > -np.inf
        rank_of = {int(v): i for i, v in enumerate(node)}
        col_of = {int(c): k for k, c in enumerate(el)}
        for j in range(n):  # an extension that is a beam of the list already joins that beam: acoustic mass only
            i, k = rank_of.get(parent[node[j]]), col_of.get(int(last[j]))
            if i is not None and k is not None and ok[i, k]:
                spnb[j] = logadd(spnb[j], s[i, k], form)
                ok[i, k] = False
        stot = logadd(spb, spnb, form)
        ok &= np.isfinite(inc)
        ei, ek = np.nonzero(ok)
        with np.errstate(all="ignore"):
            total = np.concatenate([(stot + L).astype(ft), stotal[ei, ek]])
        am = np.concatenate([stot, s[ei, ek]])
        kind = np.concatenate([np.zeros(n, np.int64), np.ones(len(ei), np.int64)])
        rank = np.concatenate([np.arange(n), ei])
        lab = np.concatenate([np.full(n, -1), el[ek]])
        newL = np.concatenate([L, Lnew[ei, ek]])
        keep = am > -np.inf
        total, am, kind, rank, lab, newL = total[keep], am[keep], kind[keep], rank[keep], lab[keep], newL[keep]
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
                if key in child:
                    if stats is not None:
                        stats["recreated"] = stats.get("recreated", 0) + 1
                    assert lm[child[key]].tobytes() == newL[o].tobytes()  # (the same operands in the same order)
                else:
                    child[key] = len(parent)
                    parent.append(key[0])
                    label.append(key[1])
                    lm.append(newL[o])
                new_node.append(child[key])
                new_pb.append(NEG)
                new_pnb.append(am[o])
        node, pb, pnb = np.array(new_node, np.int64), np.array(new_pb, ft), np.array(new_pnb, ft)
    out = []
    tot = logadd(pb, pnb, form) if len(node) else []
    for v, sc in zip(node, tot):
        toks, u = [], v
        while u > 0:
            toks.append(label[u])
            u = parent[u]
        out.append((tuple(reversed(toks)), ft(sc + lm[v]), sc))
    return out


def decode_batch_lm(em, frames, blank, W, K, nbest, w, alpha, beta, form="f64"):
    """em [B, M, C] -> (tokens int32 [B, nbest, M], lengths int32 [B, nbest], scores, am_scores [B, nbest] of the form's
    type): what the engine's call writes"""
    B, M, _ = em.shape
    tokens = np.full((B, nbest, M), -1, np.int32)
    lengths = np.zeros((B, nbest), np.int32)
    scores = np.full((B, nbest), -np.inf, fp._ft(form))
    am_scores = np.full((B, nbest), -np.inf, fp._ft(form))
    for b in range(B):
        hyp = beam_search_lm(em[b], blank, W, K, w, alpha, beta, form, None if frames is None else frames[b])
        for r, (toks, sc, am) in enumerate(hyp[:nbest]):
            tokens[b, r, :len(toks)] = toks
            lengths[b, r] = len(toks)
            scores[b, r] = sc
            am_scores[b, r] = am
    return tokens, lengths, scores, am_scores


# ---- the case generators ----
def table_case(seed, C, holes=0.0):
    """seeded normal(0, 2) table; with `holes` that share of its entries -inf (a seeded choice)"""
    w = np.random.default_rng(seed + 11000).normal(0, 2, C + C * C).astype(np.float32)
    if holes:
        w[np.random.default_rng(seed + 13000).random(C + C * C) < holes] = -np.inf
    return w


@functools.lru_cache(maxsize=None)
def case_results(seed, B, T, C, blank, W, K, frames=None, holes=0.0):
    """(em, w, {form: [final list per utterance]}, re-creations in the float64 form) of a generated case, computed once
    per process and left unchanged"""
    em = fp.continuous_case(seed, B, T, C)
    w = table_case(seed, C, holes)
    em.setflags(write=False)
    w.setflags(write=False)
    stats = {}
    res = {f: [beam_search_lm(em[b], blank, W, K, w, ALPHA, BETA, f, None if frames is None else frames[b],
                              stats if f == "f64" else None) for b in range(B)] for f in fp.FORMS}
    return em, w, res, stats.get("recreated", 0)


def results_of(case):
    """case_results of an entry of the case lists below (its nbest is not part of the computation)"""
    seed, B, T, C, blank, W, K, _, frames, holes = case
    return case_results(seed, B, T, C, blank, W, K, frames, holes)


def split(res):
    """the results as ctc_beam_fp's vet and case_err read them: (by combined total, by acoustic total)"""
    return ({f: [[(y, s) for y, s, _ in h] for h in hs] for f, hs in res.items()},
            {f: [[(y, a) for y, _, a in h] for h in hs] for f, hs in res.items()})


def case_err_lm(res, ncmp):
    """the largest distance of either float32 form's scores from float64 over the compared hypotheses, both score kinds"""
    both, am = split(res)
    return max(case_err(both, ncmp), case_err(am, ncmp))


def vet_lm(res, ncmp):
    """ctc_beam_fp's rule over the combined totals (the ranking), with err over both score kinds: (ok, err, gap)"""
    both, _ = split(res)
    ok, _, gap = vet(both, ncmp)
    err = case_err_lm(res, ncmp)
    return bool(ok and gap >= GAP_FACTOR * err), err, gap


# The cases test_ctc_beam_lm_gpu.py runs: (seed, B, T, C, blank, W, K, nbest, frames, holes).  Seeds found by host search
# with `python tests/ctc_beam_lm_fp.py` (the first that vets with err > 0); test_ctc_beam_lm_cpu.py asserts that every one
# vets.
SHAPE_CASES = [
    (2, 2, 65, 5, 0, 4, 3, 2, None, 0.0),
    (1, 2, 64, 33, 32, 2, 32, 2, None, 0.0),
    (1, 1, 128, 64, 0, 64, 32, 4, None, 0.0),
    (1, 2, 40, 65, 7, 63, 32, 4, None, 0.0),
    (1, 2, 33, 300, 299, 16, 32, 4, None, 0.0),
    (1, 3, 65, 29, 0, 16, 16, 4, None, 0.0),
    (2, 2, 129, 257, 256, 16, 8, 1, None, 0.0),
    (1, 65, 3, 5, 0, 4, 3, 4, None, 0.0),
]
RAGGED_FRAMES = fp.RAGGED_FRAMES
RAGGED_CASE = (1, 7, 40, 29, 0, 8, 6, 2, RAGGED_FRAMES, 0.0)
RAGGED_ROWS_CASE = (1, 6, 40, 29, 0, 8, 6, 2, tuple(f for f in RAGGED_FRAMES if f > 0), 0.0)
CONSTRAINED_CASE = (1, 3, 40, 12, 0, 16, 8, 4, None, 0.2)  # 15-30 % of the table -inf
# a prefix leaves the list and is created again: its L must be the same bits (re-creation count > 0)
RECREATED_CASES = [(2, 2, 40, 4, 0, 4, 4, 2, None, 0.0), (1, 2, 100, 5, 0, 8, 5, 2, None, 0.0)]
UNPRUNED_CASES = [(1, 2, 1, 2, 0, 64, 2, 2, None, 0.0), (1, 2, 2, 3, 0, 64, 3, 4, None, 0.0),
                  (1, 2, 3, 4, 0, 64, 4, 4, None, 0.0), (1, 2, 3, 3, 2, 64, 3, 4, None, 0.0)]
TORCH_CASE = (1, 3, 40, 12, 0, 16, 8, 2, None, 0.0)
ALL_GPU_CASES = (SHAPE_CASES + [RAGGED_CASE, RAGGED_ROWS_CASE, CONSTRAINED_CASE] + RECREATED_CASES + UNPRUNED_CASES
                 + [TORCH_CASE])


def find_seed(case, tries=400, recreated=False):
    _, B, T, C, blank, W, K, nbest, frames, holes = case
    for seed in range(1, tries):
        _, _, res, again = case_results(seed, B, T, C, blank, W, K, frames, holes)
        ok, err, gap = vet_lm(res, nbest)
        case_results.cache_clear()
        if ok and (err > 0 or T == 1) and (again > 0 or not recreated):
            return seed, err, gap, again
    return None


if __name__ == "__main__":
    for case in ALL_GPU_CASES:
        print(case, "->", find_seed(case, recreated=case in RECREATED_CASES), flush=True)
