"""compose / intersect in every cell of op_compose_impl's dispatch (gtn_amd/csrc/ops_compose.cpp): the case table of
tests/test_compose_cells_cpu.py and tests/test_compose_cells_gpu.py, and a Python restatement of the dispatch.

A case is one call (or, for "calls", several) of gtn.compose / gtn.intersect on a list of pairs.  An operand is a dict
graph in tests/graphgen.py's format, or {"chain": (T, C), "w": float32[T*C]} for gtn.linear_graph(T, C).  Everything is
built from SEED and the case's name.

predict() restates
  * the HOST rules of op_compose_impl: wide_pref, pairs_pref, `wide` (512 lanes), the budget arithmetic of the classic
    and the chain-window bitmaps, g1's LDS cache, skip, defer (max_deg <= 4, A <= 768 / 1536, full window),
    inline_rep_for, and where a handed-back product goes; and
  * the DEVICE rules that are functions of the shape, by walking the product the way the kernels do (sim_chain,
    sim_pairs): the FAST variant hands back on a frontier pair with more than KC candidates (phase B: in-lists, phase F:
    out-lists), on a 256 / 512-node chunk of a level with more arcs than 3/4 of the claim hash, and on a chain window
    that runs out of slices before the co-reachable sets become stationary (chs >= Wmax); the in-rows are built in the
    kernel while the product is layered, no level brings more than WC new nodes and (general variant) every chunk
    took the LDS path -- otherwise the transpose passes build them.
expected_routes(name) is predict() of the case: the exact delta of gtn.debug_compose_routes() the case must produce.
The table also STATES, per case, the product sizes and the cells the case was designed for; the CPU tests hold the
model and the oracle to those statements."""
import functools
import zlib

import numpy as np

import graphgen as gg

SEED = 20261021
KC = 4                      # compose.hip: candidates a lane caches
WIDE_NODE_CAP = 2048        # compose_wide.hip: NO_CAP
MAX_BITMAP = 2 * 26624      # compose.hip: kMaxBitmapBytes
EPS = gg.EPS

CELLS = ["fast256", "fast512", "general/lds", "general/hbm", "wide_chain", "pairs",
         "redo/fast->wide_chain", "redo/fast->pairs", "redo/fast->general", "redo/wide_chain->general",
         "bitmap/classic", "bitmap/window_full", "bitmap/window_partial",
         "sizes/deferred", "sizes/read", "arrays/skipped", "arrays/full", "replicate/inline", "replicate/grid",
         "g1_cache/on", "g1_cache/off", "transpose", "layered", "not_layered", "symbolic"]
# compose_wide.hip's plan kernel hands back (overflow = 2) only for a partner of more than NO_CAP nodes, none at all, or
# an empty chain -- exactly what the host's wide_ok already excludes (ex.N in 1..compose_wide_node_cap(), M >= 1).  So
# the host's wide -> general re-run cannot be reached from any input; the counter exists, no case can name it.
UNREACHABLE = {"redo/wide_chain->general"}


def lds_budget(blk):
    """compose_lds_budget(): dynamic bytes that keep two workgroups per CU"""
    return 80 * 1024 - (38 if blk == 512 else 19) * 1024


def bitmap_budget(blk):
    return min(MAX_BITMAP, lds_budget(blk))


def g1_cache_bytes(N1, A1):
    return 16 + 4 * ((N1 + 1 + 3) & ~3) + 16 * A1 + ((N1 + 15) & ~15)


# ---------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------
def rng_of(name):
    return np.random.default_rng([SEED, zlib.crc32(name.encode())])


def chain(T, C, rng):
    return {"chain": (T, C), "w": rng.normal(0, 1, T * C).astype(np.float32)}


def is_chain(g):
    return "chain" in g


def graph(start, accept, arcs, rng, sort=None):
    """arcs: (src, dst, ilabel, olabel); weights N(0, 1) in float32"""
    arcs = list(arcs)
    return {"start": [int(x) for x in start], "accept": [int(x) for x in accept],
            "src": [int(a[0]) for a in arcs], "dst": [int(a[1]) for a in arcs], "il": [int(a[2]) for a in arcs],
            "ol": [int(a[3]) for a in arcs], "w": gg._f32(rng.normal(0, 1, len(arcs))), "sort": sort}


def acceptor(start, accept, arcs, rng, sort=None):
    return graph(start, accept, [(s, d, l, l) for s, d, l in arcs], rng, sort)


class Facts:
    """what the host and the kernels read of an operand"""

    def __init__(self, g):
        self.lin = is_chain(g)
        if self.lin:
            self.M, self.C = g["chain"]
            self.N, self.A = self.M + 1, self.M * self.C
            self.il_sorted = self.ol_sorted = True
            self.eps_free = self.acceptor = True
            self.device = False
            return
        self.device = "product" in g           # the result of an earlier compose: not resident on the host
        if self.device:
            # node ids, arc ids and arc order are the reference's; a product is sorted on nothing, and its flags are
            # its operands' (ops_compose.cpp: v.flags), whatever its arcs turned out to be
            a, b, mode = g["product"]
            inherited = Facts(a), Facts(b)
            g = to_oracle(g).to_dict()
        self.N, self.A = len(g["start"]), len(g["src"])
        self.src, self.dst = np.asarray(g["src"], np.int64), np.asarray(g["dst"], np.int64)
        self.il, self.ol = np.asarray(g["il"], np.int64), np.asarray(g["ol"], np.int64)
        self.il_sorted, self.ol_sorted = g.get("sort") == "i", g.get("sort") == "o"
        self.eps_free = not ((self.il == EPS).any() or (self.ol == EPS).any())
        self.acceptor = bool((self.il == self.ol).all())
        if self.device:
            self.eps_free = inherited[0].eps_free and inherited[1].eps_free
            self.acceptor = inherited[0].acceptor and inherited[1].acceptor
        self.starts = [n for n in range(self.N) if g["start"][n]]
        self.accepts = [n for n in range(self.N) if g["accept"][n]]
        self.is_start = np.asarray(g["start"], bool)
        self.is_accept = np.asarray(g["accept"], bool)
        key = self.il if self.il_sorted else (self.ol if self.ol_sorted else None)
        order = np.arange(self.A) if key is None else np.argsort(key, kind="stable")
        self.out = [[] for _ in range(self.N)]   # arc ids in list order (arcSort reorders the lists, not the ids)
        self.inn = [[] for _ in range(self.N)]
        for a in order.tolist():
            self.out[self.src[a]].append(a)
            self.inn[self.dst[a]].append(a)
        self.max_deg = max([0] + [max(len(o), len(i)) for o, i in zip(self.out, self.inn)])


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' walk, in Python: what the device decides
# ---------------------------------------------------------------------------------------------------------------------
class Walk:
    """N, A: product sizes; handback: why the FAST variant would give the pair back (None: it finishes);
    layered; new_max: most new nodes one level brings; chunks_fast[blk]: every blk-node chunk took the LDS path;
    pairs / arcs: the product's node pairs and (src, dst, arc of g1, arc of g2) in the reference's order"""


def sim_chain(ex, T, C, chain_first, slices, blks=(256, 512)):
    """chain product with an epsilon-free partner `ex` (compose.hip's time-layered view: B[t] co-reachable partner
    nodes, S[t] the ordered frontier).  slices: ComposeArgs::chain_bits (0: classic bitmaps, no window rule)."""
    lab = ex.il if chain_first else ex.ol      # the chain's olabel / ilabel meets this label of the partner
    match = (lab >= 0) & (lab < C)
    msrc, mdst = ex.src[match], ex.dst[match]
    indeg = np.bincount(mdst, minlength=ex.N)
    w = Walk()
    w.handback = None
    # ---- phase B
    w.stationary = False
    rows = [None] * (T + 1)
    cur = ex.is_accept.copy() if T > 0 else np.zeros(ex.N, bool)   # (linear_graph(0, C) has no accept node)
    rows[T] = cur
    tau = T
    while tau >= 1 and cur.any():
        if (indeg[cur] > KC).any():
            w.handback = w.handback or "B: in-degree > KC"
        prev = np.zeros(ex.N, bool)
        prev[msrc[cur[mdst]]] = True
        if slices > 0 and prev.any() and T - (tau - 1) >= slices:
            w.handback = w.handback or "B: chs >= Wmax"
        rows[tau - 1] = prev
        if (prev == cur).all():   # B[tau-1] == B[tau]: every earlier time shares it
            for t in range(tau - 1):
                rows[t] = prev
            w.stationary = True
            break
        cur = prev
        tau -= 1
    for t in range(T + 1):
        if rows[t] is None:
            rows[t] = np.zeros(ex.N, bool)
    # ---- phase F
    S = [n for n in ex.starts if rows[0][n]]
    w.N, w.A, w.new_max = len(S), 0, 0
    w.width_max, w.level_arcs_max = len(S), 0
    w.chunks_fast = {b: True for b in blks}
    w.kc_f = False
    memo = {}
    out_m = [[(a, int(ex.dst[a])) for a in ex.out[n] if match[a]] for n in range(ex.N)]
    t = 0
    while S and t < T:
        key = (tuple(S), rows[t + 1].tobytes())
        if key not in memo:
            B = rows[t + 1]
            seen, nxt, per_node, wide_node = set(), [], [], []
            for n in S:
                k = 0
                for _, d in out_m[n]:
                    if B[d]:
                        k += 1
                        if d not in seen:
                            seen.add(d)
                            nxt.append(d)
                per_node.append(k)
                wide_node.append(len(out_m[n]) > KC)
            fast = {}
            for b in blks:
                fast[b] = all(sum(per_node[c:c + b]) <= 3 * b and not any(wide_node[c:c + b]) for c in range(0, len(S), b))
            memo[key] = (nxt, sum(per_node), fast, any(wide_node))
        nxt, arcs, fast, kc = memo[key]
        for b in blks:
            w.chunks_fast[b] = w.chunks_fast[b] and fast[b]
        w.kc_f = w.kc_f or kc
        w.A += arcs
        w.N += len(nxt)
        w.new_max = max(w.new_max, len(nxt))
        w.width_max = max(w.width_max, len(nxt))
        w.level_arcs_max = max(w.level_arcs_max, arcs)
        S = nxt
        t += 1
    w.layered = True
    return w


def _by_label(f, lists, lab):
    out = []
    for n in range(f.N):
        d = {}
        for a in lists[n]:
            d.setdefault(int(lab[a]), []).append(a)
        out.append(d)
    return out


def explicit_of_chain(g):
    T, C = g["chain"]
    d = gg.linear(T, C, g["w"])
    d["sort"] = "i"
    f = Facts(d)
    f.il_sorted = f.ol_sorted = True
    return f


def sim_pairs(f1, f2, intersect, blks=(256, 512)):
    """two explicit graphs, gtn/functions/compose.cpp:377-522 as compose.hip walks it: the co-reachable pairs
    backwards, then the breadth-first numbering with the matcher's arc order"""
    N1 = f1.N
    w = Walk()
    w.handback = None
    w.chunks_fast = {b: True for b in blks}
    w.pairs, w.arcs = [], []
    w.N = w.A = w.new_max = w.width_max = w.level_arcs_max = 0
    w.layered = True
    w.kc_f = False
    if f1.N == 0 or f2.N == 0:
        return w
    c1 = (f1.il_sorted or f1.ol_sorted) if intersect else f1.ol_sorted
    c2 = (f2.il_sorted or f2.ol_sorted) if intersect else f2.il_sorted
    in1, in2 = _by_label(f1, f1.inn, f1.ol), _by_label(f2, f2.inn, f2.il)
    out1, out2 = _by_label(f1, f1.out, f1.ol), _by_label(f2, f2.out, f2.il)
    # ---- phase B
    reach = set()
    front = []
    for a1 in f1.accepts:
        for a2 in f2.accepts:
            reach.add(a1 + N1 * a2)
            front.append(a1 + N1 * a2)
    while front:
        nxt = []
        for idx in front:
            n1, n2 = idx % N1, idx // N1
            cands = []
            for l, xs in in1[n1].items():     # (eps:eps pairs are walked too: a superset is all phase B needs)
                ys = in2[n2].get(l)
                if ys:
                    cands += [int(f1.src[x]) + N1 * int(f2.src[y]) for x in xs for y in ys]
            cands += [int(f1.src[x]) + N1 * n2 for x in in1[n1].get(EPS, [])]
            cands += [n1 + N1 * int(f2.src[y]) for y in in2[n2].get(EPS, [])]
            if len(cands) > KC:
                w.handback = w.handback or "B: candidates > KC"
            for c in cands:
                if c not in reach:
                    reach.add(c)
                    nxt.append(c)
        front = nxt
    w.coreachable = len(reach)
    # ---- phase F
    ids = {}
    level = []
    for s1 in f1.starts:
        for s2 in f2.starts:
            idx = s1 + N1 * s2
            if idx in reach:
                ids[idx] = len(ids)
                level.append(idx)
    w.pairs = list(level)
    w.width_max = len(level)
    hi = len(level)
    while level:
        nxt, per_node, wide_node = [], [], []
        for idx in level:
            n1, n2 = idx % N1, idx // N1
            l1, l2 = f1.out[n1], f2.out[n2]
            cand = []
            # matcher order: "for q in the query list: for s in the equal-label run of the search list"
            search_g1 = (c1 and not c2) or (c1 and c2 and len(l1) > len(l2))
            if search_g1:
                for y in l2:
                    l = int(f2.il[y])
                    if l != EPS:
                        cand += [(int(f1.dst[x]) + N1 * int(f2.dst[y]), x, y) for x in out1[n1].get(l, [])]
            else:
                for x in l1:
                    l = int(f1.ol[x])
                    if l != EPS:
                        cand += [(int(f1.dst[x]) + N1 * int(f2.dst[y]), x, y) for y in out2[n2].get(l, [])]
            e1, e2 = out1[n1].get(EPS, []), out2[n2].get(EPS, [])
            em = bool(e1) and bool(e2)
            acc1, acc2 = bool(f1.is_accept[n1]), bool(f2.is_accept[n2])
            if not em or acc2 or not acc1:       # compose.cpp:461
                cand += [(int(f1.dst[x]) + N1 * n2, x, -1) for x in e1]
            if not em or acc1:                   # compose.cpp:476
                cand += [(n1 + N1 * int(f2.dst[y]), -1, y) for y in e2]
            k = 0
            for c, x, y in cand:
                if c in reach:
                    k += 1
                    if c not in ids:
                        ids[c] = len(ids)
                        nxt.append(c)
                        w.pairs.append(c)
                    if ids[c] < hi:
                        w.layered = False
                    w.arcs.append((ids[idx], ids[c], x, y))
            per_node.append(k)
            wide_node.append(len(cand) > KC)
        for b in blks:
            w.chunks_fast[b] = w.chunks_fast[b] and all(
                sum(per_node[c:c + b]) <= 3 * b and not any(wide_node[c:c + b]) for c in range(0, len(level), b))
        w.kc_f = w.kc_f or any(wide_node)
        w.level_arcs_max = max(w.level_arcs_max, sum(per_node))
        w.new_max = max(w.new_max, len(nxt))
        w.width_max = max(w.width_max, len(nxt))
        level = nxt
        hi = len(ids)
    w.N, w.A = len(ids), len(w.arcs)
    return w


def walk(a, b, intersect, slices):
    fa, fb = Facts(a), Facts(b)
    if fa.lin != fb.lin:
        ex, ch = (fb, fa) if fa.lin else (fa, fb)
        if ex.eps_free:
            return sim_chain(ex, ch.M, ch.C, fa.lin, slices)
        # (a partner with epsilons: no time-layered view, the classic walk on the chain written out)
        return sim_pairs(explicit_of_chain(a) if fa.lin else fa, explicit_of_chain(b) if fb.lin else fb, intersect)
    assert not fa.lin, "chain x chain is not a case of this table"
    return sim_pairs(fa, fb, intersect)


# ---------------------------------------------------------------------------------------------------------------------
# predict(): the host rules around the walk
# ---------------------------------------------------------------------------------------------------------------------
def predict(pairs, mode="compose", env=(), detail=None):
    """{cell: count} one call of compose / intersect on `pairs` (graphs built, gtn.compose_mode(0)) must add to
    gtn.debug_compose_routes().  env: the GTNX_* switches that are set.  detail (a list) receives one dict per pair."""
    env = set(env)
    intersect = mode == "intersect"
    n = len(pairs)
    F = [(Facts(a), Facts(b)) for a, b in pairs]
    chainp = [fa.lin != fb.lin for fa, fb in F]
    ex = [(fb if fa.lin else fa) for fa, fb in F]
    ch = [(fa if fa.lin else fb) for fa, fb in F]
    l1 = [fa.lin for fa, _ in F]
    wide_ok, wide_pref, pairs_ok, pairs_pref = ([False] * n for _ in range(4))
    for i, (fa, fb) in enumerate(F):
        if chainp[i] and "GTNX_NO_WIDE_COMPOSE" not in env:
            e = ex[i]
            claim = (e.il_sorted or e.ol_sorted) if intersect else (e.il_sorted if l1[i] else e.ol_sorted)
            on_match = (e.il_sorted if l1[i] else e.ol_sorted) or (e.acceptor and claim)
            wide_ok[i] = e.eps_free and ch[i].M >= 1 and 1 <= e.N <= WIDE_NODE_CAP and (not claim or on_match)
            wide_pref[i] = wide_ok[i] and (e.A > 4 * e.N or "GTNX_FORCE_WIDE_COMPOSE" in env)
        if not fa.lin and not fb.lin and not ({"GTNX_NO_WIDE_COMPOSE", "GTNX_NO_PAIRS_COMPOSE"} & env):
            c1 = (fa.il_sorted or fa.ol_sorted) if intersect else fa.ol_sorted
            c2 = (fb.il_sorted or fb.ol_sorted) if intersect else fb.il_sorted
            a1 = fa.acceptor and (fa.il_sorted or fa.ol_sorted)
            a2 = fb.acceptor and (fb.il_sorted or fb.ol_sorted)
            t1 = (fa.ol_sorted or a1) if c1 else True
            t2 = (fb.il_sorted or a2) if c2 else True
            pairs_ok[i] = t1 and t2
            pairs_pref[i] = pairs_ok[i] and (fa.A > 4 * fa.N or fb.A > 4 * fb.N or "GTNX_FORCE_WIDE_COMPOSE" in env)
    # 512 lanes: some chain product's partner has 257..512 nodes and none has more
    widths = [ex[i].N for i in range(n) if chainp[i]]
    wide = bool(widths) and max(widths) > 256 and max(widths) <= 512 and "GTNX_NARROW_COMPOSE" not in env
    blk = 512 if wide else 256
    budget = bitmap_budget(blk)
    classic_ok, slices, full_window = [False] * n, [0] * n, [False] * n
    fast_ok, fast_bm = True, 0
    for i, (fa, fb) in enumerate(F):
        classic = 2 * 4 * ((fa.N * fb.N + 31) // 32)
        classic_ok[i] = classic <= budget
        mine = classic
        if "GTNX_CLASSIC_BITMAPS" not in env and chainp[i] and ex[i].eps_free and 1 <= ex[i].N <= 1024:
            No, TM = ex[i].N, ch[i].M
            room = budget // (4 * ((No + 31) // 32)) - 3
            s = min(TM + 1, room)
            if s < TM + 1:
                s = min(No + 64, room)
            full_window[i] = s >= TM + 1
            if s >= min(TM + 1, 64):
                slices[i] = s
                mine = 4 * ((No + 31) // 32) * (s + 3)
        if wide_pref[i] or pairs_pref[i]:
            continue
        fast_ok = fast_ok and mine <= budget
        fast_bm = max(fast_bm, mine)
    g1c = max([0] + [g1_cache_bytes(fa.N, fa.A) for fa, _ in F if not fa.lin])
    cache1 = fast_ok and g1c > 0 and fast_bm + g1c <= lds_budget(blk)
    skip = [("GTNX_FULL_COMPOSE" not in env and fast_ok and not wide_pref[i] and chainp[i] and ex[i].eps_free and
             ex[i].N <= blk) for i in range(n)]
    defer = fast_ok and "GTNX_SYNC_COMPOSE" not in env and not any(wide_pref) and not any(pairs_pref)
    for i in range(n):
        if not defer:
            break
        defer = (chainp[i] and skip[i] and full_window[i] and slices[i] > 0 and not ex[i].device and
                 ex[i].max_deg <= 4 and ex[i].A <= (1536 if wide else 768) and ex[i].N >= 1 and ch[i].M >= 1)

    def inline_rep_for(m):
        if "GTNX_INLINE_REPLICATION" in env:
            return True
        if "GTNX_GRID_REPLICATION" in env:
            return False   # (the table only ever sets it to "1")
        return m > 128

    out = {}

    def hit(c):
        out[c] = out.get(c, 0) + 1

    n_all = sum(1 for i in range(n) if not wide_pref[i] and not pairs_pref[i])
    for i, (a, b) in enumerate(pairs):
        fa, fb = F[i]
        first = 2 if wide_pref[i] else 3 if pairs_pref[i] else (1 if fast_ok else 0)
        w = walk(a, b, intersect, slices[i] if first == 1 else 0)
        d = {"first": first, "walk": w, "slices": slices[i], "full_window": full_window[i], "skip": skip[i],
             "defer": defer, "wide": wide, "cache1": cache1, "classic_ok": classic_ok[i]}
        if detail is not None:
            detail.append(d)
        hit({0: "general/lds" if classic_ok[i] else "general/hbm", 1: "fast512" if wide else "fast256",
             2: "wide_chain", 3: "pairs"}[first])
        if first == 1 and chainp[i]:
            hit("bitmap/window_full" if slices[i] and full_window[i] else
                "bitmap/window_partial" if slices[i] else "bitmap/classic")
        last, m_last = first, n_all
        # the FAST variant's own reasons to give the pair back
        hb = None
        if first == 1:
            hb = w.handback or (None if w.chunks_fast[blk] else "F: a chunk off the LDS path")
        d["handback"] = hb
        if first == 1 and defer:
            assert hb is None, ("the host deferred the sizes of a product the FAST variant gives back", hb)
        if hb:
            if wide_ok[i] and not wide_pref[i]:
                hit("redo/fast->wide_chain")
                last = 2
            elif pairs_ok[i] and not pairs_pref[i] and (fa.A > 2 * fa.N or fb.A > 2 * fb.N):
                hit("redo/fast->pairs")
                last = 3
            else:
                hit("redo/fast->general")
                last = 0
        deferred = defer and first == 1
        hit("sizes/deferred" if deferred else "sizes/read")
        # (a pair with a node-less operand leaves at the top of the kernel: nothing skipped, nothing to transpose)
        hit("arrays/skipped" if (last == 1 and skip[i] and fa.N and fb.N) else "arrays/full")
        layered = True if last == 2 or deferred else w.layered
        hit("layered" if layered else "not_layered")
        if last in (2, 3):
            hit("transpose")       # compose_wide.hip never builds the in-rows
        elif not deferred and w.N >= 0:
            built = w.layered and w.new_max <= 2 * (blk if last == 1 else 256) and (last == 1 or w.chunks_fast[256])
            if not built:
                hit("transpose")
        if last == 1:
            hit("g1_cache/on" if cache1 else "g1_cache/off")
            if chainp[i]:
                hit("replicate/inline" if inline_rep_for(m_last) else "replicate/grid")
        d["last"] = last
    return out


# ---------------------------------------------------------------------------------------------------------------------
# partners
# ---------------------------------------------------------------------------------------------------------------------
def ctc_partner(U, C, rng):
    tg = rng.integers(1, C, U).tolist()
    for k in range(1, U):          # no repeats: every label arc of benchmarks/ctc.cpp's target is there
        if tg[k] == tg[k - 1]:
            tg[k] = 1 + tg[k] % (C - 1)
    d = gg.ctc_target_graph(tg)
    d["w"] = gg._f32(rng.normal(0, 1, len(d["src"])))
    return d


def strands(No, rng, extra=0, per_node=2):
    """every node start and accept, `per_node` arcs each (labels 0 .. per_node-1: to itself, to the next node, to the one
    after ...; the last nodes wrap around), `extra` more arcs from node 0 (further labels): levels are No wide from t = 0"""
    arcs = []
    for n in range(No):
        for k in range(per_node):
            if per_node == 2 and k == 1 and n == No - 1:
                continue           # the classic strands: the last node has its loop only
            arcs.append((n, (n + k) % No, k))
    for k in range(extra):
        arcs.append((0, (per_node + k) % No, per_node + k))
    return acceptor([1] * No, [1] * No, arcs, rng)


def ring(No, deg, rng):
    """node i -> i + 1 (mod No) with deg distinct labels: one node per time, the co-reachable sets never settle"""
    arcs = [(n, (n + 1) % No, l) for n in range(No) for l in range(deg)]
    return acceptor([1] + [0] * (No - 1), [0] * (No - 1) + [1], arcs, rng)


def fan_out(k, rng, big_label_at=None, C=6):
    """node 0 (start) with k arcs to k loop-and-accept nodes"""
    arcs = [(0, 1 + j, (C + 3 if j == big_label_at else j)) for j in range(k)] + [(1 + j, 1 + j, 0) for j in range(k)]
    return acceptor([1] + [0] * k, [0] + [1] * k, arcs, rng)


def fan_in(k, rng):
    """k looping start nodes, each with one arc into node 0 (accept, no loop): in-degree exactly k"""
    arcs = []
    for j in range(k):
        arcs += [(1 + j, 1 + j, 0), (1 + j, 0, 1 + j)]
    return acceptor([0] + [1] * k, [1] + [0] * k, arcs, rng)


def dense_strands(No, deg, rng):
    """every node start and accept with deg arcs (labels 0 .. deg-1) to the next deg nodes: A = deg * No"""
    arcs = [(n, (n + 1 + k) % No, k) for n in range(No) for k in range(deg)]
    return acceptor([1] * No, [1] * No, arcs, rng)


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
CASES = {}      # name -> {"build": fn(rng) -> [(a, b), ...], "mode", "env", "sizes": [(N, A), ...], "cells": {...}}
THRESHOLDS = {}  # what the pair of cases sits on either side of -> (case below / at, case above)


def case(name, build, sizes, cells, mode="compose", env=(), calls=None):
    assert name not in CASES, name
    CASES[name] = {"build": build, "mode": mode, "env": tuple(env), "sizes": sizes, "cells": set(cells), "calls": calls}


def chain_case(base, partner, T, C, sizes, cells, env=(), combos=None):
    """the four ways to write a chain product: chain first / second x compose / intersect"""
    for side in ("cf", "cs"):
        for mode in ("compose", "intersect"):
            if combos and (side, mode) not in combos:
                continue

            def build(rng, side=side):
                p, c = partner(rng), chain(T, C, rng)
                return [(c, p) if side == "cf" else (p, c)]
            case("%s/%s/%s" % (base, side, mode), build, [sizes], cells, mode, env)


FAST_DEFERRED = {"fast256", "bitmap/window_full", "arrays/skipped", "sizes/deferred", "layered",
                 "replicate/grid"}

# ---- FAST chain products -------------------------------------------------------------------------------------------
chain_case("ctc/U3-T8", lambda r: ctc_partner(3, 5, r), 8, 5, (39, 75), FAST_DEFERRED)
# (deep enough for the narrow shortest-distance kernels, whose backward scatters compose's gradient itself)
chain_case("ctc/U3-T40", lambda r: ctc_partner(3, 5, r), 40, 5, (263, 555), FAST_DEFERRED)
for _T, _sz in ((1, (0, 0)), (2, (0, 0))):
    chain_case("ctc/U3-T%d" % _T, lambda r: ctc_partner(3, 5, r), _T, 5, _sz, FAST_DEFERRED)
    chain_case("ctc/U3-T%d/classic-bitmaps" % _T, lambda r: ctc_partner(3, 5, r), _T, 5, _sz,
               {"fast256", "bitmap/classic", "sizes/read", "arrays/skipped"}, env=("GTNX_CLASSIC_BITMAPS",))
for _T, _sz in ((1, (2, 1)), (2, (5, 5))):
    chain_case("ctc/U1-T%d" % _T, lambda r: ctc_partner(1, 5, r), _T, 5, _sz, FAST_DEFERRED)
    chain_case("ctc/U1-T%d/classic-bitmaps" % _T, lambda r: ctc_partner(1, 5, r), _T, 5, _sz,
               {"fast256", "bitmap/classic", "sizes/read", "arrays/skipped"}, env=("GTNX_CLASSIC_BITMAPS",))
# degenerate operands
chain_case("degenerate/T0", lambda r: ctc_partner(3, 5, r), 0, 5, (0, 0), {"fast256", "bitmap/window_full", "sizes/read"})
chain_case("degenerate/one-node-loop", lambda r: acceptor([1], [1], [(0, 0, 2)], r), 6, 5, (7, 6), FAST_DEFERRED)
chain_case("degenerate/no-nodes", lambda r: acceptor([], [], [], r), 4, 5, (0, 0), {"fast256", "bitmap/classic", "sizes/read"})
chain_case("degenerate/no-accept", lambda r: acceptor([1, 0], [0, 0], [(0, 1, 0), (1, 1, 1)], r), 4, 5, (0, 0), FAST_DEFERRED)
chain_case("degenerate/labels-beyond-C", lambda r: acceptor([1, 0], [0, 1], [(0, 1, 5), (1, 1, 7), (0, 0, 6)], r), 4, 5,
           (0, 0), FAST_DEFERRED)
# strands: 256 / 512 lanes, single / multi-chunk levels, the widest chain window, classic bitmaps beyond it
chain_case("strands/256", lambda r: strands(256, r), 5, 3, (1536, 2555), FAST_DEFERRED)
chain_case("strands/257", lambda r: strands(257, r), 5, 3, (1542, 2565),
           {"fast512", "bitmap/window_full", "arrays/skipped", "sizes/deferred"})
chain_case("strands/257/narrow", lambda r: strands(257, r), 5, 3, (1542, 2565),
           {"fast256", "bitmap/window_full", "arrays/full", "sizes/read"}, env=("GTNX_NARROW_COMPOSE",))
chain_case("strands/512", lambda r: strands(512, r), 5, 3, (3072, 5115),
           {"fast512", "bitmap/window_full", "arrays/skipped", "sizes/deferred"})
chain_case("strands/513", lambda r: strands(513, r), 5, 3, (3078, 5125),
           {"fast256", "bitmap/window_full", "arrays/full", "sizes/read", "transpose"})
chain_case("strands/1024", lambda r: strands(1024, r), 5, 3, (6144, 10235),
           {"fast256", "bitmap/window_full", "arrays/full", "sizes/read", "transpose"})
chain_case("strands/1025", lambda r: strands(1025, r), 5, 3, (6150, 10245),
           {"fast256", "bitmap/classic", "arrays/full", "sizes/read", "transpose"})
chain_case("strands/1025-T208", lambda r: strands(1025, r), 208, 3, (214225, 426192),
           {"general/hbm", "arrays/full", "sizes/read", "transpose", "layered"})
# a window shorter than the chain
chain_case("window/ctc-U2-T13400", lambda r: ctc_partner(2, 3, r), 13400, 3, (66993, 133980),
           {"fast256", "bitmap/window_partial", "sizes/read", "arrays/skipped", "replicate/grid"})
chain_case("window/strands-512-T700", lambda r: strands(512, r), 700, 3, (358912, 716100),
           {"fast512", "bitmap/window_partial", "sizes/read", "arrays/skipped"})
# periodic partners: never stationary
chain_case("ring/3x3-T8", lambda r: ring(3, 3, r), 8, 5, (9, 24), FAST_DEFERRED)
chain_case("ring/2-T9", lambda r: ring(2, 2, r), 9, 5, (10, 18), FAST_DEFERRED)
chain_case("ring/2-T8-empty", lambda r: ring(2, 2, r), 8, 5, (0, 0), FAST_DEFERRED)
chain_case("ring/3x3-T13400", lambda r: ring(3, 3, r), 13400, 5, (13401, 40200),
           {"fast256", "bitmap/window_partial", "redo/fast->wide_chain", "transpose", "arrays/full", "sizes/read"})
chain_case("ring/3x3-T13400/no-wide", lambda r: ring(3, 3, r), 13400, 5, (13401, 40200),
           {"fast256", "bitmap/window_partial", "redo/fast->general", "arrays/full", "sizes/read"},
           env=("GTNX_NO_WIDE_COMPOSE",))
chain_case("ring/2x9-T9", lambda r: ring(2, 9, r), 9, 12, (10, 81), {"wide_chain", "transpose", "arrays/full", "layered"})
# KC candidates per node, out-lists (phase F) and in-lists (phase B)
chain_case("degree/out-4", lambda r: fan_out(4, r), 5, 6, (21, 20), FAST_DEFERRED)
chain_case("degree/out-5", lambda r: fan_out(5, r), 5, 6, (26, 25), {"fast256", "sizes/read", "redo/fast->wide_chain"})
chain_case("degree/out-5-one-beyond-C", lambda r: fan_out(5, r, big_label_at=2), 5, 6, (21, 20),
           {"fast256", "sizes/read", "arrays/skipped"})
chain_case("degree/in-4", lambda r: fan_in(4, r), 5, 6, (21, 20), FAST_DEFERRED)
chain_case("degree/in-5", lambda r: fan_in(5, r), 5, 6, (26, 25), {"fast256", "sizes/read", "redo/fast->wide_chain"})
# a level's arcs against 3/4 of the claim hash (and the host's A <= 768 / 1536 rule for deferring the sizes)
chain_case("level-arcs/256x768", lambda r: strands(256, r, per_node=3), 4, 5, (1280, 3072), FAST_DEFERRED)
chain_case("level-arcs/256x769", lambda r: strands(256, r, per_node=3, extra=1), 4, 5, (1280, 3076),
           {"fast256", "sizes/read", "redo/fast->wide_chain"})
chain_case("level-arcs/512x1536", lambda r: strands(512, r, per_node=3), 4, 5, (2560, 6144),
           {"fast512", "sizes/deferred", "arrays/skipped"})
chain_case("level-arcs/512x1537", lambda r: strands(512, r, per_node=3, extra=1), 4, 5, (2560, 6148),
           {"fast512", "sizes/read", "redo/fast->wide_chain"})
# ---- wide chain products: the node cap of compose_wide.hip ---------------------------------------------------------------
chain_case("wide/2048", lambda r: dense_strands(2048, 5, r), 3, 6, (8192, 30720), {"wide_chain", "transpose", "layered"})
chain_case("wide/2049", lambda r: dense_strands(2049, 5, r), 3, 6, (8196, 30735),
           {"fast256", "bitmap/classic", "redo/fast->general", "arrays/full"})


# ---- more than 128 FAST chain pairs in one call ------------------------------------------------------------------------
def _many(_, n=130):
    rng = rng_of("batch/130")     # the same 130 pairs in both cases
    return [(chain(6 + k % 5, 5, rng), ctc_partner(1 + k % 3, 5, rng)) for k in range(n)]


case("batch/130-inline", _many, None, {"fast256", "replicate/inline", "sizes/deferred"})
case("batch/130-in-two-calls", _many, None, {"fast256", "replicate/grid", "sizes/deferred"}, calls=[(0, 65), (65, 130)])


# ---- two explicit graphs ----------------------------------------------------------------------------------------------------
def dag(rng, N, A, nlabels, sort=None, eps_i=0.0, eps_o=0.0, p_start=0.3, p_accept=0.3, cyclic=False):
    """random graph (acyclic unless asked: arcs go to later nodes, so forwardScore applies to the product), the labels
    of a node's arcs distinct on either side (equal sort keys would expose std::sort's freedom), epsilons with the
    given probability on either label (several per node stay in insertion order: the lists are short)"""
    start = (rng.random(N) < p_start).astype(int).tolist()
    accept = (rng.random(N) < p_accept).astype(int).tolist()
    start[0] = 1
    accept[-1] = 1
    src = rng.integers(0, N if cyclic else N - 1, A).tolist()
    arcs = []
    for n in range(N):
        k = min(src.count(n), nlabels)
        li, lo = rng.permutation(nlabels)[:k], rng.permutation(nlabels)[:k]
        for x, y in zip(li, lo):
            i, o = int(x), int(y)
            if rng.random() < eps_i:
                i = EPS
            if rng.random() < eps_o:
                o = EPS
            arcs.append((n, int(rng.integers(0 if cyclic else n + 1, N)), i, o))
    perm = rng.permutation(len(arcs))
    return graph(start, accept, [arcs[k] for k in perm], rng, sort)


def search(rng, make, ok, tries=400):
    """the first draw of `make` from the case's stream that `ok` accepts"""
    for _ in range(tries):
        c = make(rng)
        if ok(c):
            return c
    raise AssertionError("no draw fits")


def _with_arcs(rng, N, A, nlabels, sort):
    """an acceptor of exactly A arcs, distinct labels per node (the pairs_pref threshold is on A against 4 N)"""
    d = dag(rng, N, A, nlabels, sort, cyclic=True)
    while len(d["src"]) < A:
        n = int(rng.integers(0, N))
        used = {d["il"][k] for k in range(len(d["src"])) if d["src"][k] == n}
        free = [l for l in range(nlabels) if l not in used]
        if not free:
            continue
        d["src"].append(n); d["dst"].append(int(rng.integers(0, N))); d["il"].append(free[0]); d["ol"].append(free[0])
        d["w"].append(float(np.float32(rng.normal())))
    d["ol"] = list(d["il"])
    return d


SORTS = {"unsorted": (None, None), "singly-g1": ("o", None), "singly-g2": (None, "i"), "doubly": ("o", "i")}


def eps_deciders(d1, d2, w):
    """product nodes where epsilon_matched holds and compose.cpp:461 (g1's epsilon arcs held back) / :476 (g2's)
    decides: (n461, n476)"""
    f1, f2 = Facts(d1), Facts(d2)
    n461 = n476 = 0
    for idx in w.pairs:
        n1, n2 = idx % f1.N, idx // f1.N
        em = any(f1.ol[a] == EPS for a in f1.out[n1]) and any(f2.il[a] == EPS for a in f2.out[n2])
        n461 += em and bool(f1.is_accept[n1]) and not f2.is_accept[n2]
        n476 += em and not f1.is_accept[n1]
    return n461, n476


def _eps_pair(rng, sorts, where, hub):
    e1 = 0.35 if where in ("g1", "both") else 0.0
    e2 = 0.35 if where in ("g2", "both") else 0.0

    def make(r):
        d1 = dag(r, 9, 16, 4, sorts[0], eps_o=e1, p_accept=0.5)
        d2 = dag(r, 8, 14, 4, sorts[1], eps_i=e2, p_accept=0.5)
        if hub:
            # five parallel matches between a start pair and an accept pair of their own: more than KC candidates in
            # either direction, the FAST variant gives the product back; both graphs keep A <= 2 N, so the general
            # variant takes it (not compose_wide.hip's pair kernel)
            for d, N, k in ((d1, 9, 5), (d2, 8, 1)):
                d["start"] += [1, 0] + [0] * 8
                d["accept"] += [0, 1] + [0] * 8
                for j in range(k):
                    d["src"].append(N); d["dst"].append(N + 1); d["il"].append(30 + j); d["ol"].append(20)
                    d["w"].append(0.125 * j)
            d2["il"][-1] = 20
        return d1, d2

    def ok(c):
        f1, f2 = Facts(c[0]), Facts(c[1])
        w = sim_pairs(f1, f2, False)
        gone = w.handback or not w.chunks_fast[256]
        if bool(gone) != hub or w.A < 8 or f1.A > 2 * f1.N or f2.A > 2 * f2.N:
            return False
        use1, use2 = any(y < 0 for _, _, _, y in w.arcs), any(x < 0 for _, _, x, _ in w.arcs)
        if where == "g1":
            return use1
        if where == "g2":
            return use2
        n461, n476 = eps_deciders(c[0], c[1], w)
        return use1 and use2 and n461 > 0 and n476 > 0
    return search(rng, make, ok, 4000)


for _m, _s in SORTS.items():
    for _where in ("g1", "g2", "both"):
        case("eps/%s/%s/fast" % (_m, _where), lambda r, s=_s, wh=_where: [_eps_pair(r, s, wh, False)], None,
             {"fast256", "g1_cache/on", "sizes/read", "arrays/full"})
        case("eps/%s/%s/general" % (_m, _where), lambda r, s=_s, wh=_where: [_eps_pair(r, s, wh, True)], None,
             {"fast256", "redo/fast->general", "arrays/full"})
    # pairs_pref: A = 4 N against 4 N + 1
    case("pairs-pref/%s/4N" % _m, lambda r, s=_s: [(_with_arcs(r, 12, 48, 8, s[0]), _with_arcs(r, 10, 30, 8, s[1]))], None,
         {"fast256", "redo/fast->pairs", "transpose"})
    case("pairs-pref/%s/4N+1" % _m, lambda r, s=_s: [(_with_arcs(r, 12, 49, 8, s[0]), _with_arcs(r, 10, 30, 8, s[1]))], None,
         {"pairs", "transpose"})


def ladder(rng, N):
    """node n -> n + 1 and n + 2 with the labels 0 and 1 in random order: two arcs out of and into every node, so a
    pair of ladders never has more than KC candidates in either direction"""
    arcs = []
    for n in range(N - 1):
        a = int(rng.integers(0, 2))
        arcs.append((n, n + 1, a))
        if n + 2 < N:
            arcs.append((n, n + 2, 1 - a))
    return acceptor([1] + [0] * (N - 1), [0] * (N - 2) + [1, 1], arcs, rng)


def _fast_pair(rng):
    def ok(c):
        w = sim_pairs(Facts(c[0]), Facts(c[1]), False)
        return not w.handback and w.chunks_fast[256] and w.A >= 30
    return search(rng, lambda r: (ladder(r, 24), ladder(r, 20)), ok)


case("explicit/fast-cache-on", lambda r: [_fast_pair(r)], None, {"fast256", "g1_cache/on", "sizes/read", "arrays/full"})


def grad_chain_pair(rng):
    """3100 steps of two parallel arcs against a one-node loop graph: the product is g1's shape, 6200 arcs in two
    4096-arc chunks of compose_grad_kernel.  g1's ARC IDS are dealt so that the first chunk's arcs span ids 0 .. 6199
    (direct atomics) and the second chunk's 2104 arcs the ids 2048 .. 4151 (the LDS window).  g1's records (97 KB) do
    not fit beside the bitmaps: g1_cache/off."""
    steps = 3100
    prod = [(m, m + 1, l) for m in range(steps) for l in range(2)]          # in the product's arc order
    ids = list(range(0, 2048)) + list(range(4152, 6200)) + list(range(2048, 4152))
    arcs = [None] * len(prod)
    for k, a in enumerate(prod):
        arcs[ids[k]] = a
    d1 = acceptor([1] + [0] * steps, [0] * steps + [1], arcs, rng)
    d2 = acceptor([1], [1], [(0, 0, 0), (0, 0, 1)], rng)
    return d1, d2


case("explicit/grad-chunks", lambda r: [grad_chain_pair(r)], [(3101, 6200)], {"fast256", "g1_cache/off", "arrays/full"})


def _big_pair(rng, N1, N2):
    return (gg.random_graph(rng, N1, 3 * N1, nlabels=6), gg.random_graph(rng, N2, 3 * N2, nlabels=6))


# the classic-bitmap budget: 2 * 4 * ceil(N1 N2 / 32) against 53248 bytes, i.e. N1 N2 <= 212992 = 416 * 512
case("budget/416x512", lambda r: [_big_pair(r, 416, 512)], None, {"fast256"})
case("budget/417x512", lambda r: [_big_pair(r, 417, 512)], None, {"general/hbm", "not_layered", "transpose"})
case("budget/470x470", lambda r: [_big_pair(r, 470, 470)], None, {"general/hbm", "not_layered", "transpose"})


def _mixed(rng):
    return [_big_pair(rng, 470, 470), _fast_pair(rng), _eps_pair(rng, (None, None), "both", False)]


case("batch/mixed-big-and-small", _mixed, None, {"general/hbm", "general/lds"})


# ---- a device-built operand: {"product": (a, b, mode)} is composed on the device first -------------------------------
def _nested_inner(rng):
    return {"product": (ladder(rng, 9), ladder(rng, 8), "compose")}


def _nonempty(c):
    return to_oracle(c[0]).compose(to_oracle(c[1])).A >= 20


case("device-built/chain-x-product", lambda r: [search(r, lambda q: (chain(5, 3, q), _nested_inner(q)), _nonempty)], None,
     {"fast256", "sizes/read"})
case("device-built/product-x-graph", lambda r: [search(r, lambda q: (_nested_inner(q), ladder(q, 9)), _nonempty)], None,
     {"sizes/read"})

# ---- the product stays symbolic (gtn.compose_mode(1)) ---------------------------------------------------------------------
case("symbolic/ctc-U3-T8", lambda r: [(ctc_partner(3, 5, r), chain(8, 5, r))], [(39, 75)], {"symbolic"}, mode="intersect")
CASES["symbolic/ctc-U3-T8"]["compose_mode"] = 1

# every threshold of the issue -> the case at or below it, the case above it
THRESHOLDS.update({
    "KC out-arcs": ("degree/out-4/cf/compose", "degree/out-5/cf/compose"),
    "KC in-arcs": ("degree/in-4/cf/compose", "degree/in-5/cf/compose"),
    "3/4 HC, 256 lanes": ("level-arcs/256x768/cf/compose", "level-arcs/256x769/cf/compose"),
    "3/4 HC, 512 lanes": ("level-arcs/512x1536/cf/compose", "level-arcs/512x1537/cf/compose"),
    "partner 256/257": ("strands/256/cf/compose", "strands/257/cf/compose"),
    "partner 512/513": ("strands/512/cf/compose", "strands/513/cf/compose"),
    "partner 1024/1025": ("strands/1024/cf/compose", "strands/1025/cf/compose"),
    "wide node cap": ("wide/2048/cf/compose", "wide/2049/cf/compose"),
    "classic budget, chain": ("strands/1025/cf/compose", "strands/1025-T208/cf/compose"),
    "classic budget, explicit": ("budget/416x512", "budget/417x512"),
    "window shorter than the chain": ("ctc/U3-T8/cf/compose", "window/ctc-U2-T13400/cf/compose"),
    "pairs_pref 4N": ("pairs-pref/unsorted/4N", "pairs-pref/unsorted/4N+1"),
    "inline_rep_for 128": ("batch/130-in-two-calls", "batch/130-inline"),
})


# an edge inside one kernel: both sides take the same cells (the classic stationarity fill needs tau >= 2: chains of one
# and two steps under GTNX_CLASSIC_BITMAPS)
SAME_ROUTE_EDGES = {"tau >= 2": ("ctc/U1-T1/classic-bitmaps/cf/compose", "ctc/U1-T2/classic-bitmaps/cf/compose")}


@functools.lru_cache(maxsize=None)
def build(name):
    return CASES[name]["build"](rng_of(name.split("/cf/")[0].split("/cs/")[0]))


def calls_of(name):
    """the slices of build(name) that go into one call each"""
    c = CASES[name]["calls"]
    return c if c else [(0, len(build(name)))]


@functools.lru_cache(maxsize=None)
def expected_routes(name):
    c = CASES[name]
    total = {}
    pairs = build(name)
    if c.get("compose_mode") == 1:     # eligible chain products stay symbolic: nothing is built
        return {"symbolic": len(pairs)}
    calls = [(pairs[lo:hi], c["mode"]) for lo, hi in calls_of(name)]
    for a, b in pairs:                 # device-built operands are composed first, one call each
        for g in (a, b):
            if "product" in g:
                calls.append(([g["product"][:2]], g["product"][2]))
    for ps, mode in calls:
        for k, v in predict(ps, mode, c["env"]).items():
            total[k] = total.get(k, 0) + v
    return total


# ---------------------------------------------------------------------------------------------------------------------
# oracle side and API side of an operand
# ---------------------------------------------------------------------------------------------------------------------
def to_oracle(g):
    from oracle_lib import OGraph
    if is_chain(g):
        T, C = g["chain"]
        return OGraph.linear(T, C, g["w"] if T * C else None)
    if "product" in g:
        return to_oracle(g["product"][0]).compose(to_oracle(g["product"][1]), g["product"][2])
    return OGraph.from_dict(g)


def to_api(gtn, g, calc_grad=True):
    if is_chain(g):
        T, C = g["chain"]
        e = gtn.linear_graph(T, C, calc_grad)
        if T * C:
            e.set_weights(g["w"])
        return e
    if "product" in g:
        a, b, mode = g["product"]
        fn = gtn.intersect if mode == "intersect" else gtn.compose
        return fn(to_api(gtn, a, calc_grad), to_api(gtn, b, calc_grad))
    return gg.to_api(gtn, g, calc_grad)


def num_arcs(g):
    if "product" in g:
        return to_oracle(g).A
    return g["chain"][0] * g["chain"][1] if is_chain(g) else len(g["src"])


def oracle_arrays(og):
    """(start, accept, src, dst, il, ol, w) of an OGraph as numpy arrays"""
    from oracle_lib import lib
    N, A = og.N, og.A
    st, ac = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
    s, d, i, o = (np.zeros(A, np.int32) for _ in range(4))
    w = np.zeros(A, np.float32)
    lib().og_get_nodes(og.h, st.ctypes.data, ac.ctypes.data)
    lib().og_get_arcs(og.h, s.ctypes.data, d.ctypes.data, i.ctypes.data, o.ctypes.data, w.ctypes.data)
    return np.flatnonzero(st), np.flatnonzero(ac), s, d, i, o, w


@functools.lru_cache(maxsize=8)
def oracle_products(name):
    """[OGraph product] of the case, in pair order (the largest cases take a few tenths of a second)"""
    mode = CASES[name]["mode"]
    return [to_oracle(a).compose(to_oracle(b), mode) for a, b in build(name)]


# ---- product sizes of the cases that do not state them inline (the oracle's numbers when the case was written;
# tests/test_compose_cells_cpu.py holds the oracle to them)
SIZES = {
    'batch/130-inline': [(17, 25), (28, 50), (39, 75), (26, 40), (43, 80), (25, 45), (20, 30), (33, 60), (46, 90), (29, 45), (23, 40), (32, 60), (23, 35), (38, 70), (53, 105), (17, 25), (28, 50), (39, 75), (26, 40), (43, 80), (25, 45), (20, 30), (33, 60), (46, 90), (29, 45), (23, 40), (32, 60), (23, 35), (38, 70), (53, 105), (17, 25), (28, 50), (39, 75), (26, 40), (43, 80), (25, 45), (20, 30), (33, 60), (46, 90), (29, 45), (23, 40), (32, 60), (23, 35), (38, 70), (53, 105), (17, 25), (28, 50), (39, 75), (26, 40), (43, 80), (25, 45), (20, 30), (33, 60), (46, 90), (29, 45), (23, 40), (32, 60), (23, 35), (38, 70), (53, 105), (17, 25), (28, 50), (39, 75), (26, 40), (43, 80), (25, 45), (20, 30), (33, 60), (46, 90), (29, 45), (23, 40), (32, 60), (23, 35), (38, 70), (53, 105), (17, 25), (28, 50), (39, 75), (26, 40), (43, 80), (25, 45), (20, 30), (33, 60), (46, 90), (29, 45), (23, 40), (32, 60), (23, 35), (38, 70), (53, 105), (17, 25), (28, 50), (39, 75), (26, 40), (43, 80), (25, 45), (20, 30), (33, 60), (46, 90), (29, 45), (23, 40), (32, 60), (23, 35), (38, 70), (53, 105), (17, 25), (28, 50), (39, 75), (26, 40), (43, 80), (25, 45), (20, 30), (33, 60), (46, 90), (29, 45), (23, 40), (32, 60), (23, 35), (38, 70), (53, 105), (17, 25), (28, 50), (39, 75), (26, 40), (43, 80), (25, 45), (20, 30), (33, 60), (46, 90), (29, 45)],
    'batch/130-in-two-calls': [(17, 25), (28, 50), (39, 75), (26, 40), (43, 80), (25, 45), (20, 30), (33, 60), (46, 90), (29, 45), (23, 40), (32, 60), (23, 35), (38, 70), (53, 105), (17, 25), (28, 50), (39, 75), (26, 40), (43, 80), (25, 45), (20, 30), (33, 60), (46, 90), (29, 45), (23, 40), (32, 60), (23, 35), (38, 70), (53, 105), (17, 25), (28, 50), (39, 75), (26, 40), (43, 80), (25, 45), (20, 30), (33, 60), (46, 90), (29, 45), (23, 40), (32, 60), (23, 35), (38, 70), (53, 105), (17, 25), (28, 50), (39, 75), (26, 40), (43, 80), (25, 45), (20, 30), (33, 60), (46, 90), (29, 45), (23, 40), (32, 60), (23, 35), (38, 70), (53, 105), (17, 25), (28, 50), (39, 75), (26, 40), (43, 80), (25, 45), (20, 30), (33, 60), (46, 90), (29, 45), (23, 40), (32, 60), (23, 35), (38, 70), (53, 105), (17, 25), (28, 50), (39, 75), (26, 40), (43, 80), (25, 45), (20, 30), (33, 60), (46, 90), (29, 45), (23, 40), (32, 60), (23, 35), (38, 70), (53, 105), (17, 25), (28, 50), (39, 75), (26, 40), (43, 80), (25, 45), (20, 30), (33, 60), (46, 90), (29, 45), (23, 40), (32, 60), (23, 35), (38, 70), (53, 105), (17, 25), (28, 50), (39, 75), (26, 40), (43, 80), (25, 45), (20, 30), (33, 60), (46, 90), (29, 45), (23, 40), (32, 60), (23, 35), (38, 70), (53, 105), (17, 25), (28, 50), (39, 75), (26, 40), (43, 80), (25, 45), (20, 30), (33, 60), (46, 90), (29, 45)],
    'eps/unsorted/g1/fast': [(11, 10)],
    'eps/unsorted/g1/general': [(10, 14)],
    'eps/unsorted/g2/fast': [(11, 12)],
    'eps/unsorted/g2/general': [(15, 22)],
    'eps/unsorted/both/fast': [(16, 11)],
    'eps/unsorted/both/general': [(19, 18)],
    'pairs-pref/unsorted/4N': [(40, 65)],
    'pairs-pref/unsorted/4N+1': [(39, 49)],
    'eps/singly-g1/g1/fast': [(19, 12)],
    'eps/singly-g1/g1/general': [(36, 41)],
    'eps/singly-g1/g2/fast': [(11, 8)],
    'eps/singly-g1/g2/general': [(23, 26)],
    'eps/singly-g1/both/fast': [(16, 16)],
    'eps/singly-g1/both/general': [(25, 29)],
    'pairs-pref/singly-g1/4N': [(33, 45)],
    'pairs-pref/singly-g1/4N+1': [(32, 43)],
    'eps/singly-g2/g1/fast': [(13, 10)],
    'eps/singly-g2/g1/general': [(10, 11)],
    'eps/singly-g2/g2/fast': [(23, 27)],
    'eps/singly-g2/g2/general': [(16, 18)],
    'eps/singly-g2/both/fast': [(18, 14)],
    'eps/singly-g2/both/general': [(21, 33)],
    'pairs-pref/singly-g2/4N': [(49, 79)],
    'pairs-pref/singly-g2/4N+1': [(41, 58)],
    'eps/doubly/g1/fast': [(9, 10)],
    'eps/doubly/g1/general': [(14, 13)],
    'eps/doubly/g2/fast': [(17, 17)],
    'eps/doubly/g2/general': [(10, 13)],
    'eps/doubly/both/fast': [(17, 21)],
    'eps/doubly/both/general': [(23, 25)],
    'pairs-pref/doubly/4N': [(27, 36)],
    'pairs-pref/doubly/4N+1': [(24, 25)],
    'explicit/fast-cache-on': [(99, 170)],
    'budget/416x512': [(52162, 79756)],
    'budget/417x512': [(51774, 77102)],
    'budget/470x470': [(54711, 82701)],
    'batch/mixed-big-and-small': [(46698, 67734), (69, 112), (15, 16)],
    'device-built/chain-x-product': [(22, 26)],
    'device-built/product-x-graph': [(20, 21)],
}
for _n, _s in SIZES.items():
    CASES[_n]["sizes"] = _s
