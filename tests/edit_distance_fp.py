"""The yardstick of the batched edit distance (gtnx_batch_edit_distance), on the host.

* `table` / `walk_back` / `distance_ops`: the textbook O(mn) table in numpy and the contract's walk back from
  (len_ref, len_hyp): at every cell the first move that attains D[i][j] of diagonal (match or substitution), up (a
  deletion: a reference token without counterpart), left (an insertion).
* `blocks_forward` / `blocks_cell` / `blocks_walk`: a plain-Python transcription of what edit_distance.hip does --
  Myers' bit-vector recurrence in Hyyro's block form over 64-row blocks, block-major with the horizontal carries of a
  chunk of 64 columns kept as two masks, the distance followed along row len_ref of the last block, and the walk over
  the (Pv, Mv) words of every (column, block) by popcounts.  A GPU miss then means a wrong kernel, not a wrong formula.
* the seeded case lists test_edit_distance_cpu.py and test_edit_distance_gpu.py share.

Everything is an integer: every comparison in the tests is ==."""
import functools

import numpy as np

M64 = (1 << 64) - 1
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1


# ---- the textbook table ----
def table(ref, hyp):
    """D[i][j] = distance of ref[:i] and hyp[:j], int64 [m + 1, n + 1], unit costs"""
    ref, hyp = np.asarray(ref, np.int64), np.asarray(hyp, np.int64)
    m, n = len(ref), len(hyp)
    D = np.zeros((m + 1, n + 1), np.int64)
    D[0] = np.arange(n + 1)
    cols = np.arange(n + 1)
    for i in range(1, m + 1):
        t = np.empty(n + 1, np.int64)
        t[0] = i
        t[1:] = np.minimum(D[i - 1, :-1] + (hyp != ref[i - 1]), D[i - 1, 1:] + 1)
        # the moves to the left: D[i][j] = min over k <= j of t[k] + (j - k)
        D[i] = np.minimum.accumulate(t - cols) + cols
    return D


def walk_back(D, ref, hyp):
    """(substitutions, deletions, insertions, matches) of the contract's walk"""
    i, j = len(ref), len(hyp)
    s = d = ins = mt = 0
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i - 1][j - 1] + (ref[i - 1] != hyp[j - 1]) == D[i][j]:
            if ref[i - 1] != hyp[j - 1]:
                s += 1
            else:
                mt += 1
            i, j = i - 1, j - 1
        elif i > 0 and D[i - 1][j] + 1 == D[i][j]:
            d += 1
            i -= 1
        else:
            assert j > 0 and D[i][j - 1] + 1 == D[i][j]
            ins += 1
            j -= 1
    return s, d, ins, mt


def distance_ops(ref, hyp):
    """(dist, (S, D, I), matches) by the table"""
    ref, hyp = [int(v) for v in ref], [int(v) for v in hyp]
    D = table(ref, hyp)
    s, d, ins, mt = walk_back(D, ref, hyp)
    return int(D[len(ref)][len(hyp)]), (s, d, ins), mt


# ---- the kernel's recurrence, transcribed ----
def _popc(x):
    return bin(x).count("1")


def blocks_forward(ref, hyp):
    """(dist, words): words[j - 1][blk] = (Pv, Mv) of block blk after column j, as the kernel keeps them for the walk"""
    ref, hyp = [int(v) for v in ref], [int(v) for v in hyp]
    m, n = len(ref), len(hyp)
    nb, chunks = (m + 63) >> 6, (n + 63) >> 6
    words = [[None] * nb for _ in range(n)]
    carry = [(0, 0)] * chunks
    score = n if nb == 0 else m
    lastbit = (m - 1) & 63
    for blk in range(nb):
        rows = ref[64 * blk:64 * blk + 64]
        last = blk == nb - 1
        Pv, Mv = M64, 0
        for c in range(chunks):
            hp, hm = (M64, 0) if blk == 0 else carry[c]
            op = om = 0
            for k in range(min(64, n - 64 * c)):
                tok = hyp[64 * c + k]
                Eq = 0
                for lane, r in enumerate(rows):
                    if r == tok:
                        Eq |= 1 << lane
                hpos, hneg = (hp >> k) & 1, (hm >> k) & 1
                Xv = Eq | Mv
                Eq |= hneg
                Xh = ((((Eq & Pv) + Pv) & M64) ^ Pv) | Eq
                Ph = (Mv | ~(Xh | Pv)) & M64
                Mh = Pv & Xh
                if last:
                    score += ((Ph >> lastbit) & 1) - ((Mh >> lastbit) & 1)
                op |= (Ph >> 63) << k
                om |= (Mh >> 63) << k
                Ph = ((Ph << 1) | hpos) & M64
                Mh = ((Mh << 1) | hneg) & M64
                Pv = (Mh | ~(Xv | Ph)) & M64
                Mv = Ph & Xv
                words[64 * c + k][blk] = (Pv, Mv)
            if not last:
                carry[c] = (op, om)
    return score, words


def blocks_cell(words, nb, i, j):
    """D[i][j] from the words: j + popcount(Pv_j & low_i) - popcount(Mv_j & low_i) summed over the blocks"""
    v = j
    for blk in range(nb):
        rows = min(max(i - 64 * blk, 0), 64)
        low = (1 << rows) - 1
        Pv, Mv = (M64, 0) if j == 0 else words[j - 1][blk]
        v += _popc(Pv & low) - _popc(Mv & low)
    return v


def blocks_walk(ref, hyp, dist, words):
    """(S, D, I) as the kernel's walk finds them: D[i][j] carried along, D[i-1][j-1] by popcounts of column j - 1, up by
    bit i - 1 of column j's Pv"""
    ref, hyp = [int(v) for v in ref], [int(v) for v in hyp]
    i, j, d = len(ref), len(hyp), dist
    nb = (len(ref) + 63) >> 6
    s = dl = ins = 0
    while i > 0 and j > 0:
        dd = blocks_cell(words, nb, i - 1, j - 1)
        cost = int(ref[i - 1] != hyp[j - 1])
        if dd + cost == d:
            s += cost
            d = dd
            i, j = i - 1, j - 1
        else:
            r = i - 1
            d -= 1
            if (words[j - 1][r >> 6][0] >> (r & 63)) & 1:
                dl += 1
                i -= 1
            else:
                ins += 1
                j -= 1
    return s, dl + i, ins + j


def blocks_distance_ops(ref, hyp):
    dist, words = blocks_forward(ref, hyp)
    return dist, blocks_walk(ref, hyp, dist, words)


# ---- seeded cases ----
def edited(ref, rng, n, alphabet):
    """`ref` under random edits (a tenth of the tokens dropped, a tenth replaced, a tenth followed by a new one), cut
    or filled up to n tokens"""
    out = []
    for t in ref:
        u = rng.rand()
        if u < 0.1:
            continue
        out.append(int(rng.randint(0, alphabet)) if u < 0.2 else int(t))
        if u > 0.9:
            out.append(int(rng.randint(0, alphabet)))
    while len(out) < n:
        out.append(int(rng.randint(0, alphabet)))
    return out[:n]


def seeded_pair(seed, m, n, alphabet):
    """a reference of m and a hypothesis of n tokens below `alphabet`: the hypothesis is the reference under random
    edits where the seed is odd (so that a large alphabet does not just give max(m, n)), independent otherwise"""
    rng = np.random.RandomState(seed)
    ref = rng.randint(0, alphabet, size=m).tolist()
    hyp = edited(ref, rng, n, alphabet) if seed % 2 and m else rng.randint(0, alphabet, size=n).tolist()
    return ref, hyp


# (seed, len_ref, len_hyp, alphabet) of the fixture tests/golden/edit_distance.json: alphabet <= 5, lengths 0 .. 70
GOLDEN_SPECS = ([(0, 0, 0, 2), (1, 0, 9, 3), (2, 11, 0, 3), (3, 64, 70, 5), (4, 65, 63, 5), (5, 1, 1, 2), (6, 1, 1, 1),
                 (7, 64, 64, 2), (8, 63, 65, 3), (9, 70, 70, 4)]
                + [(10 + s, (7 * s) % 41, (11 * s + 3) % 37, 2 + s % 4) for s in range(26)])

REF_EDGES = (0, 1, 63, 64, 65, 127, 128, 129, 200)
HYP_EDGES = (0, 1, 2, 63, 64, 65, 300)


class Case:
    """one call: refs[b] and hyps[b][k] (lists of ints); dev_ref_len / dev_hyp_len are what the device is told (None:
    the true lengths) -- the yardstick runs on the clamped ones; L, U: the rows' widths"""

    def __init__(self, name, refs, hyps, L=None, U=None, dev_ref_len=None, dev_hyp_len=None, cap=None):
        self.name, self.refs, self.hyps = name, refs, hyps
        self.B, self.N = len(refs), len(hyps[0]) if hyps else 1
        assert all(len(h) == self.N for h in hyps)
        self.L = L if L is not None else max([len(h) for hs in hyps for h in hs] + [1])
        self.U = U if U is not None else max([len(r) for r in refs] + [1])
        self.dev_ref_len = dev_ref_len if dev_ref_len is not None else [len(r) for r in refs]
        self.dev_hyp_len = dev_hyp_len if dev_hyp_len is not None else [[len(h) for h in hs] for hs in hyps]
        self.cap = cap  # GTNX_EDIT_DISTANCE_SCRATCH_BYTES for the call, or None

    def __repr__(self):
        return self.name

    def arrays(self, seed=0, pad_l=3, pad_u=5):
        """(hyp [B, N, L + pad_l], hyp_len [B, N], ref [B, U + pad_u], ref_len [B]) int32: behind every length tokens of
        the row's own alphabet (reading them would change the answer), behind the widths guard columns"""
        rng = np.random.RandomState(1000 + seed)
        hyp = np.zeros((self.B, self.N, self.L + pad_l), np.int64)
        ref = np.zeros((self.B, self.U + pad_u), np.int64)
        for b in range(self.B):
            pool = np.array(list(self.refs[b]) + [t for h in self.hyps[b] for t in h] + [0], np.int64)
            ref[b] = pool[rng.randint(0, len(pool), size=ref.shape[1])]
            ref[b, :len(self.refs[b])] = self.refs[b]
            for k in range(self.N):
                hyp[b, k] = pool[rng.randint(0, len(pool), size=hyp.shape[2])]
                hyp[b, k, :len(self.hyps[b][k])] = self.hyps[b][k]
        return (hyp.astype(np.int32), np.array(self.dev_hyp_len, np.int32).reshape(self.B, self.N),
                ref.astype(np.int32), np.array(self.dev_ref_len, np.int32).reshape(self.B))

    def pairs(self):
        """(b, k, ref tokens, hyp tokens) at the lengths the kernel uses: what the device is told, clamped; a row the
        device is told to read beyond its tokens is read as arrays() filled it"""
        hyp, hl, ref, rl = self.arrays()
        for b in range(self.B):
            m = min(max(int(rl[b]), 0), self.U)
            for k in range(self.N):
                n = min(max(int(hl[b, k]), 0), self.L)
                yield b, k, ref[b, :m].astype(np.int64), hyp[b, k, :n].astype(np.int64)


def _edges_case(alphabet):
    """every reference length at a block edge against every hypothesis length at a chunk edge: B = 9, N = 7"""
    rng = np.random.RandomState(alphabet)
    refs, hyps = [], []
    for bi, m in enumerate(REF_EDGES):
        ref = rng.randint(0, alphabet, size=m).tolist()
        refs.append(ref)
        hyps.append([edited(ref, rng, n, alphabet) if (bi + ki) % 2 and m else rng.randint(0, alphabet, size=n).tolist()
                     for ki, n in enumerate(HYP_EDGES)])
    return Case(f"edges-a{alphabet}", refs, hyps)


def _random_case(name, seed, B, N, max_m, max_n, alphabet, **kw):
    rng = np.random.RandomState(seed)
    refs, hyps = [], []
    for b in range(B):
        ref = rng.randint(0, alphabet, size=int(rng.randint(0, max_m + 1))).tolist()
        row = []
        for k in range(N):
            n = int(rng.randint(0, max_n + 1))
            row.append(edited(ref, rng, n, alphabet) if (b + k) % 2 and ref else rng.randint(0, alphabet, size=n).tolist())
        refs.append(ref)
        hyps.append(row)
    return Case(name, refs, hyps, **kw)


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """every call test_edit_distance_gpu.py launches and judges by the table"""
    rng = np.random.RandomState(7)
    cases = [_edges_case(2), _edges_case(5), _edges_case(1000)]
    # identical sequences across a block edge
    same = [rng.randint(0, 4, size=m).tolist() for m in (64, 65, 128, 130)]
    cases.append(Case("identical", same, [[s] for s in same]))
    # one token everywhere: the longest carry chains of the add
    cases.append(Case("all-equal", [[7] * 129, [7] * 64, [7] * 200, [7] * 65], [[[7] * 64], [[7] * 129], [[7] * 200],
                                                                                 [[7] * 300]]))
    # hyp = ref shifted by one position: the best path crosses every block edge
    r = rng.randint(0, 50, size=200).tolist()
    cases.append(Case("shifted", [r, r], [[r[1:] + [51]], [[51] + r[:-1]]]))
    # nothing in common: dist = max(m, n)
    cases.append(Case("disjoint", [rng.randint(0, 5, size=m).tolist() for m in (70, 129, 3)],
                      [[rng.randint(10, 15, size=n).tolist()] for n in (129, 70, 3)]))
    cases.append(Case("one-empty", [[], [1, 2, 3], []], [[[4, 5]], [[]], [[]]]))
    # any int32 is a token
    ext = [-1, INT_MIN, INT_MAX, 0]
    er = [ext[i] for i in rng.randint(0, 4, size=70)]
    cases.append(Case("extreme-tokens", [er, er[:5]], [[[ext[i] for i in rng.randint(0, 4, size=66)], er[3:] + [-1]],
                                                       [[INT_MIN], [INT_MAX, -1, INT_MIN]]]))
    cases.append(_random_case("B1-N1", 11, 1, 1, 90, 90, 3))
    cases.append(_random_case("B5-N3", 12, 5, 3, 140, 100, 4))
    cases.append(_random_case("B70-N1", 13, 70, 1, 70, 80, 3))
    cases.append(_random_case("B70-N3", 14, 70, 3, 40, 50, 5))
    # device lengths outside the widths: -3 counts as 0, L + 5 as L (U + 5 as U)
    lies = _random_case("clamped-lengths", 15, 3, 2, 70, 66, 3)
    lies.dev_hyp_len = [[-3, lies.L + 5], [len(lies.hyps[1][0]), -3], [lies.L + 5, lies.L + 5]]
    lies.dev_ref_len = [lies.U + 5, -3, len(lies.refs[2])]
    cases.append(lies)
    # more than eight blocks of reference rows (the walk sums its popcounts across the whole wave from there)
    big = [rng.randint(0, 3, size=m).tolist() for m in (600, 530)]
    cases.append(Case("ten-blocks", big, [[edited(big[0], rng, 500, 3), rng.randint(0, 3, size=40).tolist()],
                                          [rng.randint(0, 3, size=450).tolist(), edited(big[1], rng, 560, 3)]]))
    # the walk's scratch beyond the (lowered) cap: 15 pairs of 16 * 100 * 3 bytes each in slices of two
    cases.append(_random_case("sliced", 17, 5, 3, 140, 100, 4, L=100, U=140, cap=2 * 16 * 100 * 3 + 100))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def expected(case):
    """(dist [B, N], ops [B, N, 3]) int32 by the table: computed once per case and shared"""
    dist = np.zeros((case.B, case.N), np.int32)
    ops = np.zeros((case.B, case.N, 3), np.int32)
    for b, k, ref, hyp in case.pairs():
        dist[b, k], ops[b, k], _ = distance_ops(ref, hyp)
    dist.setflags(write=False)
    ops.setflags(write=False)
    return dist, ops
