"""Host builders of the token lattices `torch_loss.ctc_lattice_score` takes (plain Python and numpy, no GPU needed).

A lattice is `(arcs, num_nodes)` or `(arcs, num_nodes, weights)`: `arcs` int32 [A, 3] rows of (src, dst, label) with
0 <= src < dst < num_nodes, node 0 the start and node num_nodes - 1 the accepting one, `weights` float32 [A].
`pack_lattices` pads a list of them into the arrays the device entry points read.
"""
import numpy as np


def _sorted(arcs, weights=None):
    """the arcs by (dst, src, label); the order the kernel needs is dst alone, the rest makes it reproducible"""
    arcs = np.asarray(arcs, dtype=np.int32).reshape(-1, 3)
    order = np.lexsort((arcs[:, 2], arcs[:, 0], arcs[:, 1]))
    return arcs[order], (None if weights is None else np.asarray(weights, dtype=np.float32).reshape(-1)[order])


def decomposition_lattice(units, pieces, max_piece_len=None):
    """Every decomposition of `units` (a sequence of base symbols) into `pieces` (a mapping from tuples of base symbols
    to labels; a string key counts as the tuple of its characters): one node per offset 0 .. len(units), one arc
    (i, j, pieces[units[i:j]]) per piece that matches at an offset, pieces of up to `max_piece_len` symbols (default: the
    longest key).  Returns (arcs int32 [A, 3] sorted by (dst, src, label), num_nodes).  The lattice of
    examples/learned_decompositions.cpp for "the" over {e, h, t, th, he, the} has six arcs."""
    units = tuple(units)
    table = {tuple(k): int(v) for k, v in pieces.items()}
    longest = max((len(k) for k in table), default=0)
    if max_piece_len is not None:
        longest = min(longest, int(max_piece_len))
    arcs = []
    for j in range(1, len(units) + 1):
        for i in range(max(0, j - longest), j):
            label = table.get(units[i:j])
            if label is not None:
                arcs.append((i, j, label))
    return _sorted(arcs)[0], len(units) + 1


def lattice_from_graph(graph):
    """The lattice of an acyclic acceptor `Graph` with one start and one accepting node: the nodes that lie on a path
    from the start to the accepting node, renumbered topologically (start 0, accepting node last), and the arcs between
    them with their weights.  Returns (arcs int32 [A, 3], num_nodes, weights float32 [A]), sorted by (dst, src, label).
    ValueError: a cycle, an epsilon arc, an arc whose input and output labels differ, not exactly one start and one
    accepting node.  A graph whose accepting node cannot be reached gives two nodes without an arc (the score is -inf)."""
    starts, accepts = graph.start(), graph.accept()
    if len(starts) != 1 or len(accepts) != 1:
        raise ValueError("lattice_from_graph: the graph must have exactly one start and one accepting node")
    src, dst, ilabel, olabel, weight = graph.arcs()
    if (ilabel < 0).any() or (olabel < 0).any():
        raise ValueError("lattice_from_graph: epsilon arcs have no token state")
    if (ilabel != olabel).any():
        raise ValueError("lattice_from_graph: the graph must be an acceptor")
    n = graph.num_nodes()
    out = [[] for _ in range(n)]
    indeg = np.zeros(n, dtype=np.int64)
    for a, (s, d) in enumerate(zip(src.tolist(), dst.tolist())):
        out[s].append(a)
        indeg[d] += 1
    # Kahn's order over every node: what is left over lies on or behind a cycle
    order, ready = [], [v for v in range(n) if indeg[v] == 0]
    while ready:
        v = ready.pop()
        order.append(v)
        for a in out[v]:
            indeg[dst[a]] -= 1
            if indeg[dst[a]] == 0:
                ready.append(int(dst[a]))
    if len(order) != n:
        raise ValueError("lattice_from_graph: the graph has a cycle")
    start, accept = starts[0], accepts[0]
    fwd = np.zeros(n, dtype=bool)
    fwd[start] = True
    for v in order:
        if fwd[v]:
            for a in out[v]:
                fwd[dst[a]] = True
    bwd = np.zeros(n, dtype=bool)
    bwd[accept] = True
    for v in reversed(order):
        bwd[v] = bwd[v] or any(bwd[dst[a]] for a in out[v])
    live = fwd & bwd
    if not live[accept]:
        return np.zeros((0, 3), dtype=np.int32), 2, np.zeros(0, dtype=np.float32)
    # (the accepting node has no live arc leaving it, so it may come last)
    kept = [v for v in order if live[v] and v != accept] + [accept]
    number = {v: i for i, v in enumerate(kept)}
    keep = [a for a in range(len(src)) if live[src[a]] and live[dst[a]]]
    arcs = [(number[int(src[a])], number[int(dst[a])], int(ilabel[a])) for a in keep]
    arcs, weights = _sorted(arcs, np.asarray(weight, dtype=np.float32)[keep])
    return arcs, len(kept), weights


def pack_lattices(lattices):
    """The arrays of a batch of lattices, each `(arcs, num_nodes)` or `(arcs, num_nodes, weights)`: (arcs int32
    [B, A, 3], num_arcs int32 [B], num_nodes int32 [B], weights float32 [B, A]) with A the largest arc count (at least
    1); every lattice's arcs are sorted by dst, rows past num_arcs are zeros, weights not given are zeros."""
    lattices = list(lattices)
    B = len(lattices)
    A = max([1] + [len(np.asarray(l[0]).reshape(-1, 3)) for l in lattices])
    arcs = np.zeros((B, A, 3), dtype=np.int32)
    weights = np.zeros((B, A), dtype=np.float32)
    num_arcs = np.zeros(B, dtype=np.int32)
    num_nodes = np.zeros(B, dtype=np.int32)
    for b, l in enumerate(lattices):
        a, w = _sorted(l[0], l[2] if len(l) > 2 and l[2] is not None else None)
        if w is not None and w.size != len(a):
            raise ValueError("pack_lattices: one weight per arc")
        arcs[b, :len(a)] = a
        if w is not None:
            weights[b, :len(a)] = w
        num_arcs[b] = len(a)
        num_nodes[b] = int(l[1])
    return arcs, num_arcs, num_nodes, weights
