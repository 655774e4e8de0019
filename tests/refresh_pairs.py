"""Test helper: pairs of graphs for the tests of the cost-field refresh -- an earlier graph A, the current graph B, the
node map new2old from B's ids to A's (-1: a node A did not have) and the sources as ids of A -- each pair at the
smallest size at which one piece of the refresh can go wrong.  Both the CPU test of tests/refresh_ref.py and the GPU
test of the engine take them from here.  Test code only."""
from collections import namedtuple

import numpy as np

import field_graphs as fg

F32 = np.float32

# a, b: fg.FieldGraph; new2old: int32 over b's nodes; sources: ids of a, one per field (the GPU test takes the first
# for m == 1); sets: None, or the source sets as lists of ids of a
Pair = namedtuple("Pair", "a b new2old sources sets", defaults=(None,))


def edges_of(g):
    """(src, dst, w, dist) per edge, in CSR order."""
    V = len(g.state)
    return np.repeat(np.arange(V), np.diff(g.rowptr)), g.col.copy(), g.w.copy(), g.dist.copy()


def rebuilt(g, keep=None, extra=(), w=None, dist=None, state=None):
    """g with only the edges of mask `keep`, then the edges `extra` (src, dst, w, dist) pushed after them, other
    weights / dists / states where given."""
    s, d, ww, dd = edges_of(g)
    ww = ww if w is None else np.asarray(w, F32)
    dd = dd if dist is None else np.asarray(dist, F32)
    keep = np.ones(s.shape[0], bool) if keep is None else keep
    xs = [(a, b, c, e) for a, b, c, e in extra]
    s = np.concatenate([s[keep], np.array([x[0] for x in xs], np.int64)])
    d = np.concatenate([d[keep], np.array([x[1] for x in xs], np.int64)])
    ww = np.concatenate([ww[keep], np.array([x[2] for x in xs], F32)])
    dd = np.concatenate([dd[keep], np.array([x[3] for x in xs], F32)])
    return fg.from_edges(len(g.state), s, d, ww, dd, state=g.state if state is None else state, pos=g.pos)


def without_link(g, u, v):
    """g without the edges between u and v, either way."""
    s, d, _, _ = edges_of(g)
    return rebuilt(g, keep=~(((s == u) & (d == v)) | ((s == v) & (d == u))))


def identity(g):
    return np.arange(len(g.state), dtype=np.int32)


def renumbered(g, keep_nodes, n_new, new_edges, rng):
    """g with only the nodes of `keep_nodes` (a mask), n_new nodes more (ids after them) joined by `new_edges`
    ((src, dst, w, dist) in the ids before the permutation: kept nodes keep their order, new ones follow), then all
    ids permuted at random -> (graph, new2old)."""
    V = len(g.state)
    old_ids = np.flatnonzero(keep_nodes)
    dense = np.full(V, -1, np.int64)
    dense[old_ids] = np.arange(old_ids.shape[0])
    Vn = old_ids.shape[0] + n_new
    s, d, w, dist = edges_of(g)
    ok = keep_nodes[s] & keep_nodes[d]
    s, d, w, dist = dense[s[ok]], dense[d[ok]], w[ok], dist[ok]
    if new_edges:
        xs = np.array([(a, b) for a, b, _, _ in new_edges], np.int64)
        s = np.concatenate([s, xs[:, 0]])
        d = np.concatenate([d, xs[:, 1]])
        w = np.concatenate([w, np.array([x[2] for x in new_edges], F32)])
        dist = np.concatenate([dist, np.array([x[3] for x in new_edges], F32)])
    perm = rng.permutation(Vn)  # the id a node gets
    state = np.zeros(Vn, np.int32)
    state[perm[:old_ids.shape[0]]] = g.state[old_ids]
    new2old = np.full(Vn, -1, np.int32)
    new2old[perm[:old_ids.shape[0]]] = old_ids
    return fg.from_edges(Vn, perm[s], perm[d], w, dist, state=state, pos=fg.square_positions(Vn)), new2old


def chain_pair(cut):
    """A symmetric unit chain of 1 000 and the same chain cut between 899 and 900; cut: full -> cut, else back."""
    V = 1000
    a = np.arange(V - 1)
    src = np.stack([a, a + 1], axis=1)
    dst = np.stack([a + 1, a], axis=1)
    full = fg.from_edges(V, src, dst, np.zeros(2 * (V - 1), F32), np.ones(2 * (V - 1), F32))
    broken = without_link(full, 899, 900)
    # every source upstream of the cut: what is relabelled is the 100 nodes past it, in every field
    return Pair(full, broken, identity(full), [0, 3, 450]) if cut else Pair(broken, full, identity(full), [0, 3, 450])


def random_pair(seed=7, protect=()):
    """The random family at V ~ 2 000: 5 % of the nodes deleted, 5 % new ones with edges, weights raised and lowered,
    ids permuted."""
    rng = np.random.default_rng(seed)
    a = fg.with_positions(fg.random_graph(np.random.default_rng(100), 40, 50))
    V = len(a.state)
    sources = [0, 11, V // 2 + 5]
    keep = np.ones(V, bool)
    gone = rng.choice(V, size=V // 20, replace=False)
    keep[gone] = False
    keep[sources] = True
    keep[list(protect)] = True
    s, d, w, dist = edges_of(a)
    touched = rng.choice(s.shape[0], size=s.shape[0] // 20, replace=False)
    w = w.copy()
    w[touched] = (w[touched] * rng.choice(np.array([0.0, 0.5, 2.0, 4.0], F32), size=touched.shape[0])).astype(F32)
    a2 = rebuilt(a, w=w)
    n_keep, n_new = int(keep.sum()), V // 20
    new_edges = []
    for j in range(n_new):
        for _ in range(3):
            o = int(rng.integers(0, n_keep + n_new))
            wd = (F32(rng.choice([0.0, 0.4])), F32(rng.choice([0.0, 1e-9, 0.45, 150.0])))
            new_edges.append((n_keep + j, o, *wd))
            new_edges.append((o, n_keep + j, *wd))
    b, new2old = renumbered(a2, keep, n_new, new_edges, rng)
    return Pair(a, b, new2old, sources)


def lattice_pair():
    """A 24 x 17 lattice of equal edge costs -- every key has many supporters, the smallest decides -- and the same
    with a block of nodes made Invalid (their in-edges are never relaxed) and two weights raised on least walks."""
    a = fg.lattice(24, 17)
    state = a.state.copy()
    for iy in range(5, 11):
        state[iy * 24 + 6:iy * 24 + 13] = fg.INVALID
    s, d, w, dist = edges_of(a)
    w = w.copy()
    w[(s == 1) & (d == 2)] = 0.5
    w[(s == 24) & (d == 48)] = 0.5
    return Pair(a, rebuilt(a, w=w, state=state), identity(a), [0, 24 * 17 - 1, 24 * 8 + 2])


def plateau_pair():
    """Sub-ulp costs: in B the added edge 0 -> 4 lowers node 1's cost (1e-6 in one hop -> 3e-7 in three), node 2's
    cost 1 000 absorbs either (the same bits), and its hops go from 2 to 4, as do the hops of everything behind it.
    A single warm pass on (cost, hops) keeps (1 000, 2) at node 2: no extension of node 1's new key improves it."""
    e = [(0, 1, 0.0, 1e-6), (1, 2, 0.0, 1000.0), (2, 3, 0.0, 1.0), (3, 6, 0.0, 2.0), (4, 5, 0.0, 1e-7),
         (5, 1, 0.0, 1e-7), (2, 7, 0.0, 0.0), (7, 3, 0.0, 0.5), (6, 0, 0.0, 1.0)]
    a = fg.from_edges(8, *zip(*e))
    b = rebuilt(a, extra=[(0, 4, 0.0, 1e-7)])
    return Pair(a, b, identity(a), [0, 4, 0])


def saturating_pairs():
    """+inf folds: the chain without its link 3 -> 4, the branch without 2 -> 10 (node 10 then hangs on the longer
    +inf walk) and without 0 -> 7."""
    c = fg.saturating_chain()
    br = fg.saturating_branch()
    s, d, _, _ = edges_of(br)
    b2 = rebuilt(br, keep=~(((s == 2) & (d == 10)) | ((s == 0) & (d == 7))))
    return {"saturating_chain": Pair(c, without_link(c, 3, 4), identity(c), [0, 1, 0]),
            "saturating_branch": Pair(br, b2, identity(br), [0, 7, 2])}


def star_pair():
    """One hub with a row of 30 000 leaves; the source is a leaf, and in B its edge to the hub is gone: the hub is
    reached over the ring, every key changes, and the hub's whole row is seeded and relaxed again."""
    a = fg.star(30000)
    s, d, _, _ = edges_of(a)
    return Pair(a, rebuilt(a, keep=~((s == 1) & (d == 0))), identity(a), [1, 0, 15001])


def invalid_pair():
    """Invalid nodes, one of them a source (it is expanded, never entered); B makes more nodes Invalid, revalidates
    one and drops edges."""
    a = fg.with_positions(fg.random_graph(np.random.default_rng(31), 30, 4))
    inv = np.flatnonzero(a.state == fg.INVALID)
    rng = np.random.default_rng(32)
    state = a.state.copy()
    state[inv[1]] = 0
    ok = np.flatnonzero(a.state != fg.INVALID)
    state[rng.choice(ok[ok > 3], size=6, replace=False)] = fg.INVALID
    keep = rng.random(len(a.col)) > 0.05
    return Pair(a, rebuilt(a, keep=keep, state=state), identity(a), [int(inv[0]), 0, int(inv[2])])


def set_pair():
    """Two source sets on the random pair's graphs, one with a member named twice."""
    sets = [[0, 11, 0, 57], [1005, 1009]]
    p = random_pair(seed=9, protect=sets[0] + sets[1])
    return Pair(p.a, p.b, p.new2old, [0, 1005], sets=sets)


def all_pairs():
    """name -> Pair, every pair of the refresh tests but the identity ones (which any graph gives)."""
    out = {"chain_cut": chain_pair(True), "chain_join": chain_pair(False), "random": random_pair(),
           "lattice": lattice_pair(), "plateau": plateau_pair(), "star": star_pair(), "invalid": invalid_pair()}
    out.update(saturating_pairs())
    return out


def new_sources(pair):
    """The pair's sources as ids of b: the first node of b that names each."""
    first = {}
    for v, o in enumerate(pair.new2old.tolist()):
        first.setdefault(o, v)
    return [first[int(s)] for s in pair.sources]


def new_sets(pair):
    first = {}
    for v, o in enumerate(pair.new2old.tolist()):
        first.setdefault(o, v)
    return [[first[int(s)] for s in members] for members in pair.sets]
