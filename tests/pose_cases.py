"""Test helper: the poses of the pose-link tests and their reference -- the plain loop over all nodes of DESIGN.md
section 2, "Pose links", over three probes (is_collision, nearest_z, edge_risk of an Engine or of the oracle).
Test code only."""
import numpy as np

F32 = np.float32
INVALID = -1
# map fixture -> (parameters' name in oracle_api, start, generator seed, conditions() that seed does NOT show).  The
# seeds were chosen with the oracle on the CPU, the first of 1, 2, ... that shows the most: the terrain shows all six
# conditions; the indoor map's floor is flat, so a pose that is not itself in collision meets no slope gate there and
# always keeps some link (seeds 1..11 tried).
MAPS = {"mountain_small": ("MOUNTAIN", [15.0, 15.0, 0.0], 1, ()),
        "indoor_small": ("INDOOR", [1.5, 1.5, 0.0], 9, ("candidates but no links", "rejected at the slope gate"))}
N_POSES = 64


def poses(cloud, g, seed, robot_size, n=N_POSES):
    """n positions from one seeded stream, a quarter each: node positions themselves, edge midpoints, uniform draws in
    the map's box, and draws within robot_size of a raised map point (an indoor wall; on terrain, the upper tenth of
    the elevations) -> (n, 2) float32."""
    rng = np.random.default_rng(seed)
    q = n // 4
    xy = g.xyz[:, :2]
    nodes = xy[rng.choice(g.V, q, replace=False)]
    eu = np.repeat(np.arange(g.V), np.diff(g.rowptr))
    k = rng.choice(g.E, q, replace=False)
    mid = (xy[eu[k]] + xy[g.col[k]]) * F32(0.5)
    lo, hi = cloud[:, :2].min(0), cloud[:, :2].max(0)
    box = rng.uniform(lo, hi, size=(q, 2))
    high = cloud[cloud[:, 2] >= np.quantile(cloud[:, 2], 0.9)]
    w = high[rng.choice(high.shape[0], n - 3 * q, replace=False), :2]
    ang, rad = rng.uniform(0, 2 * np.pi, w.shape[0]), robot_size * np.sqrt(rng.uniform(0, 1, w.shape[0]))
    wall = w + np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    return np.concatenate([nodes, mid, box, wall]).astype(F32)


def reference(probes, g, xy, radius, collision_threshold):
    """The definition, pose by pose over ALL nodes.  probes: an object with is_collision(xy, threshold=) ->
    (flag, ...), nearest_z(xy) and edge_risk(p1, p2) -> (status, n_pts, weight, dist), all on the global map.
    -> list of dicts: status, z, n_candidates, n_links, nodes, weight, dist (links sorted by (dist bits, node)), and
    `rejected`, the edge statuses of the candidates that are no links."""
    xy = np.ascontiguousarray(xy, F32).reshape(-1, 2)
    hit = probes.is_collision(xy, threshold=collision_threshold)[0]
    z = probes.nearest_z(xy)
    out = []
    for k in range(xy.shape[0]):
        one = {"status": int(hit[k] != 0), "z": F32(z[k]), "n_candidates": 0, "n_links": 0,
               "nodes": np.empty(0, np.int32), "weight": np.empty(0, F32), "dist": np.empty(0, F32), "rejected": []}
        out.append(one)
        if hit[k]:
            continue
        dx = xy[k, 0] - g.xyz[:, 0]
        dy = xy[k, 1] - g.xyz[:, 1]
        d = np.sqrt(dx * dx + dy * dy)  # float32 throughout, each operation rounded
        assert d.dtype == np.float32
        cand = np.flatnonzero((g.state != INVALID) & (d <= F32(radius)))
        one["n_candidates"] = int(cand.size)
        here, away = cand[d[cand] == 0], cand[d[cand] != 0]
        links = [(0, int(v), F32(0), F32(0)) for v in here]
        if away.size:
            p1 = np.tile(np.array([xy[k, 0], xy[k, 1], z[k]], F32), (away.size, 1))
            st, _, w, dd = probes.edge_risk(p1, g.xyz[away])
            one["rejected"] = st[st != 0].tolist()
            links += [(int(dd[i:i + 1].view(np.uint32)[0]), int(away[i]), w[i], dd[i]) for i in np.flatnonzero(st == 0)]
        links.sort(key=lambda t: (t[0], t[1]))
        one["n_links"] = len(links)
        one["nodes"] = np.array([t[1] for t in links], np.int32)
        one["weight"] = np.array([t[2] for t in links], F32)
        one["dist"] = np.array([t[3] for t in links], F32)
    return out


def conditions(ref):
    """Which of the situations the test must meet the reference shows -> dict of booleans."""
    return {"a pose in collision": any(r["status"] == 1 for r in ref),
            "candidates but no links": any(r["n_candidates"] > 0 and r["n_links"] == 0 for r in ref),
            "rejected for segment collision": any(2 in r["rejected"] for r in ref),
            "rejected at the slope gate": any(1 in r["rejected"] for r in ref),
            "at least 3 links": any(r["n_links"] >= 3 for r in ref),
            "a link at distance 0": any(r["n_links"] and r["dist"][0] == 0 for r in ref)}


class OracleProbes:
    """The oracle's probes with the Engine's call shapes."""

    def __init__(self, o):
        self.o = o

    def is_collision(self, xy, threshold):
        return self.o.is_collision(xy, 0, threshold)

    def nearest_z(self, xy):
        return self.o.nearest_z(xy, 0)

    def edge_risk(self, p1, p2):
        return self.o.edge_risk(p1, p2, 0)
