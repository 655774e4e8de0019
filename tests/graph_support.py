"""Test helper: what the tests of built graphs share -- a local-map crop of a cloud with an obstacle that the global
map lacks, and the reference's invariants of a built graph.  Test code only."""
import numpy as np


def obs_crop(cloud, centre, half, box=None):
    m = (np.abs(cloud[:, 0] - centre[0]) < half) & (np.abs(cloud[:, 1] - centre[1]) < half)
    obs = cloud[m].copy()
    if box is not None:  # raise a block of points: an obstacle that was not in the global map
        b = (np.abs(obs[:, 0] - box[0]) < box[2]) & (np.abs(obs[:, 1] - box[1]) < box[2])
        obs[b, 2] += np.float32(1.0) * (np.arange(b.sum()) % 2).astype(np.float32)
    return obs


def graph_invariants(g, expand_dist):
    assert (g.state != -1).all() and (np.diff(g.rowptr) >= 1).all()       # cleanGraph post-condition
    assert (g.dist < 2.5 * expand_dist).all()                              # trg.cpp:279
    nz = g.w[g.w != 0]
    assert ((nz >= 0.1) & (nz <= 0.4761)).all()                            # trg.cpp:359-363
    src = np.repeat(np.arange(g.V, dtype=np.int64), np.diff(g.rowptr))
    key = src * g.V + g.col
    rev = g.col.astype(np.int64) * g.V + src
    assert np.array_equal(np.sort(key), np.sort(rev))                      # edges are symmetric
    assert np.unique(key).size == key.size                                 # wireEdge's dedupe
    # nodes are at least robot_size apart only in a statistical sense (merge test is against the
    # NEAREST node); what must hold exactly: every edge length equals the fp32 node distance
    d = np.sqrt(((g.xyz[src, 0] - g.xyz[g.col, 0]) ** 2 + (g.xyz[src, 1] - g.xyz[g.col, 1]) ** 2))
    assert np.abs(d - g.dist).max() < 1e-5
