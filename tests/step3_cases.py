"""Test data: builds with expandGraph's step 3 on (trg.cpp:429-444, indoor.yaml's parameters) on ROUGH ground, where
it matters -- parent edges fail, nodes are rescued by an edge to a neighbour, weights are non-zero -- and what the
oracle must show on each of them before a GPU test may rest on it.  Test code only; nothing here needs a GPU.

On the flat indoor fixture no parent edge fails at all (test_step3_cases_cpu.py keeps that on record), so the rescue
search of k_level_spec3, the rescue wait of k_level_resolve and k_node_cov's pass over a node without a creating edge
never decide anything there.

rescue_census() reads the oracle's wireEdge trace (Oracle.set_trace).  The ids of the graph before cleanGraph are
creation ids, and a trace record is (src, dst, status, ...) of one EVALUATED wireEdge call, in call order:
    parent of X        the src of the first record with dst == X and src < X (wireEdge(node, new_node), trg.cpp:425:
                       the first call that names X); its status is the parent edge's
    depth(X)           depth(parent) + 1, depth(0) = 0: X is a candidate of engine level depth(X) - 1 (level 0 expands
                       the root)
    rescued            X is not Invalid before cleanGraph although its parent edge failed (status != 0)
    ... by a pre-level node      some status-0 record has src == X and depth(dst) < depth(X)
    ... by its level only        otherwise, and some status-0 record has src == X, depth(dst) == depth(X), dst < X
    chain              rescued by its level only, and every such same-level rescuer is itself rescued
    trap               an Invalid node with a sound edge (edgeRisk status 0) to an earlier candidate of its level,
                       within expand_dist, that ended Invalid as well: a rescue search that forgets the rescuer's
                       own fate makes it a valid node
    gate band          records whose slope gate (trg.cpp:269-274) lies within a relative band of its threshold,
                       | |dz| robot_size / (height_threshold dist) - 1 | < band; 1e-4 is the engine's gate_margin,
                       inside which the device leaves the gate to the host and a step-3 build declines
Only the records of X's own step 3 count as rescues: the run of records with src == X that follows X's creating
call.  (Later, when X is expanded, a sample that lands within robot_size of an older node makes another record with
src == X, up to expand_dist + robot_size away; X was a valid node long before.)
"""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name cloud overrides seed start")
# cloud: a key of clouds(); overrides: changes to oracle_api.INDOOR; seed: sampler seed (table_bits 16)

START_R160, START_R160_B, START_R120 = [8.0, 8.0, 0.0], [4.0, 12.0, 0.0], [6.0, 6.0, 0.0]
TABLE_BITS = 16


def r160(synth):
    """16 m x 16 m of the terrain of conftest's mountain_small."""
    return synth.mountain_cloud(160, 160, seed=11, amplitude=5.0, wavelength=14.0)


def clouds(synth):
    return {"R160": r160(synth), "R120": synth.mountain_cloud(120, 120, seed=3, amplitude=4.0, wavelength=10.0)}


CASES = [
    Case("r160_s7", "R160", {}, 7, START_R160),
    Case("r160_s21", "R160", {}, 21, START_R160),
    # the seeds a route moves to when it declines on s7 for a reason no trace shows (a tie among samples, an
    # uncertain gate on a speculative edge the reference never evaluates)
    Case("r160_s5", "R160", {}, 5, START_R160),
    Case("r160_s13", "R160", {}, 13, START_R160),
    Case("r160_s33", "R160", {}, 33, START_R160),
    Case("r160_s7_start_b", "R160", {}, 7, START_R160_B),
    Case("r160_S64_s7", "R160", {"sample_num": 64}, 7, START_R160),
    Case("r120_s21", "R120", {}, 21, START_R120),
]
BY_NAME = {c.name: c for c in CASES}
CHAIN_CASES = ("r160_s21", "r160_s13", "r160_s33")  # at least one of the suite's cases must hold a chain
TRAP_CASE = "r160_s7_start_b"  # ... and this one a trap

# Natural nearest-node ties in a step-3 build: 16 sampling directions on nearly level ground put the nodes on a few
# lattices (test_gpu_parity.test_natural_node_ties_settled_like_the_reference).  Used for one decline only.
TIES = dict(cloud_args=dict(nx=160, ny=160, seed=5, amplitude=0.3), overrides={"sample_num": 8}, seed=33,
            table_bits=4, start=[8.0, 8.0, 0.0])


def ties_cloud(synth):
    a = TIES["cloud_args"]
    return synth.mountain_cloud(a["nx"], a["ny"], seed=a["seed"], amplitude=a["amplitude"])


def params(oa, case):
    return dict(oa.INDOOR, **case.overrides)


def step3_is_on(prm):
    """trg.cpp:429, in the reference's arithmetic (float members, a double literal)."""
    ed, rs = np.float32(prm["expand_dist"]), np.float32(prm["robot_size"])
    return float(ed - rs) < 0.25 * float(ed)


def build_oracle(oa, prm, cloud, start, seed, *, f64=False, trace=False, table_bits=TABLE_BITS):
    o = oa.Oracle(**prm)
    o.set_sampler(seed, 0, table_bits)
    o.set_cov_f64(f64)
    o.set_trace(trace)
    o.set_global_map(cloud)
    assert o.init_graph(start), "the oracle builds no graph"
    return o


# ---- the census ---------------------------------------------------------------------------------------------------
def rescue_census(oracle_with_trace, preclean_graph, prm):
    """What the build's trace shows, see the module's docstring.  -> dict"""
    tr = oracle_with_trace.trace()
    src, dst, status = tr["src"].astype(np.int64), tr["dst"].astype(np.int64), tr["status"]
    pre = preclean_graph
    V = pre.V
    assert np.array_equal(pre.cid, np.arange(V)), "ids before cleanGraph are creation ids"
    n = src.shape[0]
    # the creating call of every node but the root
    down = np.flatnonzero(src < dst)
    who, first = np.unique(dst[down], return_index=True)
    assert np.array_equal(who, np.arange(1, V)), "every created node has a creating call in the trace"
    rec_of = np.zeros(V, np.int64)
    rec_of[1:] = down[first]
    parent = np.zeros(V, np.int64)
    pstatus = np.zeros(V, np.int32)
    parent[1:] = src[rec_of[1:]]
    pstatus[1:] = status[rec_of[1:]]
    depth = np.zeros(V, np.int64)
    for x in range(1, V):
        depth[x] = depth[parent[x]] + 1
    assert (np.diff(depth) >= 0).all(), "creation order is breadth first"
    # X's own step 3: the records with src == X right behind its creating call
    own = np.zeros(n, bool)
    run_end = np.empty(n + 1, np.int64)  # run_end[i]: first j >= i with src[j] != src[i]
    run_end[n] = n
    for i in range(n - 1, -1, -1):
        run_end[i] = run_end[i + 1] if i + 1 < n and src[i + 1] == src[i] else i + 1
    for x in range(1, V):
        i = rec_of[x] + 1
        if i < n and src[i] == x:
            own[i:run_end[i]] = True
    ok = own & (status == 0)
    assert (dst[ok] < src[ok]).all()  # a neighbour call goes to a node that exists
    invalid = pre.state == -1
    assert not invalid[dst[ok]].any()  # trg.cpp:436-439
    rescued = ~invalid & (pstatus != 0)
    rescued[0] = False
    by_pre = np.zeros(V, bool)
    by_level = np.zeros(V, bool)
    by_pre[src[ok & (depth[dst] < depth[src])]] = True
    same = ok & (depth[dst] == depth[src])
    by_level[src[same]] = True
    pre_rescued = rescued & by_pre
    level_rescued = rescued & ~by_pre & by_level
    assert np.array_equal(rescued, pre_rescued | level_rescued), "a valid node has an edge"
    # a chain: none of the same-level rescuers has a parent edge of its own
    unrescued_helper = np.zeros(V, bool)
    unrescued_helper[src[same & ~rescued[dst]]] = True
    chain = level_rescued & ~unrescued_helper
    # An Invalid node with a sound edge to an EARLIER candidate of its level that ended Invalid too: the reference
    # never calls that pair (trg.cpp:436-439), k_level_spec3 lists it and k_level_resolve must not count it
    traps = 0
    r2 = np.float32(prm["expand_dist"]) * np.float32(prm["expand_dist"])
    bad = np.flatnonzero(invalid)
    for x in bad:
        dx, dy = pre.xyz[bad, 0] - pre.xyz[x, 0], pre.xyz[bad, 1] - pre.xyz[x, 1]
        near = bad[(bad < x) & (depth[bad] == depth[x]) & (dx * dx + dy * dy <= r2)]
        if near.size:
            st = oracle_with_trace.edge_risk(np.repeat(pre.xyz[x][None], near.size, axis=0), pre.xyz[near])[0]
            traps += int((st == 0).any())
    # weights
    deg = np.diff(pre.rowptr)
    row = np.repeat(np.arange(V), deg)
    nonzero_on_rescued = int(((pre.w != 0) & rescued[row]).sum())
    # the slope gates of every evaluated call
    z = pre.xyz[:, 2].astype(np.float64)
    dz = np.abs(z[src] - z[dst])
    dist = tr["dist"].astype(np.float64)
    thr = float(np.float32(prm["height_threshold"])) * dist
    ratio = np.divide(dz * float(np.float32(prm["robot_size"])), thr, out=np.full(n, np.inf), where=thr > 0)
    return dict(
        Vpre=V, failed=int((pstatus[1:] != 0).sum()), rescued=int(rescued.sum()),
        by_pre=int(pre_rescued.sum()), by_level=int(level_rescued.sum()), chains=int(chain.sum()),
        invalid=int(invalid.sum()), nonzero_pre=int((pre.w != 0).sum()), nonzero_on_rescued=nonzero_on_rescued,
        level_only_depths=sorted(set(int(d) for d in depth[level_rescued])), max_depth=int(depth.max()),
        max_valid_depth=int(depth[~invalid].max()),
        gates_1e3=int((np.abs(ratio - 1.0) < 1e-3).sum()), gates_1e4=int((np.abs(ratio - 1.0) < 1e-4).sum()),
        invalid_rescuer_traps=traps)


def check_preconditions(c, clean_graph):
    """What every case a GPU test uses must show.  Conditions, not measurements."""
    assert c["by_pre"] >= 10, c
    assert c["by_level"] >= 5, c
    assert int((clean_graph.w != 0).sum()) >= 1000, int((clean_graph.w != 0).sum())
    assert c["nonzero_on_rescued"] >= 50, c
    assert c["invalid"] >= 20, c
    assert c["gates_1e4"] == 0, c


def stall_level(census):
    """The engine level at which the stall hooks are set: that of the first depth >= 5 at which a node is rescued by
    its level only (depth d is decided in level d - 1)."""
    return next(d for d in census["level_only_depths"] if d >= 5) - 1


_MEMO = {}


def vetted(oa, synth, name):
    """The case's cloud, parameters, the two oracles' graphs and its census, built once per process.
    -> dict(case, cloud, prm, pre, clean, wpre, wclean, counters, census)"""
    if name in _MEMO:
        return _MEMO[name]
    case = BY_NAME[name]
    if "clouds" not in _MEMO:
        _MEMO["clouds"] = clouds(synth)
    cloud = _MEMO["clouds"][case.cloud]
    prm = params(oa, case)
    assert step3_is_on(prm)
    o = build_oracle(oa, prm, cloud, case.start, case.seed, trace=True)
    w = build_oracle(oa, prm, cloud, case.start, case.seed, f64=True)
    pre, clean = o.graph(1), o.graph(0)
    rec = dict(case=case, cloud=cloud, prm=prm, pre=pre, clean=clean, wpre=w.graph(1), wclean=w.graph(0),
               counters=o.counters(), census=rescue_census(o, pre, prm))
    o.close()
    w.close()
    _MEMO[name] = rec
    return rec
