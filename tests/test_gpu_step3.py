"""GPU: expandGraph's step 3 (trg.cpp:429-444) where it decides something -- the rough-ground cases of step3_cases.py,
vetted on the oracle alone by test_step3_cases_cpu.py: parent edges fail, dozens of nodes are rescued by an edge to a
pre-level node or to a node of their own level only (k_level_spec3, the rescue wait of k_level_resolve), a hundred stay
Invalid, thousands of weights are non-zero (k_node_cov passes over the rescued nodes, k_step3_calls orders their rows).

Every route the build can take is compared with the live oracle in the same way (_check): the graphs before and after
cleanGraph by conftest.assert_graph_equal (structure bit for bit, weights within 1e-5, no clamp flip), col and w bit
for bit with the oracle's fp64-covariance witness, and the expansion counters.  A route that must stay on the device
says so, a decline says why.  Each test is one or two builds of at most 1 700 nodes."""
import numpy as np
import pytest

import step3_cases as s3
from conftest import assert_graph_equal

pytestmark = pytest.mark.gpu

WEIGHT_TOL = 1e-5
MAIN = "r160_s7"
REPORT = ("used_device_bfs", "bfs_fallbacks", "bfs_ticket_reruns", "bfs_levels", "bfs_multipass_rows",
          "launches_edge_kernel", "bfs_host_levels", "gate_uncertain", "nn_ties")


def _build(prm, cloud, start, seed, table_bits=s3.TABLE_BITS, **options):
    import trg_planner
    e = trg_planner.Engine(**prm)
    e.set_sampler(seed, table_bits)
    e.set_option("keep_preclean", 1)
    for k, v in options.items():
        e.set_option(k, v)
    e.set_global_map(cloud)
    e.init_graph(start)
    return e


def _build_case(v, **options):
    return _build(v["prm"], v["cloud"], v["case"].start, v["case"].seed, **options)


def _report(route, e):
    st = e.stats()
    print(f"[step3] {route}: " + " ".join(f"{k}={st[k]}" for k in REPORT) + f" fallback_reason={e.fallback_reason!r}")
    return st


def _same_as_witness(g, ref, what):
    assert np.array_equal(g.col, ref.col), f"{what}: col differs from the witness's"
    same = g.w.view(np.uint32) == ref.w.view(np.uint32)
    assert same.all(), f"{what}: w differs from the witness's on {int((~same).sum())} of {g.E} edges, by " \
                       f"{float(np.abs(g.w - ref.w).max())} at the most"


def _check_graphs(e, pre, clean, wpre, wclean):
    gp, gc = e.graph("preclean"), e.graph("global")
    assert_graph_equal(gp, pre, WEIGHT_TOL)
    assert_graph_equal(gc, clean, WEIGHT_TOL)
    _same_as_witness(gp, wpre, "before cleanGraph")
    _same_as_witness(gc, wclean, "after cleanGraph")
    return gp, gc


def _check_counters(st, c):
    assert (st["trials"], st["samples"], st["created_nodes"], st["invalid_nodes"]) == \
        (c["trials"], c["samples"], c["created"], c["invalid_created"]), (st, c)


def _check(e, v):
    """The engine's build against the vetted case's oracle and witness.  -> the two graphs"""
    graphs = _check_graphs(e, v["pre"], v["clean"], v["wpre"], v["wclean"])
    _check_counters(e.stats(), v["counters"])
    return graphs


def _on_device(e, st, v=None):
    assert (st["used_device_bfs"], st["bfs_fallbacks"]) == (1, 0), (st, e.fallback_reason)
    if v is not None:
        # level k expands the valid nodes of depth k: the census's depths are the engine's levels + 1
        assert st["bfs_levels"] == v["census"]["max_valid_depth"] + 1, (st["bfs_levels"], v["census"])


def _declined(e, st, cause):
    assert (st["used_device_bfs"], st["bfs_fallbacks"]) == (0, 1), (st, e.fallback_reason)
    assert cause in e.fallback_reason, e.fallback_reason


def _bytes(graphs):
    return [a.tobytes() for g in graphs
            for a in (np.array([g.V, g.E]), g.xyz, g.state, g.cid, g.rowptr, g.col, g.w, g.dist)]


@pytest.fixture(scope="module")
def main(oa, synth):
    return s3.vetted(oa, synth, MAIN)


@pytest.fixture(scope="module")
def default_bytes(main):
    """Route 1's graphs on the main case, byte for byte: what every variant of the device build must reproduce."""
    e = _build_case(main)
    _on_device(e, e.stats(), main)
    ref = _bytes(_check(e, main))
    e.close()
    return ref


# ---- 1. the device build as it is -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [MAIN, "r160_s21", "r120_s21", s3.TRAP_CASE])
def test_device_build(oa, synth, name):
    """r160_s21 holds a chain (a node rescued by rescued nodes of its level only), the last case a trap (an Invalid
    node with a sound edge to an earlier candidate of its level that ended Invalid: no rescuer)."""
    v = s3.vetted(oa, synth, name)
    e = _build_case(v)
    st = _report(f"device {name}", e)
    _on_device(e, st, v)
    _check(e, v)
    e.close()


# ---- 2. the control: the host replay, whose !parent_ok branch asks the device about one node's neighbour edges ------
def test_host_replay(main):
    e = _build_case(main, replay="host")
    st = _report("replay=host", e)
    assert (st["used_device_bfs"], st["bfs_fallbacks"]) == (0, 0), (st, e.fallback_reason)
    _check(e, main)
    e.close()


# ---- 3. variants of the launches: the same bytes, on the device ------------------------------------------------------
@pytest.mark.parametrize("option,value", [("resolve_tickets", 1), ("debug_spec_bound", 3), ("defer_overlap", 0)])
def test_launch_variant_builds_the_same_bytes(main, default_bytes, option, value):
    """Start tickets for every resolve launch; an expansion bound of 3 nodes, so that the top-up launches run
    k_level_spec3 for nearly every candidate; the deferred calls all after the loop."""
    e = _build_case(main, **{option: value})
    st = _report(f"{option}={value}", e)
    _on_device(e, st, main)
    assert _bytes(_check(e, main)) == default_bytes
    e.close()


# ---- 4. a level with rescue records, left partially decided: undone and repeated with tickets ------------------------
@pytest.mark.parametrize("rerun_fails", [0, 1], ids=["ticketed-repeat", "repeat-fails"])
@pytest.mark.parametrize("hook", ["debug_stall_level", "debug_lookback_level"])
def test_level_with_rescues_is_undone_and_repeated(main, default_bytes, hook, rerun_fails):
    """The level is the first from 4 on in which a node is rescued by its own level only: its RescueRec must survive
    the undo.  The repeat with start tickets settles it on the device; if the repeat fails as well (debug_wait_rerun)
    the build declines -- a level of a step-3 build cannot be replayed on the host alone, a look-back that ran out
    twice sends any build there -- and the host replay builds the same graph."""
    level = s3.stall_level(main["census"])
    assert level + 1 in main["census"]["level_only_depths"] and level >= 4
    e = _build_case(main, **{hook: level, "debug_wait_rerun": rerun_fails})
    st = _report(f"{hook}={level} debug_wait_rerun={rerun_fails}", e)
    assert st["bfs_ticket_reruns"] == 1, st
    if rerun_fails:
        _declined(e, st, "needs the host replay" if hook == "debug_stall_level" else "look-back")
        _check(e, main)
    else:
        _on_device(e, st, main)
        assert _bytes(_check(e, main)) == default_bytes
    e.close()


# ---- 5. the declines of a step-3 build: counted, with the cause, and the host replay's graph is the oracle's ---------
@pytest.mark.parametrize("option,value,cause", [("debug_tie_every", 3, "distance tie"),
                                                ("debug_gate_margin", 0.15, "slope gate"),
                                                ("debug_fallback_level", 6, "declined on request")])
def test_decline(main, option, value, cause):
    e = _build_case(main, **{option: value})
    st = _report(f"{option}={value}", e)
    _declined(e, st, cause)
    if option == "debug_gate_margin":
        assert st["gate_uncertain"] > 20, st["gate_uncertain"]
    _check(e, main)
    e.close()


def test_decline_by_a_natural_tie(oa, synth):
    """16 sampling directions on nearly level ground: samples at exactly the same fp32 distance from two nodes.  The
    tie repairs know nothing of step 3, the build goes to the host replay."""
    t = s3.TIES
    prm = dict(oa.INDOOR, **t["overrides"])
    cloud = s3.ties_cloud(synth)
    e = _build(prm, cloud, t["start"], t["seed"], t["table_bits"])
    st = _report("natural ties", e)
    _declined(e, st, "distance tie")
    assert st["nn_ties"] > 0, st
    o = s3.build_oracle(oa, prm, cloud, t["start"], t["seed"], table_bits=t["table_bits"])
    w = s3.build_oracle(oa, prm, cloud, t["start"], t["seed"], f64=True, table_bits=t["table_bits"])
    _check_graphs(e, o.graph(1), o.graph(0), w.graph(1), w.graph(0))
    _check_counters(st, o.counters())
    e.close()


# ---- 6. sample_num 64: dozens of same-level candidates within expand_dist of one another ----------------------------
def test_sample_num_64(oa, synth):
    """S3_LIST (48 neighbours looked at) or RESC_MAX (14 rescuers kept) may overflow, and rescuers join pass 0 of a
    row that takes its blockers in several passes: either the device builds the oracle's graph or it declines with
    step 3 as the cause and the host replay does."""
    v = s3.vetted(oa, synth, "r160_S64_s7")
    e = _build_case(v)
    st = _report("sample_num=64", e)
    print(f"[step3] sample_num=64: {'stayed on the device' if st['bfs_fallbacks'] == 0 else 'declined'}, "
          f"bfs_multipass_rows={st['bfs_multipass_rows']}")
    if st["bfs_fallbacks"] == 0:
        _on_device(e, st, v)
    else:
        _declined(e, st, "step 3")
    _check(e, v)
    e.close()


# ---- 7. one engine, three builds: resc, s3_scratch and the level hash's tags are reused ------------------------------
def test_three_builds_on_one_engine(oa, synth, main):
    import trg_planner
    other = s3.vetted(oa, synth, "r160_s7_start_b")
    prm, cloud, seed = main["prm"], main["cloud"], main["case"].seed
    assert (other["prm"], other["case"].seed, other["case"].cloud) == (prm, seed, main["case"].cloud)
    e = trg_planner.Engine(**prm)
    e.set_sampler(seed, s3.TABLE_BITS)
    e.set_option("keep_preclean", 1)
    o, w = oa.Oracle(**prm), oa.Oracle(**prm)
    for x in (o, w):
        x.set_sampler(seed, 0, s3.TABLE_BITS)
    w.set_cov_f64(True)
    for who in (e, o, w):
        who.set_global_map(cloud)
    for k, v in enumerate((main, other, main)):
        o.reset_counters()
        e.init_graph(v["case"].start)
        assert o.init_graph(v["case"].start) and w.init_graph(v["case"].start)
        st = _report(f"one engine, build {k}", e)
        _on_device(e, st, v)
        # (cleanGraph's numbering follows the node container's history: the oracle that went through the same calls)
        _check_graphs(e, o.graph(1), o.graph(0), w.graph(1), w.graph(0))
        _check_counters(st, o.counters())
        # ... and before cleanGraph the build is that of a fresh engine
        assert_graph_equal(e.graph("preclean"), v["pre"], WEIGHT_TOL)
    e.close()


# ---- 8. determinism --------------------------------------------------------------------------------------------------
def test_five_builds_are_byte_equal(main, default_bytes):
    """k_level_resolve lets the lanes of a level decide concurrently, the waits for rescuers included: nothing may
    depend on timing."""
    for k in range(5):
        e = _build_case(main)
        _on_device(e, e.stats(), main)
        assert _bytes((e.graph("preclean"), e.graph("global"))) == default_bytes, k
        e.close()
