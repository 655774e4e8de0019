"""The step-3 cases of step3_cases.py on the two oracles alone (fp32 covariance and the fp64 witness): every case a
GPU test rests on still shows what it was chosen for -- failed parent edges, nodes rescued by a pre-level node and by
their own level only, non-zero weights on the rescued nodes' rows, nodes that stay Invalid, no slope gate inside the
engine's gate_margin -- so that a later edit to a cloud or a seed cannot quietly turn one into a flat floor.  No GPU."""
import pytest

import step3_cases as s3
from conftest import assert_graph_equal

WEIGHT_TOL = 1e-5


@pytest.mark.parametrize("name", [c.name for c in s3.CASES])
def test_case_on_the_oracles(oa, synth, name):
    v = s3.vetted(oa, synth, name)
    c = v["census"]
    print(name, "V", v["clean"].V, "E", v["clean"].E, "non-zero w", int((v["clean"].w != 0).sum()), c)
    s3.check_preconditions(c, v["clean"])
    # the census and the oracle's own counters tell the same story
    assert c["Vpre"] == v["pre"].V == v["counters"]["created"]
    assert c["invalid"] == v["counters"]["invalid_created"]
    assert c["failed"] == c["rescued"] + c["invalid"]  # (with step 3 a node is Invalid only if every call failed)
    assert c["by_pre"] + c["by_level"] == c["rescued"]
    assert c["max_valid_depth"] >= 10
    # the stall hooks need a level >= 4 in which a node waits for a rescuer of its own level
    assert 4 <= s3.stall_level(c) <= c["max_valid_depth"] - 1
    # the literal fp32 oracle and the fp64-covariance witness: same structure, no clamp flip
    assert_graph_equal(v["wpre"], v["pre"], WEIGHT_TOL)
    assert_graph_equal(v["wclean"], v["clean"], WEIGHT_TOL)


def test_the_suite_holds_a_chain_and_a_trap(oa, synth):
    """A node rescued only by nodes of its level that were rescued themselves; an Invalid node next to an Invalid
    earlier candidate of its level that it has a sound edge to."""
    chains = {name: s3.vetted(oa, synth, name)["census"]["chains"] for name in s3.CHAIN_CASES}
    assert chains["r160_s21"] >= 1, chains
    assert s3.vetted(oa, synth, s3.TRAP_CASE)["census"]["invalid_rescuer_traps"] >= 1


def test_the_flat_indoor_fixture_has_no_failed_parent_edge(oa, indoor_small):
    """Why the fixture of test_gpu_node_cov.test_step3_build_structure_and_states, test_init_graph_parity[indoor_S15],
    test_gpu_deferred_select[indoor_step3] and indoor_step3_updates is not enough: step 3 is on, and decides
    nothing."""
    prm = dict(oa.INDOOR)
    assert s3.step3_is_on(prm)
    o = s3.build_oracle(oa, prm, indoor_small, [1.5, 1.5, 0.0], 7, trace=True)
    c = s3.rescue_census(o, o.graph(1), prm)
    assert c["Vpre"] > 200
    assert (c["failed"], c["rescued"], c["invalid"], c["nonzero_pre"]) == (0, 0, 0, 0), c


def test_the_natural_tie_case_on_the_oracles(oa, synth):
    """The decline by a natural nearest-node tie runs on nearly level ground (16 sampling directions); the oracles
    must agree on it, and step 3 must be on."""
    t = s3.TIES
    prm = dict(oa.INDOOR, **t["overrides"])
    assert s3.step3_is_on(prm)
    cloud = s3.ties_cloud(synth)
    o = s3.build_oracle(oa, prm, cloud, t["start"], t["seed"], table_bits=t["table_bits"])
    w = s3.build_oracle(oa, prm, cloud, t["start"], t["seed"], f64=True, table_bits=t["table_bits"])
    assert o.graph(0).V > 1000
    assert_graph_equal(w.graph(1), o.graph(1), WEIGHT_TOL)
    assert_graph_equal(w.graph(0), o.graph(0), WEIGHT_TOL)
