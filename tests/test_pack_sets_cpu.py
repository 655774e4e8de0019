"""CPU: _engine.pack_sets, the one place where source sets (and their start costs) become the arrays the set entries
take -- shapes, dtypes and contiguity for no set, a set of one and sets of different length, with and without start
costs, and the refusal of start costs of another shape under the name of the call that answers for them.  (The other
refusal, of more than 2^31 - 1 entries, would need 8 GiB of them.)  No engine handle, no GPU."""
import numpy as np
import pytest

from trg_planner._engine import pack_sets


def _check(sets, ptr, ids, want_sets):
    assert len(sets) == len(want_sets)
    for s, w in zip(sets, want_sets):
        assert s.dtype == np.int32 and s.ndim == 1 and s.tolist() == list(w)
    assert ptr.dtype == np.int32 and ptr.tolist() == np.cumsum([0] + [len(w) for w in want_sets]).tolist()
    assert ids.dtype == np.int32 and ids.ndim == 1 and ids.flags.c_contiguous
    assert ids.tolist() == [v for w in want_sets for v in w]


def test_pack_sets():
    # no set at all: ptr is the one zero, nothing is concatenated
    sets, ptr, ids, starts, c0 = pack_sets("who", [])
    _check(sets, ptr, ids, [])
    assert starts is None and c0 is None
    sets, ptr, ids, starts, c0 = pack_sets("who", [], [])
    _check(sets, ptr, ids, [])
    assert starts == [] and c0.dtype == np.float32 and c0.shape == (0,) and c0.flags.c_contiguous
    # a set of one
    sets, ptr, ids, starts, c0 = pack_sets("who", [[7]])
    _check(sets, ptr, ids, [[7]])
    assert starts is None and c0 is None
    # three sets of different length: an int64 array, a Python list, a strided view; with and without start costs
    given = [np.array([5, 5, 2], np.int64), [9], np.arange(10, dtype=np.int32)[::3]]
    want = [[5, 5, 2], [9], [0, 3, 6, 9]]
    sets, ptr, ids, starts, c0 = pack_sets("who", given)
    _check(sets, ptr, ids, want)
    assert starts is None and c0 is None
    costs = [[0.5, 0.0, 2.0], np.array([1.0], np.float64), (0.25, 0.25, 3.0, 4.0)]
    sets, ptr, ids, starts, c0 = pack_sets("who", given, costs)
    _check(sets, ptr, ids, want)
    assert [c.dtype for c in starts] == [np.float32] * 3 and [c.tolist() for c in starts] == [list(c) for c in costs]
    assert c0.dtype == np.float32 and c0.flags.c_contiguous and c0.tolist() == [v for c in costs for v in c]
    # start costs of another shape -- too few arrays, too many, one too long, one too short -- under the caller's name
    for who, who_starts, named in (("tiled_cost_fields_from", None, "tiled_cost_fields_from"),
                                   ("cost_fields_from", "cost_fields_seeded", "cost_fields_seeded")):
        for bad in ([[0.0, 0.0]], [[0.0, 0.0], [0.0], [0.0]], [[0.0, 0.0], [0.0, 1.0]], [[0.0], [0.0]]):
            with pytest.raises(ValueError) as err:
                pack_sets(who, [[1, 2], [3]], bad, who_starts=who_starts)
            assert str(err.value) == f"{named}: start_costs and sets differ in shape"
