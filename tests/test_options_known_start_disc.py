"""CPU: the option known_start_disc through the C ABI -- its default, the values it accepts, the values it
rejects and the text trg_engine_last_error then holds (set_option needs no device; tests/test_options.py pins
the other keys the same way), and the statistic that goes with it."""
import ctypes as C

import pytest

OK, INVALID_ARG, ERR_DEVICE = 0, 1, 4
TEXT = b"known_start_disc must be 0 or 1"


@pytest.fixture()
def handle():
    import trg_planner
    from trg_planner._engine import TrgParams
    trg_planner.build_library()
    L = trg_planner.load_library()
    prm = TrgParams(0, 0.6, 0.3, 8, 0.3, 0.2, 0.5, 1.0, 0.5)
    h = C.c_void_p()
    st = L.trg_engine_create(C.byref(prm), 0, C.byref(h))
    assert h.value and st in (OK, ERR_DEVICE), (st, L.trg_engine_last_error(h))
    yield L, h
    L.trg_engine_destroy(h)


def test_known_start_disc_accepts_0_and_1(handle):
    L, h = handle
    before = L.trg_engine_last_error(h)
    for v in (b"0", b"1", b"0", b"1"):
        assert L.trg_engine_set_option(h, b"known_start_disc", v) == OK, v
    assert L.trg_engine_last_error(h) == before  # (an accepted option leaves the last error alone)


@pytest.mark.parametrize("value", [b"2", b"", b"true", b"-1", b"01", b"1 ", b"on"])
def test_known_start_disc_rejects_everything_else(handle, value):
    L, h = handle
    assert L.trg_engine_set_option(h, b"known_start_disc", value) == INVALID_ARG, value
    assert L.trg_engine_last_error(h) == TEXT, value
    # ... and goes on accepting a valid value afterwards; the text stays
    assert L.trg_engine_set_option(h, b"known_start_disc", b"1") == OK
    assert L.trg_engine_last_error(h) == TEXT


def test_the_key_is_spelled_exactly(handle):
    L, h = handle
    assert L.trg_engine_set_option(h, b"Known_start_disc", b"1") == INVALID_ARG
    assert L.trg_engine_last_error(h) == b"unknown option Known_start_disc"


def test_the_statistic_is_appended_and_starts_at_zero(handle):
    """start_discs_known follows stitch_regrows in TrgStats (the struct only grows at its end) and is 0 before a
    build."""
    from trg_planner._engine import TrgStats
    L, h = handle
    names = [f[0] for f in TrgStats._fields_]
    assert names.index("start_discs_known") == names.index("stitch_regrows") + 1
    st = TrgStats()
    assert L.trg_engine_get_stats(h, C.byref(st)) == OK
    assert st.start_discs_known == 0
