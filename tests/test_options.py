"""CPU: trg_engine_set_option through the C ABI -- every key the engine accepts, the values it rejects and the
text trg_engine_last_error then holds.  trg_engine_create hands out a handle even when it fails for lack of a
device and set_option needs no device, so this also runs create-fails -> destroy on a machine without a GPU.
There is no getter for options: status and error text are what is pinned here, what the options do is pinned
by the GPU suite."""
import ctypes as C

import pytest

OK, INVALID_ARG, ERR_DEVICE = 0, 1, 4

# key -> values that are accepted (text that is not a number goes through atoi / atof / `!= "0"` as it is)
ACCEPTED = {
    "replay": ["host", "device"],
    "debug_gate_margin": ["0.15", "1e-4", "abc", ""],
    "debug_tie_every": ["3", "0", "-1", "abc", ""],
    "debug_spec_bound": ["3", "0", "7x"],
    "defer_overlap": ["0", "1"],
    "debug_stall_level": ["9", "-1", "abc"],
    "debug_lookback_level": ["7", "-1", ""],
    "debug_call_stride": ["1", "0", "yes", ""],
    "debug_wait_rerun": ["1", "0", "no"],
    "resolve_tickets": ["1", "0", "abc"],
    "tie_inplace": ["0", "1", "True"],
    "debug_fallback_level": ["6", "-1", "abc"],
    "keep_preclean": ["1", "0", "2"],
    "field_delta_scale": ["4", "0.5", "inf", "1e3", "2x"],
    "debug_stitch_cap": ["4", "0", "-1", "abc"],
    "comm_wait_seconds": ["20", "0.5", "1e3"],
}

# (key, value, the error text)
REJECTED = [
    ("replay", "x", "replay must be host or device"),
    ("replay", "", "replay must be host or device"),
    ("replay", "Host", "replay must be host or device"),
    ("defer_overlap", "2", "defer_overlap must be 0 or 1"),
    ("defer_overlap", "", "defer_overlap must be 0 or 1"),
    ("defer_overlap", "true", "defer_overlap must be 0 or 1"),
    ("field_delta_scale", "0", "field_delta_scale must be > 0"),
    ("field_delta_scale", "-1", "field_delta_scale must be > 0"),
    ("field_delta_scale", "abc", "field_delta_scale must be > 0"),
    ("field_delta_scale", "nan", "field_delta_scale must be > 0"),
    ("field_delta_scale", "", "field_delta_scale must be > 0"),
    ("comm_wait_seconds", "0", "comm_wait_seconds must be > 0"),
    ("comm_wait_seconds", "-2", "comm_wait_seconds must be > 0"),
    ("no_such_option", "1", "unknown option no_such_option"),
    ("", "1", "unknown option "),
    ("Replay", "host", "unknown option Replay"),
    ("replay ", "host", "unknown option replay "),
]


def _params():
    from trg_planner._engine import TrgParams
    return TrgParams(0, 0.6, 0.3, 8, 0.3, 0.2, 0.5, 1.0, 0.5)


def _library():
    import trg_planner
    trg_planner.build_library()
    return trg_planner.load_library()


@pytest.fixture()
def handle():
    L = _library()
    prm = _params()
    h = C.c_void_p()
    st = L.trg_engine_create(C.byref(prm), 0, C.byref(h))
    assert h.value, "create hands a handle out even when it fails"
    assert st in (OK, ERR_DEVICE), (st, L.trg_engine_last_error(h))
    if st == ERR_DEVICE:
        assert L.trg_engine_last_error(h), "a failed create leaves its reason"
    yield L, h
    L.trg_engine_destroy(h)


def test_every_key_accepts_its_values(handle):
    L, h = handle
    before = L.trg_engine_last_error(h)
    for key, values in ACCEPTED.items():
        for v in values:
            assert L.trg_engine_set_option(h, key.encode(), v.encode()) == OK, (key, v)
    # an accepted option leaves the last error alone
    assert L.trg_engine_last_error(h) == before


def test_rejected_values_and_their_text(handle):
    L, h = handle
    for key, v, text in REJECTED:
        assert L.trg_engine_set_option(h, key.encode(), v.encode()) == INVALID_ARG, (key, v)
        assert L.trg_engine_last_error(h) == text.encode(), (key, v)
        # ... and the key goes on accepting a valid value afterwards; the text stays
        if key in ACCEPTED:
            assert L.trg_engine_set_option(h, key.encode(), ACCEPTED[key][0].encode()) == OK, key
            assert L.trg_engine_last_error(h) == text.encode(), key


def test_null_arguments(handle):
    L, h = handle
    before = L.trg_engine_last_error(h)
    assert L.trg_engine_set_option(h, None, b"1") == INVALID_ARG
    assert L.trg_engine_set_option(h, b"replay", None) == INVALID_ARG
    assert L.trg_engine_set_option(h, None, None) == INVALID_ARG
    assert L.trg_engine_set_option(None, b"replay", b"host") == INVALID_ARG
    assert L.trg_engine_last_error(h) == before  # (nothing was parsed: the text is untouched)
    assert L.trg_engine_last_error(None) == b"null engine"


def test_destroy_after_failed_create_and_of_null():
    """create -> destroy several times in one process (without a device create fails, and destroy has to release
    whatever create made before it failed without needing a device); destroy(NULL) does nothing."""
    L = _library()
    L.trg_engine_destroy(None)
    prm = _params()
    for device in (0, 0, 10 ** 6, -1):
        h = C.c_void_p()
        st = L.trg_engine_create(C.byref(prm), device, C.byref(h))
        assert h.value
        if device != 0:
            assert st in (INVALID_ARG, ERR_DEVICE)
            assert L.trg_engine_last_error(h) in (
                b"bad device ordinal", b"no HIP device visible: the TRG engine has no CPU fallback")
        assert L.trg_engine_set_option(h, b"replay", b"host") == OK
        L.trg_engine_destroy(h)
