"""CPU: the C boundary's frame.  tests/cpp/abi_frame_check.cpp checks csrc/abi_frame.h on its own (plain and under
the sanitizers); the structural tests read the engine's sources and hold every exported symbol to the one shape:
argument checks, then entry() or abi_guard() around a named function."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trg-planner_amd", "csrc")
CHECK = os.path.join(ROOT, "tests", "cpp", "abi_frame_check.cpp")

# the entries that stay bare: destroy allocates nothing and destructors do not throw; the getters return a pointer
# into the engine and touch no allocation
BARE = {"trg_engine_destroy", "trg_engine_last_error", "trg_engine_device_arch", "trg_engine_fallback_reason"}


@pytest.mark.parametrize("flags", [
    ["-O2"],
    ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"],
    ["-O1", "-g", "-fsanitize=thread"],
], ids=["plain", "asan_ubsan", "tsan"])
def test_abi_frame_header_stands_alone(tmp_path, flags):
    exe = tmp_path / "abi_frame_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread"] + flags +
                          [CHECK, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


def _sources():
    """path -> text without // comments, for every source under csrc but the pybind module"""
    out = {}
    for name in sorted(os.listdir(CSRC)):
        if name == "trg_pybind.cpp" or not name.endswith((".cpp", ".ipp", ".inc", ".h", ".hip")):
            continue
        with open(os.path.join(CSRC, name)) as f:
            out[name] = re.sub(r"//[^\n]*", "", f.read())
    return out


def _definitions(text):
    """(name, body) of every function defined at the left margin whose name starts with trg_engine_"""
    for m in re.finditer(r"^[A-Za-z_][\w \*]*?\b(trg_engine_[a-z_0-9]+)\(", text, re.M):
        brace = text.index("{", m.end())
        assert ";" not in text[m.end():brace], m.group(1)  # (a definition, not a declaration)
        depth, end = 0, brace
        while True:  # (no brace of these bodies stands in a string)
            depth += {"{": 1, "}": -1}.get(text[end], 0)
            end += 1
            if depth == 0:
                break
        yield m.group(1), text[brace:end], (m.start(), end)


def test_every_export_goes_through_the_frame():
    from trg_planner._engine import EXPORTS
    defs = {}
    for name, text in _sources().items():
        for sym, body, _ in _definitions(text):
            defs.setdefault(sym, []).append((name, body))
    assert sorted(defs) == sorted(EXPORTS)
    assert BARE <= set(EXPORTS)
    for sym, found in defs.items():
        assert len(found) == 1, (sym, [f for f, _ in found])
        body = found[0][1]
        assert ("entry(" in body or "abi_guard(" in body) == (sym not in BARE), sym
    # (the field entries' field_entry is itself entry() and nothing beside it)
    frame = re.search(r"TrgStatus field_entry\(.*?\n}\n", _sources()["trg_engine_field.ipp"], re.S).group(0)
    assert "return entry(e, call, DEVICE," in frame and "catch" not in frame


def test_no_code_calls_the_abi():
    """Outside the entries' own definitions nothing under csrc names an exported symbol with an argument list."""
    for name, text in _sources().items():
        spans = [span for _, _, span in _definitions(text)]
        for m in re.finditer(r"trg_engine_[a-z_]+\(", text):
            inside = [s for s in spans if s[0] <= m.start() < s[1]]
            assert inside, (name, m.group(0))
            # within a definition: only the definition's own name, at its head
            sym = re.search(r"trg_engine_[a-z_0-9]+", text[inside[0][0]:inside[0][1]]).group(0)
            assert m.group(0) == sym + "(" and text.index(m.group(0), inside[0][0]) == m.start(), (name, m.group(0))


def test_one_frame_one_fork_join():
    texts = _sources()
    with_comments = {}
    for name in texts:
        with open(os.path.join(CSRC, name)) as f:
            with_comments[name] = f.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        with_comments["INTEGRATION.md"] = f.read()
    assert not [n for n, t in with_comments.items() if "REQUIRE_DEVICE" in t]
    # a thread is made in abi_frame.h (std::vector<Thread>, Thread = std::thread) and by start_map_top, nowhere else:
    # whatever else names std::thread asks for the hardware's thread count or declares the member start_map_top fills
    made = {}
    for name, text in texts.items():
        for m in re.finditer(r"std::thread\b(?!::hardware_concurrency)[^\n]*", text):
            made.setdefault(name, []).append(m.group(0).strip())
    assert sorted(made) == ["abi_frame.h", "trg_engine.cpp", "trg_engine_probe.ipp"], made
    assert made["abi_frame.h"] == ["std::thread, typename F>"]
    assert made["trg_engine.cpp"] == ["std::thread top_thread;"]
    assert len(made["trg_engine_probe.ipp"]) == 1 and made["trg_engine_probe.ipp"][0].startswith("std::thread([")
    probe = texts["trg_engine_probe.ipp"]
    heads = [m for m in re.finditer(r"^[A-Za-z_][\w \*&:<>]*?\b(\w+)\([^;{]*\) \{$", probe, re.M)
             if m.start() < probe.index("std::thread([")]
    assert heads[-1].group(1) == "start_map_top", heads[-1].group(0)
    assert not [n for n, t in texts.items() if "emplace_back(work" in t or "std::vector<std::thread>" in t]
