"""CPU: the node container's iteration order as a list of runs, and its expansion on the device's terms.

A plain device build no longer writes cleanGraph's renumbering order (V ids) on the host: MapOrderSim hands out
its runs, and a kernel expands them with map_order_at (map_order_runs.h).  tests/cpp/map_order_runs_check.cpp
compares that function, compiled for the host, with MapOrderSim::iteration_order and with a real
std::unordered_map<int, int>: sizes 0, 1, 2, at and one past every rehash up to a million keys, 642 000 (the
benchmark's node count), after clear() + refill with fewer and more keys, after assign_from, and checks that
four million nodes stay under the cap of 64 runs."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "map_order_runs_check.cpp")


def _run(exe):
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr
    print(out.stdout.strip())


def test_runs_expand_to_the_container_order(tmp_path):
    exe = tmp_path / "map_order_runs_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", str(exe)])
    _run(exe)


def test_runs_check_under_sanitizers(tmp_path):
    exe = tmp_path / "map_order_runs_check.asan"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", SRC, "-o", str(exe)])
    _run(exe)
