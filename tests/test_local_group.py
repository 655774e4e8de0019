"""CPU: csrc/local_group.h, the host side of the stitch exchange's in-process transport (barriers in a condition
variable, the table of named groups), on its own: tests/cpp/local_group_check.cpp plain and under the thread sanitizer.
What the transport moves on the device is tests/test_gpu_exchange_ranks.py's."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "cpp", "local_group_check.cpp")


@pytest.mark.parametrize("flags", [
    ["-O2"],
    ["-O1", "-g", "-fsanitize=thread"],
    ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"],
], ids=["plain", "tsan", "asan_ubsan"])
def test_local_group_header_stands_alone(tmp_path, flags):
    exe = tmp_path / "local_group_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread"] + flags +
                          [CHECK, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
