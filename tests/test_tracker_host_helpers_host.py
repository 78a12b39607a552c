"""csrc/gmr_tracker_host.h, what the entry points of the motion tracker share on the host, checked on the CPU:
tests/cpp/tracker_host_check.cpp is plain C++ (g++) with its own main and a gmr_fail that records the message.  It pins
noise_spec over a table of specs (the struct the kernels read, and for every refusal the whole message under the caller's name)
and subset_check for every phrase an entry point passes."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "tracker_host_check.cpp")


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr[-2000:])
    return out


def test_noise_specs_and_environment_lists_as_the_entry_points_check_them(tmp_path):
    exe = str(tmp_path / "tracker_host_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, SRC])
    _run(exe)


def test_the_host_helpers_are_clean_under_sanitizers(tmp_path):
    """The same stand-alone program under AddressSanitizer + UBSan: the float32 conversions of a spec's bounds and the grid sizes
    are host arithmetic at the edge of their types."""
    exe = str(tmp_path / "tracker_host_check_asan")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC],
                        capture_output=True, text=True)
    if cc.returncode != 0:
        pytest.skip("sanitizer runtime not available: " + cc.stderr[-200:])
    out = _run(exe)
    assert "runtime error" not in out.stderr and "ERROR" not in out.stderr, out.stderr[-2000:]
