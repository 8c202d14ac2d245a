"""The per-device once-table behind allow_lds / launch_lds (csrc/per_device.hpp), exercised without a GPU: tests/per_device_once.cpp
is compiled as plain C++ (the header has no HIP in it) with the host compiler build.py locates, run once, and its figures asserted here.
Counting stubs stand in for hipFuncSetAttribute."""
import os
import subprocess

import pytest

from realcamnet_amd import build as rc_build

HERE = os.path.dirname(os.path.abspath(__file__))
KB = 1024


@pytest.fixture(scope="module")
def figures(tmp_path_factory):
    exe = tmp_path_factory.mktemp("per_device_once") / "per_device_once"
    cmd = [rc_build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-Wall", "-pthread", os.path.join(HERE, "per_device_once.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return dict(line.split("=", 1) for line in r.stdout.split())


def test_header_is_plain_cxx():
    text = open(os.path.join(HERE, "..", "realcamnet_amd", "csrc", "per_device.hpp")).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert includes == ["<atomic>"]


def test_threads_racing_on_fresh_slots(figures):
    """(a) 8 threads x 100 KB x all 64 devices: every request succeeds, every slot ends granted, `set` ran at least once per slot (racing threads may
    both run it, never more often than there are threads), and a second pass of requests <= 100 KB runs it not at all."""
    assert figures["slots"] == "64"
    assert figures["a_failed"] == "0"
    assert figures["a_granted"] == "64"
    assert 1 <= int(figures["a_min_calls"]) <= int(figures["a_max_calls"]) <= 8
    assert figures["a_second_calls"] == "0"
    assert figures["a_second_ok"] == "128"


def test_failure_is_never_recorded(figures):
    """(b) a failing `set` returns failure and leaves the slot unmarked, twice over; the next request runs `set` again, and its success is recorded."""
    assert figures["b_results"] == "0011"
    assert figures["b_limit_after_fail"] == "0"
    assert figures["b_calls"] == "3"
    assert figures["b_limit"] == str(100 * KB)


def test_larger_request_raises_the_limit_once(figures):
    """(c) 100 KB, then 160 KB (one more `set`, asked for 160 KB), then 120 KB (none)."""
    assert figures["c_calls"] == "1,2,2"
    assert figures["c_asked"] == str(160 * KB)
    assert figures["c_limit"] == str(160 * KB)


def test_slots_do_not_alias_and_the_last_one_works(figures):
    """(d) granting slot 0 leaves slot 1 (and every other) ungranted; index 63 is granted by one `set`."""
    assert figures["d_limit0"] == str(100 * KB)
    assert figures["d_limit1"] == "0"
    assert figures["d_limit_last"] == str(100 * KB)
    assert figures["d_calls"] == "2"
    assert figures["d_others"] == "0"
