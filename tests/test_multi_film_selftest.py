"""The film fan-out of csrc/host/multi.cpp under ThreadSanitizer and under AddressSanitizer + UBSan: `make selftest` builds
csrc/host/multi_film_selftest.cpp (a stand-alone program with stand-in devices, 1 - 5 workers) twice, together with multi.cpp, and both
programs must exit 0 without a sanitizer report.  Host code only; nothing of it is loaded into this process."""
import os
import subprocess

import pytest

import _util

BIN = os.path.join(_util.ROOT, "build", "selftest")


@pytest.fixture(scope="module")
def built():
    res = subprocess.run(["make", "-s", "-j2", "-C", _util.ROOT, "selftest"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr


@pytest.mark.parametrize("flavour", ["tsan", "asan"])
def test_fan_out_selftest_is_clean(built, flavour):
    res = subprocess.run([os.path.join(BIN, "multi_film_selftest_" + flavour)], capture_output=True, text=True, timeout=300)
    report = res.stdout + res.stderr
    assert res.returncode == 0, report
    assert "multi_film_selftest ok" in res.stdout
    for word in ("WARNING: ThreadSanitizer", "ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer", "CHECK failed"):
        assert word not in report, report
