"""csrc/hip/out_layout.h, the arithmetic the finish kernel that stores into the caller's buffer (k_finish_host) shares with the host:
`make out-layout-check` builds tests/out_layout_check.cpp, a stand-alone program, with AddressSanitizer + UBSan; it walks the kernel's
windows for packed, ragged, misaligned and strided shapes against a plain loop over rows and must exit 0 without a report.  Host
code only; nothing of it is loaded into this process."""
import os
import subprocess

import _util


def test_out_layout_matches_the_plain_loop():
    res = subprocess.run(["make", "-s", "-C", _util.ROOT, "out-layout-check"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    res = subprocess.run([os.path.join(_util.ROOT, "build", "selftest", "out_layout_check")], capture_output=True, text=True, timeout=120)
    report = res.stdout + res.stderr
    assert res.returncode == 0, report
    assert "out_layout_check ok" in res.stdout
    for word in ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer", "CHECK failed"):
        assert word not in report, report
