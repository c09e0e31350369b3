"""csrc/hip/scene_refit.h, the per-node arithmetic of spt_scene_deform's refit kernels: `make scene-deform-refit-check` builds
tests/scene_deform_refit_check.cpp, a stand-alone program, together with the scene builder under AddressSanitizer + UBSan.  Over 200
random meshes of 1 to 3000 triangles it builds the compressed 4-wide BLAS, deforms the mesh (smoothly, wildly, scaled by 100 far
off the origin, flattened to a plane, collapsed to a point, not at all) and runs the kernels' level schedule on the CPU with the
kernels' own code; it must exit 0 without a report.  Host code only; nothing of it is loaded into this process, and no device is
needed."""
import os
import subprocess

import _util


def test_refit_keeps_the_topology_and_stays_conservative():
    res = subprocess.run(["make", "-s", "-C", _util.ROOT, "scene-deform-refit-check"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    res = subprocess.run([os.path.join(_util.ROOT, "build", "selftest", "scene_deform_refit_check"), "200"], capture_output=True, text=True, timeout=120)
    report = res.stdout + res.stderr
    assert res.returncode == 0, report
    assert "scene_deform_refit_check ok: 200 meshes" in res.stdout, report
    for word in ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer", "CHECK failed"):
        assert word not in report, report
