"""include/spt_mesh_assemble.h, the arithmetic of spt_scene_deform_vertices' kernels (vertex tangent frames, triangle records):
`make mesh-assemble-check` builds tests/mesh_assemble_check.cpp, a stand-alone program, under AddressSanitizer + UBSan against the
host loader.  Over 200 random meshes of 1 to 3000 triangles (faces with a zero uv determinant, collapsed faces with NaN frames,
faces naming a vertex twice, vertices no face names), a 300-triangle fan and a one-triangle mesh it runs the header by the kernels'
schedule - per vertex over the vertex -> corner table, then per triangle through a random face_of_tri - and requires the loader's
calc_tangents / face_records words; it must exit 0 without a report.  Host code only; nothing of it is loaded into this process,
and no device is needed."""
import os
import subprocess

import _util


def test_the_header_computes_the_loaders_tangents_and_records():
    res = subprocess.run(["make", "-s", "-C", _util.ROOT, "mesh-assemble-check"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    res = subprocess.run([os.path.join(_util.ROOT, "build", "selftest", "mesh_assemble_check"), "200"], capture_output=True, text=True, timeout=120)
    report = res.stdout + res.stderr
    assert res.returncode == 0, report
    assert "mesh_assemble_check ok: 200 random meshes" in res.stdout, report
    for word in ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer", "CHECK failed"):
        assert word not in report, report
