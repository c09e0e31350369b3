"""csrc/hip/scene_build.h, the host-only scene builder behind spt_scene_create and spt_scene_update: `make scene-build-check` builds
tests/scene_build_check.cpp, a stand-alone program, together with the builder under AddressSanitizer + UBSan.  Over the scene files
written here it checks the blob's layout, that every reference of the trees stays inside its section, that an update writes what a
creation would have written, determinism and the refusals, each under the default options, the large-scene form, the caller's trees
and with the streaming walker off; it must exit 0 without a report.  Host code only; nothing of it is loaded into this process, and
no device is needed."""
import json
import math
import os
import shutil
import subprocess

import _scene_update_scenes as S
import _util

REFERENCE_SCENES = os.path.join(_util.ROOT, "tests", "golden", "reference_scenes")


def _bumpy_sphere_obj(n_lat, n_lon):
    """A closed mesh of 2 * n_lon * (n_lat - 1) triangles (an odd number of leaf remainders, trees several levels deep)."""
    v, f = ["v 0 1 0", "v 0 -1 0"], []
    for i in range(1, n_lat):
        th = math.pi * i / n_lat
        for j in range(n_lon):
            ph = 2.0 * math.pi * j / n_lon
            r = 1.0 + 0.15 * math.sin(3.0 * ph) * math.sin(2.0 * th)
            v.append("v %.6f %.6f %.6f" % (r * math.sin(th) * math.cos(ph), r * math.cos(th), r * math.sin(th) * math.sin(ph)))
    ring = lambda i, j: 3 + (i - 1) * n_lon + j % n_lon       # 1-based index of ring i (1 .. n_lat - 1), column j
    for j in range(n_lon):
        f.append((1, ring(1, j + 1), ring(1, j)))
        f.append((2, ring(n_lat - 1, j), ring(n_lat - 1, j + 1)))
        for i in range(1, n_lat - 1):
            f.append((ring(i, j), ring(i, j + 1), ring(i + 1, j + 1)))
            f.append((ring(i, j), ring(i + 1, j + 1), ring(i + 1, j)))
    return "\n".join(v + ["vn 0 1 0", "vt 0 0"] + ["f %d/1/1 %d/1/1 %d/1/1" % t for t in f]) + "\n"


def _many_instances(transforms_shift, model="bumpy"):
    """Three dozen instances of the bumpy sphere, the cube and the unit sphere on a jittered grid: multi-node TLASes of both widths,
    BLAS several levels deep; with the larger sphere a blob beyond LDS, with the smaller one a blob that fits."""
    d = S.scene_dict(S.TRANSFORMS_A)
    d["primitives"].append({"type": "trimesh", "name": "bumpy", "obj_file": "models/%s.obj" % model})
    d["light_sampler"] = "uniform"
    prims, mats = ("bumpy", "cube", "unit_sphere"), ("m_white", "m_red", "m_blue")
    for k in range(37):
        x, z = (k % 7) - 3.0, (k // 7) - 3.0
        s = 0.25 + 0.02 * (k % 5)
        d["instances"].append({"name": "g%02d" % k, "primitive": prims[k % 3], "material": mats[k % 3], "scale": [s, s * 1.1, s],
                               "rotate": [7.0 * k, 13.0 * k + transforms_shift, 0.0], "translate": [1.3 * x + 0.1 * transforms_shift, 0.4 * (k % 4), 1.3 * z]})
    return d


def _write(directory, name, scene):
    path = os.path.join(directory, name)
    with open(path, "w") as f:
        json.dump(scene, f)
    return path


def test_scene_builder_properties(tmp_path):
    d = str(tmp_path)
    S.write_models(d)
    for name, shape in (("bumpy", (12, 17)), ("bumpy_small", (9, 13))):
        with open(os.path.join(d, "models", name + ".obj"), "w") as f:
            f.write(_bumpy_sphere_obj(*shape))
    args = []
    for agg in ("bvh", "group"):
        args += ["--pair", S.write_scene(d, "a_%s.json" % agg, S.TRANSFORMS_A, aggregate=agg), S.write_scene(d, "b_%s.json" % agg, S.TRANSFORMS_B, aggregate=agg)]
    args += ["--pair", _write(d, "many_a.json", _many_instances(0.0)), _write(d, "many_b.json", _many_instances(2.5))]
    args += ["--pair", _write(d, "fits_a.json", _many_instances(0.0, "bumpy_small")), _write(d, "fits_b.json", _many_instances(2.5, "bumpy_small"))]
    # the reference's own test scenes, beside their models
    ref = os.path.join(d, "reference_scenes")
    shutil.copytree(REFERENCE_SCENES, ref)
    args += ["--scene", os.path.join(ref, "test_scene_00.json"), "--scene", os.path.join(ref, "test_scene_01.json")]
    # Catmull-Clark control meshes of the reference, as patches (the library with the Bezier primitive builds these)
    cc = S.scene_dict(S.TRANSFORMS_A)
    cc["light_sampler"] = "uniform"
    cc["surfaces"] = []
    cc["instances"] = [i for i in cc["instances"] if i["name"] != "lamp"]
    cc["primitives"] += [{"type": "catmull_clark", "name": "cc_p", "ply_file": "reference_scenes/models/letter-p.ply", "fas_times": 1},
                         {"type": "catmull_clark", "name": "cc_cube", "ply_file": "reference_scenes/models/cube.ply", "fas_times": 2}]
    for k in range(6):
        cc["instances"].append({"name": "p%d" % k, "primitive": ("cc_p", "cc_cube")[k % 2], "material": "m_red", "scale": [0.3, 0.3, 0.3],
                                "rotate": [0.0, 30.0 * k, 10.0], "translate": [k - 2.5, 0.2, -1.0]})
    args += ["--scene", _write(d, "patches.json", cc)]

    # (a first build compiles the builder under the sanitizers, some 20 - 30 s; the program itself runs in under a second)
    res = subprocess.run(["make", "-s", "-C", _util.ROOT, "host", "scene-build-check"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    res = subprocess.run([os.path.join(_util.ROOT, "build", "selftest", "scene_build_check")] + args, capture_output=True, text=True, timeout=30)
    report = res.stdout + res.stderr
    assert res.returncode == 0, report
    assert "scene_build_check ok" in res.stdout
    assert "skipped" not in res.stdout, report          # every file above is one the loader accepts
    for word in ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer", "CHECK failed"):
        assert word not in report, report
    # each scene went through the four option sets, and the large generated scene really has the shapes it is there for
    lines = [l.split() for l in res.stdout.splitlines() if l.startswith("digest ")]
    assert len(lines) == 4 * 11
    many = {l[2]: dict(kv.split("=") for kv in l[3:]) for l in lines if l[1] == "many_a.json"}
    assert many["default"]["lds_geo"] == "0" and many["default"]["n4"] == "1" and many["default"]["swalk"] == "1" and many["nostream"]["swalk"] == "0"
    assert int(many["default"]["depth"].split("/")[1]) > 3 and many["reference"]["own_bvh"] == "0"
    for name in ("a_bvh.json", "fits_a.json"):
        small = {l[2]: dict(kv.split("=") for kv in l[3:]) for l in lines if l[1] == name}
        assert small["default"]["lds_geo"] == "1" and small["large"]["lds_geo"] == "0" and small["reference"]["lds_geo"] == "1"
