"""Reconstruction filters of sample-keeping films (spt_film_filter): the header, the binding and the renderer loader agree.  No GPU."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _util

spt = _util.load_pkg()
INVALID, SCHEMA = 1, 102
BASE = {"type": "pt", "max_depth": 5, "sampler": {"type": "random", "spp": 4}}
THIRD = float(np.float32(1.0 / 3.0))


def test_header_and_binding_constants_agree():
    text = open(os.path.join(_util.ROOT, "include", "spt_abi.h")).read()
    assert re.search(r"enum \{ SPT_FILTER_BOX = 0, SPT_FILTER_TENT = 1, SPT_FILTER_GAUSSIAN = 2, SPT_FILTER_MITCHELL = 3 \};", text)
    assert re.search(r"spt_status spt_film_filter\(spt_film\* film, const spt_filter_desc\* desc\);", text)
    assert re.search(r"#define\s+SPT_ABI_VERSION\s+14\b", text) and spt.SPT_ABI_VERSION == 14      # additive: the version stays
    assert spt.FILTER_TYPES == {"box": 0, "tent": 1, "gaussian": 2, "mitchell": 3}
    host = open(os.path.join(_util.ROOT, "include", "spt_host.h")).read()
    assert re.search(r"spt_status spt_host_load_renderer_filter\(const char\* renderer_json_path, spt_render_params\* params,\s*spt_filter_desc\* filter\);", host)


def test_desc_size_in_c_and_ctypes(tmp_path):
    cc = shutil.which(os.environ.get("CC", "cc")) or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no C compiler"
    src = tmp_path / "filter_layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "spt_abi.h"\n'
                   "int main(void) {\n"
                   '    printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(spt_filter_desc), offsetof(spt_filter_desc, size), offsetof(spt_filter_desc, type),\n'
                   "           offsetof(spt_filter_desc, radius), offsetof(spt_filter_desc, p0), offsetof(spt_filter_desc, p1), offsetof(spt_filter_desc, pad));\n"
                   "    return 0;\n}\n")
    exe = str(tmp_path / "filter_layout")
    res = subprocess.run([cc, "-Wall", "-Wextra", "-I", os.path.join(_util.ROOT, "include"), "-o", exe, str(src)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    D = spt.FilterDesc
    assert [int(v) for v in out.stdout.split()] == [24, 0, 4, 8, 12, 16, 20]
    assert [C.sizeof(D), D.size.offset, D.type.offset, D.radius.offset, D.p0.offset, D.p1.offset, D.pad.offset] == [24, 0, 4, 8, 12, 16, 20]


def test_null_arguments_need_no_device():
    _util.ensure_cpu_build()
    lib = spt.hip_lib()
    desc = spt.filter_desc("tent", 1.0)
    assert (desc.size, desc.type, desc.radius) == (24, 1, 1.0)
    assert lib.spt_film_filter(None, C.byref(desc)) == INVALID
    assert b"null" in lib.spt_last_error()
    fake = C.create_string_buffer(64)          # never read: the null desc is refused first
    assert lib.spt_film_filter(C.cast(fake, C.c_void_p), None) == INVALID


def _load(tmp_path, flt):
    path = tmp_path / "r.json"
    path.write_text(json.dumps(dict(BASE, filter=flt)))
    p, fd = spt.RenderParams(), spt.FilterDesc()
    status = spt.host_lib().spt_host_load_renderer_filter(str(path).encode(), C.byref(p), C.byref(fd))
    return status, p, fd, str(path)


@pytest.mark.parametrize("flt,want", [
    ({"type": "box", "radius": 0.5}, (0, 0.5, 0.0, 0.0)),
    ({"type": "box", "radius": 1.5}, (0, 1.5, 0.0, 0.0)),
    ({"type": "tent", "radius": 1.0}, (1, 1.0, 0.0, 0.0)),
    ({"type": "gaussian", "radius": 1.5, "alpha": 3.0}, (2, 1.5, 3.0, 0.0)),
    ({"type": "gaussian", "radius": 1.5}, (2, 1.5, 2.0, 0.0)),
    ({"type": "mitchell", "radius": 1.5, "b": 0.5, "c": 0.25}, (3, 1.5, 0.5, 0.25)),
    ({"type": "mitchell"}, (3, 2.0, THIRD, THIRD)),
    ({"type": "mitchell", "b": 1.0}, (3, 2.0, 1.0, THIRD)),
])
def test_loader_returns_the_desc(tmp_path, flt, want):
    status, p, fd, path = _load(tmp_path, flt)
    assert status == 0, spt.host_lib().spt_host_last_error()
    assert (fd.size, fd.type, fd.radius, fd.p0, fd.p1, fd.pad) == (24,) + want + (0,)
    # the radius decides the halo a sample-keeping film stores
    assert p.filter_radius == want[1] and bool(p.flags & spt.RENDER_BOX_RADIUS) == (want[1] != 0.5)
    assert (p.max_depth, p.spp, p.sampler) == (5, 4, spt.SAMPLER_RANDOM)
    r = spt.load_renderer(path)
    kind = ["box", "tent", "gaussian", "mitchell"][want[0]]
    assert r.filter_type == kind and r.filter_radius == want[1]
    assert r.filter_params == ({"alpha": want[2]} if kind == "gaussian" else {"b": want[2], "c": want[3]} if kind == "mitchell" else {})


@pytest.mark.parametrize("flt,msg", [
    ({"type": "tent", "radius": 1}, "float"),
    ({"type": "box", "radius": 1}, "float"),
    ({"type": "gaussian", "radius": 1.5, "alpha": 2}, "float"),
    ({"type": "mitchell", "radius": 2}, "float"),
    ({"type": "mitchell", "b": 1}, "float"),
    ({"type": "tent"}, "radius"),
    ({"type": "lanczos", "radius": 2.0}, "unknown type"),
])
def test_loader_schema_errors(tmp_path, flt, msg):
    status, _, _, path = _load(tmp_path, flt)
    assert status == SCHEMA
    assert msg in spt.host_lib().spt_host_last_error().decode()
    with pytest.raises(spt.SptError):
        spt.load_renderer(path)


@pytest.mark.parametrize("kind", ["tent", "gaussian", "mitchell"])
def test_the_old_loader_still_refuses_weighted_filters(tmp_path, kind):
    path = tmp_path / "r.json"
    path.write_text(json.dumps(dict(BASE, filter={"type": kind, "radius": 1.5})))
    p, radius = spt.RenderParams(), C.c_float(-1.0)
    assert spt.host_lib().spt_host_load_renderer(str(path).encode(), C.byref(p), C.byref(radius)) == SCHEMA
    assert ("unknown type '%s'" % kind) in spt.host_lib().spt_host_last_error().decode()
    assert radius.value == -1.0 and p.spp == 0          # a caller of the old function gets no box in its place


def test_plans_that_reach_spt_render_refuse_a_weighted_filter():
    # spt_render knows the box only and the plan carries just the radius: handing it on would be a silent box
    from test_multi_device import StubDevices
    sc = spt.load_scene(os.path.join(_util.SCENES, "cfg2_cube.json"))
    stub = StubDevices(sc)
    md = spt.MultiDevice(sc, [0, 1], api=stub.api)
    try:
        for kind in ("tent", "gaussian", "mitchell"):
            r = spt.PathTracer(max_depth=2, sampler=spt.SAMPLER_RANDOM, spp=1, seed=1, filter_radius=1.5, filter_type=kind)
            with pytest.raises(spt.SptError) as e:
                md.render(r, spt.OutputConfig(8, 8))
            assert kind in str(e.value) and stub.calls == []
            with pytest.raises(spt.SptError):
                md.progressive(r, spt.OutputConfig(8, 8), keep_samples=True)
        box = spt.PathTracer(max_depth=2, sampler=spt.SAMPLER_RANDOM, spp=1, seed=1)
        assert md.render(box, spt.OutputConfig(8, 8)).shape == (8, 8, 3) and len(stub.calls) == 2
    finally:
        md.close()
        sc.close()
    # the single-device film refuses it without the sample store, before it touches a device
    r = spt.PathTracer(filter_radius=1.0, filter_type="tent")
    with pytest.raises(spt.SptError) as e:
        spt.ProgressiveFilm(r, None, spt.OutputConfig(8, 8))
    assert "keep_samples" in str(e.value)


def test_binding_surface():
    import inspect
    assert list(inspect.signature(spt.ProgressiveFilm.set_filter).parameters) == ["self", "kind", "radius", "alpha", "b", "c"]
    r = spt.PathTracer()
    assert r.filter_type == "box" and r.filter_params == {}
    with pytest.raises(ValueError):
        spt.PathTracer(filter_type="lanczos")
    d = spt.filter_desc("mitchell")
    assert (d.type, d.radius) == (3, 2.0) and d.p0 == d.p1 == THIRD
    d = spt.filter_desc("gaussian", 1.5)
    assert (d.type, d.radius, d.p0) == (2, 1.5, 2.0)
    # a plan whose halo a Gaussian of radius 1.5 needs: the weighted filter's radius is the plan's
    p = spt.PathTracer(filter_type="gaussian", filter_radius=1.5).params(8, 8)
    assert p.flags & spt.RENDER_BOX_RADIUS and p.filter_radius == 1.5
