"""Moving the instances of a loaded scene on the host (spt_host_scene_set_transforms / _set_light), the layout of
spt_scene_update_desc and the refusals of `spt --animate`: nothing here needs a device.

The contract of set_transforms: the descriptor afterwards is the one the loader makes of the scene file with those transforms
written in - instances (inv, fwd, nrm, world box, light), their order, tlas_nodes, the shape lights' power and the alias table,
byte for byte."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import _scene_update_scenes as S
import _util

spt = _util.load_pkg()
CLI = os.path.join(spt.LIB_DIR, "spt")
NAMES = sorted(S.TRANSFORMS_A)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("scene_update_host")
    return {"dir": d, "a": S.write_scene(d, "a.json", S.TRANSFORMS_A), "b": S.write_scene(d, "b.json", S.TRANSFORMS_B), "pt": S.write_renderer(d)}


def _same(spt_mod, got, want):
    g, w = S.dynamic_bytes(spt_mod, got), S.dynamic_bytes(spt_mod, want)
    for key in w:
        assert g[key] == w[key], key


def test_set_transforms_gives_the_loaders_descriptor(files):
    a, b = spt.load_scene(files["a"]), spt.load_scene(files["b"])
    before = S.dynamic_bytes(spt, a)
    assert before["instances"] != S.dynamic_bytes(spt, b)["instances"]
    assert before["alias_props"] != S.dynamic_bytes(spt, b)["alias_props"]      # (the lamp's area, and so its power, differs)
    assert b.desc.light_alias.n == b.desc.n_lights == 2
    a.set_transforms(S.fwd_by_name(b, NAMES))
    _same(spt, a, b)
    for n in NAMES:
        assert a.instance_index(n) == b.instance_index(n)
    # static arrays are untouched
    assert a.array("tri_pos").tobytes() == b.array("tri_pos").tobytes()


def test_group_aggregate_too(files):
    d = files["dir"]
    a, b = spt.load_scene(S.write_scene(d, "ga.json", S.TRANSFORMS_A, aggregate="group")), spt.load_scene(S.write_scene(d, "gb.json", S.TRANSFORMS_B, aggregate="group"))
    a.set_transforms(S.fwd_by_name(b, NAMES))
    _same(spt, a, b)


def test_round_trip(files):
    a, b = spt.load_scene(files["a"]), spt.load_scene(files["b"])
    fresh = spt.load_scene(files["a"])
    own = S.fwd_by_name(a, NAMES)
    a.set_transforms(S.fwd_by_name(b, NAMES))
    a.set_transforms(own)
    _same(spt, a, fresh)
    # a subset, as a 3x4 matrix [M | t]
    f = S.fwd_by_name(b, ["cube_l"])["cube_l"]
    a.set_transforms({"cube_l": f.reshape(4, 3).T})
    want = spt.load_scene(S.write_scene(files["dir"], "a_cube.json", dict(S.TRANSFORMS_A, cube_l=S.TRANSFORMS_B["cube_l"])))
    _same(spt, a, want)


def test_set_light_moves_the_point_light(files):
    a = spt.load_scene(files["a"])
    want = spt.load_scene(S.write_scene(files["dir"], "a_bulb.json", S.TRANSFORMS_A, bulb=(-1.5, 3.0, 1.0)))
    lights = a.array("lights")
    k = int(np.flatnonzero(lights["type"] == 1)[0])
    light = spt.Light.from_buffer_copy(lights[k].tobytes())
    light.pos[:] = (-1.5, 3.0, 1.0)
    a.set_light("bulb", light)
    _same(spt, a, want)
    with pytest.raises(spt.SptError) as e:
        a.set_light("nobody", light)
    assert e.value.status == 102
    light.type = 2
    with pytest.raises(spt.SptError):
        a.set_light("bulb", light)
    _same(spt, a, want)


def test_refusals_leave_the_descriptor_unchanged(files):
    a = spt.load_scene(files["a"])
    before = S.dynamic_bytes(spt, a)
    good = S.fwd_by_name(spt.load_scene(files["b"]), ["cube_r"])["cube_r"]
    singular = good.copy()
    singular[3:6] = singular[0:3]       # two equal columns
    nan = good.copy()
    nan[10] = np.nan
    huge = good.copy()
    huge[9] = np.float32(3e38)
    huge[0] = np.float32(3e38)
    with pytest.raises(spt.SptError) as e:
        a.set_transforms({"cube_r": good, "nobody": good})
    assert e.value.status == 102        # SPT_HOST_ERR_SCHEMA
    lib, names = spt.host_lib(), (C.c_char_p * 2)(b"cube_r", b"cube_r")          # one instance named twice
    twice = np.concatenate([good, good]).astype(np.float32)
    assert lib.spt_host_scene_set_transforms(a._h, 2, names, twice.ctypes.data) == 1
    assert S.dynamic_bytes(spt, a) == before
    for bad in (singular, nan, huge, np.zeros(12, np.float32)):
        with pytest.raises(spt.SptError):
            a.set_transforms({"cube_l": good, "cube_r": bad})      # (the good one of the same call is not applied either)
        assert S.dynamic_bytes(spt, a) == before
    with pytest.raises(spt.SptError) as e:
        a.instance_index("nobody")
    assert e.value.status == 102
    assert S.dynamic_bytes(spt, a) == before


def test_update_desc_layout(tmp_path):
    cc = shutil.which(os.environ.get("CC", "cc")) or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no C compiler"
    exe = str(tmp_path / "scene_update_layout_check")
    src = os.path.join(_util.ROOT, "tests", "scene_update_layout_check.c")
    res = subprocess.run([cc, "-Wall", "-Wextra", "-I", os.path.join(_util.ROOT, "include"), "-o", exe, src], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    c = {k: int(v) for k, v in (line.split() for line in out.stdout.splitlines())}
    assert c["SPT_ABI_VERSION"] == 14 == spt.SPT_ABI_VERSION       # additive: detected by symbol
    assert C.sizeof(spt.SceneUpdateDesc) == c["sizeof.spt_scene_update_desc"]
    names = [f[0] for f in spt.SceneUpdateDesc._fields_]
    assert names == ["size", "flags", "n_tlas_nodes", "tlas_nodes", "n_instances", "instances", "n_lights", "lights", "light_alias"]
    for name in names:
        assert getattr(spt.SceneUpdateDesc, name).offset == c["spt_scene_update_desc." + name], name
    assert C.sizeof(spt.AliasTable) == c["sizeof.spt_alias_table"]
    assert C.sizeof(spt.Instance) == c["sizeof.spt_instance"] == 192
    assert C.sizeof(spt.Light) == c["sizeof.spt_light"] == 64
    assert C.sizeof(spt.BvhNode) == c["sizeof.spt_bvh_node"]
    with open(os.path.join(_util.ROOT, "include", "spt_abi.h")) as f:
        header = f.read()
    assert "spt_status spt_scene_update(spt_scene* scene, const spt_scene_update_desc* u);" in header


def _cli(files, tmp_path, animate, *extra):
    return subprocess.run([CLI, "-s", files["a"], "-r", files["pt"], "-o", str(tmp_path / "o.png"), "-w", "32", "-h", "24", "--animate", str(animate)] + list(extra),
                          capture_output=True, text=True, timeout=120)


def test_cli_animate_refusals(files, tmp_path):
    good = tmp_path / "good.json"
    good.write_text(json.dumps({"frames": [{"cube_l": S.TRANSFORMS_B["cube_l"]}]}))
    cases = {
        "not json": "{\"frames\": [",
        "no frames": json.dumps({"frame": []}),
        "frames no array": json.dumps({"frames": {"cube_l": {}}}),
        "frame no object": json.dumps({"frames": [[1.0]]}),
        "transform no object": json.dumps({"frames": [{"cube_l": [1.0, 2.0, 3.0]}]}),
        "no transform key": json.dumps({"frames": [{"cube_l": {"material": "m_red"}}]}),
        "unknown instance": json.dumps({"frames": [{"cube_l": S.TRANSFORMS_B["cube_l"]}, {"nobody": {"translate": [0.0, 1.0, 0.0]}}]}),
    }
    says = {"not json": "bad.json", "no frames": "'frames'", "frames no array": "'frames'", "frame no object": "a frame must be an object",
            "transform no object": "the transform of 'cube_l'", "no transform key": "no transform", "unknown instance": "no instance named 'nobody'"}
    for what, text in cases.items():
        path = tmp_path / "bad.json"
        path.write_text(text)
        r = _cli(files, tmp_path, path)
        assert r.returncode == 2, (what, r.returncode, r.stderr)
        assert "usage:" not in r.stderr and says[what] in r.stderr, (what, r.stderr)      # refused by the animation's loader, not as an unknown flag
    r = _cli(files, tmp_path, tmp_path / "missing.json")
    assert r.returncode == 2 and "missing.json" in r.stderr and "usage:" not in r.stderr
    for extra in (["--denoise"], ["--gpus", "2"], ["--film-devices", "0,0"], ["--preview-every", "1"], ["--time-limit", "1.0"], ["--adaptive", "0.1"], ["--robust", "3"]):
        r = _cli(files, tmp_path, good, *extra)
        assert r.returncode == 2, (extra, r.returncode, r.stderr)
        assert "--animate renders plain frames on one device" in r.stderr, (extra, r.stderr)
    assert not list(tmp_path.glob("o*.png"))
