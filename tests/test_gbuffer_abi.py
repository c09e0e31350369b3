"""spt_gbuffer without a device: the layout of its structs (include/spt_abi.h as a C compiler sees it, against the binding's ctypes and
numpy declarations), the refusals of the command-line program that come before any device is touched, and the sources of
tests/_gbuffer_ref.py held to the oracle on pinhole rays, so that the GPU tests compare with values that were checked here."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _anywhere_ref
import _gbuffer_ref
import _util

spt = _util.load_pkg()
f32 = np.float32


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    cc = shutil.which(os.environ.get("CC", "cc")) or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no C compiler"
    exe = str(tmp_path_factory.mktemp("gbuffer_layout") / "gbuffer_layout_check")
    src = os.path.join(_util.ROOT, "tests", "gbuffer_layout_check.c")
    res = subprocess.run([cc, "-Wall", "-Wextra", "-I", os.path.join(_util.ROOT, "include"), "-o", exe, src], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    return {k: int(v) for k, v in (line.split() for line in out.stdout.splitlines())}


def test_the_record_is_four_16_byte_words(c_layout):
    assert c_layout["sizeof.spt_gbuffer_rec"] == 64
    want = {"p": 0, "t": 12, "n": 16, "instance": 28, "albedo": 32, "prim": 44, "v": 48, "w": 52, "surface": 56, "flags": 60}
    for f, off in want.items():
        assert c_layout["spt_gbuffer_rec." + f] == off, f
    assert (c_layout["sizeof.spt_path_ray"], c_layout["sizeof.spt_ray_aux"]) == (48, 64)


def test_the_binding_declares_the_headers_layout(c_layout):
    assert c_layout["SPT_ABI_VERSION"] == spt.SPT_ABI_VERSION == 14
    assert spt.GBUFFER_DTYPE.itemsize == c_layout["sizeof.spt_gbuffer_rec"]
    assert list(spt.GBUFFER_DTYPE.names) == ["p", "t", "n", "instance", "albedo", "prim", "v", "w", "surface", "flags"]
    for f in spt.GBUFFER_DTYPE.names:
        assert c_layout["spt_gbuffer_rec." + f] == spt.GBUFFER_DTYPE.fields[f][1], f
    for f, kind in (("p", "<f4"), ("t", "<f4"), ("n", "<f4"), ("instance", "<i4"), ("albedo", "<f4"), ("prim", "<i4"), ("v", "<f4"), ("w", "<f4"),
                    ("surface", "<u4"), ("flags", "<u4")):
        assert spt.GBUFFER_DTYPE.fields[f][0].base == np.dtype(kind), f
    assert c_layout["sizeof.spt_gbuffer_job"] == C.sizeof(spt.GBufferJob) == 48
    want = {"size": 0, "flags": 4, "n_rays": 8, "rays": 16, "aux": 24, "rays_per_pass": 32, "pad": 36, "out": 40}
    assert [f for f, _ in spt.GBufferJob._fields_] == list(want)
    for f, off in want.items():
        assert c_layout["spt_gbuffer_job." + f] == getattr(spt.GBufferJob, f).offset == off, f
    assert (c_layout["SPT_GBUFFER_DEVICE_POINTERS"], c_layout["SPT_GBUF_BACKFACING"], c_layout["SPT_GBUF_LIGHT"]) == \
        (spt.GBUFFER_DEVICE_POINTERS, spt.GBUF_BACKFACING, spt.GBUF_LIGHT) == (1, 1, 2)


def test_both_libraries_export_the_call():
    lib = spt.hip_lib()
    assert hasattr(lib, "spt_gbuffer")
    bez = C.CDLL(os.path.join(spt.LIB_DIR, "libspt_hip_bez.so"))
    assert hasattr(bez, "spt_gbuffer")
    # the two refusals that need no scene
    job = spt.GBufferJob(size=C.sizeof(spt.GBufferJob))
    assert lib.spt_gbuffer(None, C.byref(job)) == 1      # SPT_ERR_INVALID_ARG
    assert b"gbuffer" in lib.spt_last_error()


def test_camera_gbuffer_wants_a_sample():
    with pytest.raises(ValueError):
        spt.camera_gbuffer(None, None, None, 4, 4, samples=0)


# ---- the reference's own sources, on the CPU

@pytest.mark.parametrize("name", ["t_materials", "t_textured", "t_bezier"])
def test_reference_normals_are_the_oracles_debug_normals(name):
    """_gbuffer_ref.normals (meshes: _bake_ref.resolve; spheres: restated there) through n * 0.5 + 0.5 has the words of the oracle's
    SPT_RENDER_DEBUG_NORMAL film at every hit pixel of a 48 x 36 pinhole grid whose primitive has a reference normal."""
    scene = _anywhere_ref.scene(name)
    rays, film = _gbuffer_ref.debug_normal_words(scene, 48, 36, camera=_anywhere_ref.CAMERAS[name])
    hits = _util.oracle_trace_closest(scene, _util.first_segments(rays), _util.device_oracle_flags())
    n, known = _gbuffer_ref.normals(scene, rays, hits)
    hit = hits["instance"] >= 0
    kinds = scene.array("instances")["prim_type"][np.maximum(hits["instance"], 0)]
    for kind in (_gbuffer_ref.PRIM_SPHERE, _gbuffer_ref.PRIM_MESH):
        assert known[hit & (kinds == kind)].all()
    assert not known[hit & (kinds == _gbuffer_ref.PRIM_BEZIER)].any()
    assert (hit & known).sum() >= 400
    if name != "t_bezier":
        assert (hit & (kinds == _gbuffer_ref.PRIM_SPHERE)).sum() >= 100
    w = n * f32(0.5) + f32(0.5)
    assert np.array_equal(w[hit & known].view(np.uint32), film[hit & known].view(np.uint32))


@pytest.mark.parametrize("name,kind,share,distinct", [
    ("t_materials", "free", 0.15, 0), ("t_materials", "thin_lens", 0.15, 0), ("t_materials", "axes", 0.15, 0),
    ("t_textured", "free", 0.15, 50), ("t_textured", "thin_lens", 0.15, 50), ("t_textured", "axes", 0.15, 50),
    ("t_bezier", "thin_lens", 0.15, 0),
])
def test_the_expected_records_are_not_trivial(name, kind, share, distinct):
    rays, aux, _ = _anywhere_ref.make(name, kind)
    rec, known = _gbuffer_ref.expected(_anywhere_ref.scene(name), rays, aux)
    got_share, got_distinct = _gbuffer_ref.census(rec)
    print("%s, %s: %d rays, hit share %.2f, %d distinct albedos" % (name, kind, rec.shape[0], got_share, got_distinct))
    assert got_share >= share and got_distinct >= distinct
    hit = rec["instance"] >= 0
    miss = _gbuffer_ref.words(rec[~hit])
    assert (~hit).any() and (miss[:, [0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14, 15]] == 0).all() and (rec["t"][~hit] == np.finfo(f32).max).all()
    assert (rec["flags"][hit] >> 8 <= 2).all() and np.isfinite(rec["p"][hit]).all()
    if name != "t_bezier":
        assert known.all()


# ---- the command-line program's refusals (before any device is touched)

def _cli():
    cli = os.path.join(spt.LIB_DIR, "spt")
    if not os.path.exists(cli):
        subprocess.check_call(["make", "-s", "-C", _util.ROOT, "cli"])
    return [cli, "-s", os.path.join(_util.SCENES, "cfg2_cube.json"), "-r", os.path.join(_util.SCENES, "pt.json")]


@pytest.mark.parametrize("extra,word", [
    (["--gpus", "2"], "one device"), (["--devices", "0,0"], "one device"), (["--film-devices", "0,0", "--preview-every", "2"], "one device"),
    (["--animate", "frames.json"], "--animate"), (["--bake-lightmap", "cube", "--bake-size", "16x16"], "--bake-lightmap"),
    (["--bake-probes", "points.txt"], "--bake-probes"), (["--gbuffer-samples", "0"], "N >= 1"),
], ids=lambda e: e[0] if isinstance(e, list) else None)
def test_the_cli_refuses_a_gbuffer_beside_another_mode(tmp_path, extra, word):
    stem = str(tmp_path / "g")
    res = subprocess.run(_cli() + ["-o", str(tmp_path / "o.png"), "--gbuffer-out", stem] + extra, capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and "--gbuffer-" in res.stderr and word in res.stderr, res.stdout + res.stderr
    assert os.listdir(tmp_path) == []


def test_the_cli_wants_a_stem_for_the_sample_count(tmp_path):
    res = subprocess.run(_cli() + ["-o", str(tmp_path / "o.png"), "--gbuffer-samples", "2"], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and "--gbuffer-out" in res.stderr, res.stdout + res.stderr
    res = subprocess.run(_cli(), capture_output=True, text=True, timeout=60)      # neither -o nor --gbuffer-out: the usage
    assert res.returncode == 2 and "--gbuffer-out" in res.stderr
