"""spt_hits without a device: the layout of its structs (include/spt_abi.h as a C compiler sees it, against the binding's ctypes and
numpy declarations), the exports of both libraries and the refusals that need no scene, and tests/_hits_ref.py - the float32 numpy
restatement every expected value of tests/test_gpu_hits.py comes from - anchored to the CPU oracle and shown to be not trivial.

The census of the reference (share of the batch's rays with 0 / 1 / 2 / 3-4 / more than 4 crossings; with the exit root of a sphere;
with two crossings of equal t), per scene and batch; every threshold asserted below is half of the figure here:

  cfg2_cube    grid     0.861 0.000 0.139 0.000 0.000   exit 0.000  tied 0.000
               random   0.201 0.208 0.591 0.000 0.000   exit 0.000  tied 0.000
               through  0.044 0.000 0.956 0.000 0.000   exit 0.000  tied 0.000
               edges    0.122 0.098 0.564 0.216 0.000   exit 0.000  tied 0.230
  t_materials  grid     0.450 0.196 0.093 0.235 0.027   exit 0.260  tied 0.000
               random   0.487 0.314 0.059 0.121 0.019   exit 0.170  tied 0.000
               through  0.005 0.163 0.158 0.564 0.111   exit 0.590  tied 0.000
               edges    0.006 0.101 0.106 0.654 0.133   exit 0.205  tied 0.151
  t_textured   grid     0.482 0.123 0.008 0.370 0.017   exit 0.226  tied 0.000
               random   0.518 0.361 0.033 0.073 0.014   exit 0.087  tied 0.000
               through  0.004 0.176 0.084 0.595 0.141   exit 0.505  tied 0.000
               edges    0.005 0.091 0.098 0.656 0.150   exit 0.195  tied 0.156

(the variants ":short", ":window" and ":past" of each batch are printed by test_the_census_is_not_trivial; a segment of extent / 16
from the batch's own origin reaches next to nothing, which is why ":window" moves it to the first surface).  Every base batch has
more than one ray in ten with two or more crossings."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import _hits_ref as ref
import _util

spt = _util.load_pkg()
f32 = np.float32

CAMERAS = {"cfg2_cube": None, "t_materials": "main", "t_textured": None}
# half of the docstring's figures: (two or more crossings, exit root, tied)
FLOOR = {
    ("cfg2_cube", "grid"): (0.069, 0.0, 0.0), ("cfg2_cube", "random"): (0.295, 0.0, 0.0), ("cfg2_cube", "through"): (0.478, 0.0, 0.0),
    ("cfg2_cube", "edges"): (0.390, 0.0, 0.115),
    ("t_materials", "grid"): (0.177, 0.130, 0.0), ("t_materials", "random"): (0.099, 0.085, 0.0), ("t_materials", "through"): (0.416, 0.295, 0.0),
    ("t_materials", "edges"): (0.446, 0.102, 0.075),
    ("t_textured", "grid"): (0.197, 0.113, 0.0), ("t_textured", "random"): (0.060, 0.043, 0.0), ("t_textured", "through"): (0.410, 0.252, 0.0),
    ("t_textured", "edges"): (0.452, 0.097, 0.078),
}


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    cc = shutil.which(os.environ.get("CC", "cc")) or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no C compiler"
    exe = str(tmp_path_factory.mktemp("hits_layout") / "hits_layout_check")
    src = os.path.join(_util.ROOT, "tests", "hits_layout_check.c")
    res = subprocess.run([cc, "-Wall", "-Wextra", "-I", os.path.join(_util.ROOT, "include"), "-o", exe, src], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    return {k: int(v) for k, v in (line.split() for line in out.stdout.splitlines())}


def test_the_hit_record_is_two_16_byte_words(c_layout):
    assert c_layout["sizeof.spt_hit_rec"] == spt.HIT_REC_DTYPE.itemsize == 32
    want = {"t": 0, "instance": 4, "prim": 8, "flags": 12, "v": 16, "w": 20, "pad": 24}
    assert list(spt.HIT_REC_DTYPE.names) == list(want)
    for f, off in want.items():
        assert c_layout["spt_hit_rec." + f] == spt.HIT_REC_DTYPE.fields[f][1] == off, f
    for f, kind in (("t", "<f4"), ("instance", "<i4"), ("prim", "<i4"), ("flags", "<u4"), ("v", "<f4"), ("w", "<f4"), ("pad", "<u4")):
        assert spt.HIT_REC_DTYPE.fields[f][0].base == np.dtype(kind), f
    assert c_layout["sizeof.spt_hit_count"] == spt.HIT_COUNT_DTYPE.itemsize == 8
    assert (c_layout["spt_hit_count.total"], c_layout["spt_hit_count.back"]) == (spt.HIT_COUNT_DTYPE.fields["total"][1], spt.HIT_COUNT_DTYPE.fields["back"][1]) == (0, 4)
    assert c_layout["sizeof.spt_ray"] == spt.RAY_DTYPE.itemsize == 32
    for f in ("o", "t_min", "d", "t_max"):
        assert c_layout["spt_ray." + f] == spt.RAY_DTYPE.fields[f][1], f


def test_the_binding_declares_the_headers_job(c_layout):
    assert c_layout["SPT_ABI_VERSION"] == spt.SPT_ABI_VERSION == 14
    assert c_layout["sizeof.spt_hits_job"] == C.sizeof(spt.HitsJob) == 48
    want = {"size": 0, "flags": 4, "n_rays": 8, "rays": 16, "hits": 24, "counts": 32, "max_hits": 40, "rays_per_pass": 44}
    assert [f for f, _ in spt.HitsJob._fields_] == list(want)
    for f, off in want.items():
        assert c_layout["spt_hits_job." + f] == getattr(spt.HitsJob, f).offset == off, f
    assert (c_layout["SPT_HITS_DEVICE_POINTERS"], c_layout["SPT_HITS_COUNT_ALL"]) == (spt.HITS_DEVICE_POINTERS, spt.HITS_COUNT_ALL) == (1, 2)
    assert c_layout["SPT_HIT_BACKFACING"] == spt.HIT_BACKFACING == ref.BACKFACING == c_layout["SPT_GBUF_BACKFACING"] == 1
    assert (c_layout["SPT_PRIM_SPHERE"], c_layout["SPT_PRIM_MESH"]) == (ref.PRIM_SPHERE, ref.PRIM_MESH)


def test_both_libraries_export_the_call_and_refuse_without_a_scene():
    lib = spt.hip_lib()
    bez = C.CDLL(os.path.join(spt.LIB_DIR, "libspt_hip_bez.so"))
    assert hasattr(lib, "spt_hits") and hasattr(bez, "spt_hits")
    job = spt.HitsJob(size=C.sizeof(spt.HitsJob), max_hits=1)
    assert lib.spt_hits(None, C.byref(job)) == 1      # SPT_ERR_INVALID_ARG
    assert b"hits" in lib.spt_last_error()
    assert lib.spt_hits(None, None) == 1


# ---- the reference, anchored to the CPU oracle

@functools.lru_cache(maxsize=None)
def _scene(name):
    _util.ensure_cpu_build()
    return spt.load_scene(os.path.join(_util.SCENES, name + ".json"))


@functools.lru_cache(maxsize=None)
def _batches(name):
    return ref.batches(spt, _scene(name), CAMERAS[name])


@functools.lru_cache(maxsize=None)
def _crossings(name, batch):
    return ref.crossings(_scene(name), _batches(name)[batch])


def _hit_words(hits):
    """HIT_DTYPE records as (n, 5) uint32."""
    return np.ascontiguousarray(hits).view(np.uint32).reshape(-1, 5)


def _rec_as_hit(rec):
    """The (t, instance, prim, v, w) of HIT_REC_DTYPE records as HIT_DTYPE records."""
    out = np.zeros(rec.shape, dtype=spt.HIT_DTYPE)
    for f in ("t", "instance", "prim", "v", "w"):
        out[f] = rec[f]
    return out


@pytest.mark.parametrize("name", list(CAMERAS))
def test_record_0_is_the_oracles_closest_hit(name):
    scene = _scene(name)
    n = 0
    for batch, rays in _batches(name).items():
        rec, counts = ref.records(spt, _crossings(name, batch), 1)
        want = _util.oracle_trace_closest(scene, rays, _util.ORACLE_EXHAUSTIVE)
        assert np.array_equal(_hit_words(_rec_as_hit(rec[:, 0])), _hit_words(want)), batch
        assert np.array_equal(counts["total"] > 0, want["instance"] >= 0), batch
        n += int((want["instance"] >= 0).sum())
    assert n > 1000


@pytest.mark.parametrize("name", list(CAMERAS))
def test_record_j_plus_1_is_the_oracles_closest_hit_behind_record_j(name):
    """For a triangle record j whose successor does not tie it in t, the closest hit of the same ray with t_min = t_j is record j + 1."""
    scene = _scene(name)
    checked = 0
    for batch, rays in _batches(name).items():
        if ":" in batch:
            continue
        K = 6
        rec, _ = ref.records(spt, _crossings(name, batch), K)
        for j in range(K - 1):
            a, b = rec[:, j], rec[:, j + 1]
            ok = (a["instance"] >= 0) & (b["instance"] >= 0) & ((a["flags"] >> 8) == ref.PRIM_MESH) & (a["t"] != b["t"])
            behind = rays[ok].copy()
            behind["t_min"] = a["t"][ok]
            want = _util.oracle_trace_closest(scene, behind, _util.ORACLE_EXHAUSTIVE)
            assert np.array_equal(_hit_words(_rec_as_hit(b[ok])), _hit_words(want)), (batch, j)
            checked += int(ok.sum())
    assert checked > 1000


def test_total_is_the_oracles_any_hit_on_the_scene_without_spheres():
    name = "cfg2_cube"
    scene = _scene(name)
    assert len(scene.array("spheres")) == 0
    seen = set()
    for batch, rays in _batches(name).items():
        _, counts = ref.records(spt, _crossings(name, batch), 0, count_all=True)
        want = _util.oracle_trace_any(scene, rays, _util.ORACLE_EXHAUSTIVE)
        assert np.array_equal((counts["total"] > 0).astype(np.uint8), want), batch
        seen |= set(want.tolist())
    assert seen == {0, 1}


@pytest.mark.parametrize("name", list(CAMERAS))
def test_the_census_is_not_trivial(name):
    scene = _scene(name)
    for batch in _batches(name):
        c = ref.census(_crossings(name, batch))
        print("%-12s %-15s %.3f %.3f %.3f %.3f %.3f   exit %.3f  tied %.3f" % (name, batch, c["0"], c["1"], c["2"], c["3-4"], c[">4"], c["exit"], c["tied"]))
        if ":" in batch:
            continue
        two_or_more = c["2"] + c["3-4"] + c[">4"]
        assert two_or_more > 0.1, batch      # (a batch below that is changed, not its threshold)
        floor = FLOOR[(name, batch)]
        assert two_or_more >= floor[0] and c["exit"] >= floor[1] and c["tied"] >= floor[2], (batch, c)
    # the variants do what they are for: a window around the first surface ends between crossings, and past the first crossing one is gone
    for batch in ("grid", "through", "edges"):
        full, win, past = (ref.rank(_crossings(name, batch + v))[1] for v in ("", ":window", ":past"))
        assert ((win > 0) & (win < full)).mean() > 0.05, batch
        gone = full[full > 0] - past[full > 0]
        assert (gone >= 1).all() and (batch == "edges" or (gone == 1).all()), batch      # (a crossing that ties the first in t goes with it)
    assert len(scene.array("spheres")) == 0 or ref.census(_crossings(name, "through"))["exit"] > 0.1


@pytest.mark.parametrize("name", list(CAMERAS) + ["t_medium"])
def test_no_test_ray_has_a_sphere_root_at_its_t_min(name):
    scene = _scene(name)
    for batch, rays in ref.batches(spt, scene, CAMERAS.get(name)).items():
        assert ref.sphere_root_at_t_min(scene, rays) == 0, batch


def test_the_key_orders_ties_by_instance_prim_and_facing():
    """The sort of the reference on a hand-made list: the key is (t, instance, prim, backfacing)."""
    cr = {"ray": np.zeros(5, dtype=np.int64), "t": np.array([2, 1, 1, 1, 1], dtype=f32), "instance": np.array([0, 3, 2, 2, 2], dtype=np.int32),
          "prim": np.array([0, 0, 7, 5, 5], dtype=np.int32), "back": np.array([0, 0, 0, 1, 0], dtype=np.uint32), "ptype": np.ones(5, dtype=np.uint32),
          "v": np.zeros(5, dtype=f32), "w": np.zeros(5, dtype=f32)}
    order = np.lexsort((cr["back"], cr["prim"], cr["instance"], cr["t"], cr["ray"]))
    assert order.tolist() == [4, 3, 2, 1, 0]
    cr = {k: v[order] for k, v in cr.items()}
    cr["n_rays"] = 2
    rec, counts = ref.records(spt, cr, 3)
    assert rec["prim"].tolist() == [[5, 5, 7], [-1, -1, -1]] and rec["flags"][0].tolist() == [1 << 8, 1 | (1 << 8), 1 << 8]
    assert counts.tolist() == [(3, 1), (0, 0)]
    assert ref.records(spt, cr, 3, count_all=True)[1].tolist() == [(5, 1), (0, 0)]
    assert rec["t"][1].tolist() == [ref.F32_MAX] * 3 and not ref.words(rec)[1, :, 3:].any()
