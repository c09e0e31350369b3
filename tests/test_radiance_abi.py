"""spt_radiance in include/spt_abi.h and in the binding: the structs and the prototype are there, the binding's records have the
sizes and field offsets a C compiler gives the header's (tests/radiance_layout_check.c, compiled here), and the ABI version did
not move (the entry is additive: callers detect it by symbol)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import _util

spt = _util.load_pkg()
HEADER = os.path.join(_util.ROOT, "include", "spt_abi.h")


def test_header_declares_the_structs_and_the_entry():
    text = open(HEADER).read()
    for pattern in (r"typedef struct spt_path_ray \{", r"typedef struct spt_ray_aux \{", r"typedef struct spt_radiance_job \{",
                    r"enum \{ SPT_RADIANCE_DEVICE_POINTERS = 1u \};",
                    r"spt_status spt_radiance\(const spt_scene\* scene, const spt_radiance_job\* job\);"):
        assert re.search(pattern, text), pattern
    assert re.search(r"#define SPT_ABI_VERSION 14\b", text)
    assert spt.SPT_ABI_VERSION == 14


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    cc = shutil.which(os.environ.get("CC", "cc")) or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no C compiler"
    exe = str(tmp_path_factory.mktemp("radiance_layout") / "radiance_layout_check")
    src = os.path.join(_util.ROOT, "tests", "radiance_layout_check.c")
    res = subprocess.run([cc, "-Wall", "-Wextra", "-I", os.path.join(_util.ROOT, "include"), "-o", exe, src], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    return {k: int(v) for k, v in (line.split() for line in out.stdout.splitlines())}


def test_record_sizes(c_layout):
    assert spt.PATH_RAY_DTYPE.itemsize == 48 == c_layout["sizeof.spt_path_ray"]
    assert spt.RAY_AUX_DTYPE.itemsize == 64 == c_layout["sizeof.spt_ray_aux"]
    assert c_layout["SPT_ABI_VERSION"] == 14
    assert c_layout["SPT_RADIANCE_DEVICE_POINTERS"] == spt.RADIANCE_DEVICE_POINTERS == 1


def test_record_field_offsets(c_layout):
    for name in ("o", "t_min", "d", "stream_a", "stream_b", "pad"):
        assert spt.PATH_RAY_DTYPE.fields[name][1] == c_layout["spt_path_ray." + name], name
    for name in ("rx_o", "rx_d", "ry_o", "ry_d"):
        assert spt.RAY_AUX_DTYPE.fields[name][1] == c_layout["spt_ray_aux." + name], name


def test_job_layout(c_layout):
    assert C.sizeof(spt.RadianceJob) == c_layout["sizeof.spt_radiance_job"]
    names = [f[0] for f in spt.RadianceJob._fields_]
    assert names == ["size", "flags", "n_rays", "rays", "aux", "repeats", "max_depth", "seed", "rng_skip", "rays_per_pass", "rgb_out", "hits_out"]
    for name in names:
        assert getattr(spt.RadianceJob, name).offset == c_layout["spt_radiance_job." + name], name


def test_camera_t_min_is_the_reference_epsilon():
    import numpy as np
    assert np.float32(spt.CAMERA_T_MIN) == np.float32(0.0001)
