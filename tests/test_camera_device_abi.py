"""spt_camera_rays and spt_camera_gbuffer without a device: the layout of their job structs (include/spt_abi.h as a C compiler sees it,
against the binding's ctypes declarations), the exported symbols, the signatures of the Python methods and the checks that come before
any device call."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import pytest

import _util

spt = _util.load_pkg()


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    cc = shutil.which(os.environ.get("CC", "cc")) or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no C compiler"
    exe = str(tmp_path_factory.mktemp("camera_device_layout") / "camera_device_layout_check")
    src = os.path.join(_util.ROOT, "tests", "camera_device_layout_check.c")
    res = subprocess.run([cc, "-Wall", "-Wextra", "-I", os.path.join(_util.ROOT, "include"), "-o", exe, src], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    return {k: int(v) for k, v in (line.split() for line in out.stdout.splitlines())}


RAYS_JOB = {"size": 0, "flags": 4, "model": 8, "plan": 16, "first": 24, "count": 28, "rays": 32, "aux": 40, "rays_per_pass": 48, "pad": 52}
GBUFFER_JOB = {"size": 0, "flags": 4, "model": 8, "plan": 16, "first": 24, "count": 28, "albedo": 32, "normal": 40, "depth": 48, "coverage": 56,
               "rays_per_pass": 64, "pad": 68}


@pytest.mark.parametrize("c_name,cls,want,size", [("spt_camera_rays_job", "CameraRaysJob", RAYS_JOB, 56),
                                                  ("spt_camera_gbuffer_job", "CameraGBufferJob", GBUFFER_JOB, 72)])
def test_the_binding_declares_the_headers_layout(c_layout, c_name, cls, want, size):
    mirror = getattr(spt, cls)
    assert c_layout["SPT_ABI_VERSION"] == spt.SPT_ABI_VERSION == 14
    assert c_layout["sizeof." + c_name] == C.sizeof(mirror) == size
    assert [f for f, _ in mirror._fields_] == list(want)
    for f, off in want.items():
        assert c_layout["%s.%s" % (c_name, f)] == getattr(mirror, f).offset == off, f


def test_the_flags_and_the_records(c_layout):
    assert c_layout["SPT_CAMERA_RAYS_DEVICE_POINTERS"] == spt.CAMERA_RAYS_DEVICE_POINTERS == 1
    assert c_layout["SPT_CAMERA_GBUFFER_DEVICE_POINTERS"] == spt.CAMERA_GBUFFER_DEVICE_POINTERS == 1
    assert (c_layout["sizeof.spt_path_ray"], c_layout["sizeof.spt_ray_aux"]) == (spt.PATH_RAY_DTYPE.itemsize, spt.RAY_AUX_DTYPE.itemsize) == (48, 64)
    assert c_layout["sizeof.spt_camera_model"] == C.sizeof(spt.CameraModel)


def test_both_libraries_export_the_calls():
    lib = spt.hip_lib()
    bez = C.CDLL(os.path.join(spt.LIB_DIR, "libspt_hip_bez.so"))
    for name in ("spt_camera_rays", "spt_camera_gbuffer"):
        assert hasattr(lib, name) and hasattr(bez, name), name
    # the refusals that need no scene
    assert lib.spt_camera_rays(None, C.byref(spt.CameraRaysJob(size=C.sizeof(spt.CameraRaysJob)))) == 1      # SPT_ERR_INVALID_ARG
    assert b"camera_rays" in lib.spt_last_error()
    assert lib.spt_camera_gbuffer(None, C.byref(spt.CameraGBufferJob(size=C.sizeof(spt.CameraGBufferJob)))) == 1
    assert b"camera_gbuffer" in lib.spt_last_error()


def _parameters(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_the_methods_signatures():
    none = inspect.Parameter.empty
    assert _parameters(spt.DeviceScene.camera_rays)[:9] == [("self", none), ("model", none), ("renderer", none), ("width", none), ("height", none),
                                                            ("first", 0), ("count", None), ("aux", False), ("on_device", False)]
    assert _parameters(spt.DeviceScene.camera_gbuffer)[:8] == [("self", none), ("model", none), ("renderer", none), ("width", none), ("height", none),
                                                               ("samples", 1), ("first", 0), ("on_device", False)]
    # the module-level call keeps the arguments it had
    assert _parameters(spt.camera_gbuffer)[:7] == [("scene", none), ("model", none), ("renderer", none), ("width", none), ("height", none),
                                                   ("samples", 1), ("device", 0)]


class _NoDevice:
    """Stands where a DeviceScene's handle would: any use of it is a device call."""
    def __getattr__(self, name):
        raise AssertionError("the device scene was touched (%s)" % name)


@pytest.mark.parametrize("samples", [0, -1])
def test_samples_below_one_raise_before_any_device_call(samples):
    with pytest.raises(ValueError):
        spt.DeviceScene.camera_gbuffer(_NoDevice(), None, None, 4, 4, samples=samples)
    with pytest.raises(ValueError):
        spt.camera_gbuffer(None, None, None, 4, 4, samples=samples)


def test_the_cli_names_the_fallback_route():
    cli = os.path.join(spt.LIB_DIR, "spt")
    if not os.path.exists(cli):
        subprocess.check_call(["make", "-s", "-C", _util.ROOT, "cli"])
    res = subprocess.run([cli], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and "--gbuffer-host-rays" in res.stderr
    base = [cli, "-s", os.path.join(_util.SCENES, "cfg2_cube.json"), "-r", os.path.join(_util.SCENES, "pt.json"), "-o", "unused.png"]
    res = subprocess.run(base + ["--gbuffer-host-rays"], capture_output=True, text=True, timeout=60)      # no stem: refused before any device
    assert res.returncode == 2 and "--gbuffer-out" in res.stderr, res.stdout + res.stderr
