"""Progressive rendering (ABI v14) without a GPU: the entry points exist in the header, both libraries and the binding, and
the CLI refuses the progressive flags over several devices before it touches one."""
import ctypes as C
import os
import re
import subprocess

import _util

spt = _util.load_pkg()
FILM_FUNCS = ("spt_film_create", "spt_film_render", "spt_film_samples", "spt_film_read", "spt_film_destroy")


def test_header_declares_the_film_abi():
    hdr = open(os.path.join(_util.ROOT, "include", "spt_abi.h")).read()
    assert spt.SPT_ABI_VERSION == 14 and "#define SPT_ABI_VERSION 14" in hdr
    for name in FILM_FUNCS:
        assert re.search(r"\b%s\(" % name, hdr), name
    assert "SPT_FILM_MOMENTS = 1u" in hdr
    for k, v in (("SPT_FILM_MEAN", 0), ("SPT_FILM_SUM", 1), ("SPT_FILM_SUM_SQ", 2), ("SPT_FILM_VAR_OF_MEAN", 3)):
        assert re.search(r"%s = %d\b" % (k, v), hdr), k
    assert (spt.FILM_MEAN, spt.FILM_SUM, spt.FILM_SUM_SQ, spt.FILM_VAR_OF_MEAN, spt.FILM_MOMENTS) == (0, 1, 2, 3, 1)


def test_both_libraries_export_the_film_calls():
    for lib in ("libspt_hip.so", "libspt_hip_bez.so"):
        h = C.CDLL(os.path.join(spt.LIB_DIR, lib))
        for name in FILM_FUNCS:
            assert hasattr(h, name), (lib, name)


def test_film_calls_refuse_null_arguments():
    lib = spt.hip_lib()
    assert lib.spt_film_render(None, 1) == 1
    assert lib.spt_film_read(None, 0, None) == 1
    assert lib.spt_film_samples(None, None) == 1
    out = C.c_void_p()
    assert lib.spt_film_create(None, None, None, 0, 0, C.byref(out)) == 1
    lib.spt_film_destroy(None)


def test_binding_has_the_progressive_film():
    assert hasattr(spt.PathTracer, "progressive")
    for name in ("render", "samples", "mean", "sum", "sum_sq", "variance_of_mean", "close", "__enter__", "__exit__"):
        assert hasattr(spt.ProgressiveFilm, name), name


def test_cli_refuses_progressive_flags_on_several_devices(tmp_path):
    cli = os.path.join(spt.LIB_DIR, "spt")
    args = ["-s", os.path.join(_util.SCENES, "cfg2_cube.json"), "-r", os.path.join(_util.SCENES, "pt.json"), "-o", str(tmp_path / "o.png")]
    for extra in (["--gpus", "2", "--preview-every", "8"], ["--devices", "0,0", "--time-limit", "1"], ["--gpus", "3", "--variance-out", "v.exr"]):
        r = subprocess.run([cli] + args + extra, capture_output=True, text=True)
        assert r.returncode == 2 and "one device" in r.stderr, (extra, r.stderr)
        assert not (tmp_path / "o.png").exists()
