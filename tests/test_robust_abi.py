"""Bucketed films (spt_film_buckets, spt_film_read_buckets, spt_film_read_robust; additive to ABI v14) without a GPU: the entry
points exist in the header, both libraries and the binding, null arguments are refused with a message, and the CLI refuses the
combinations --robust does not serve before it touches a device."""
import ctypes as C
import os
import re
import subprocess

import pytest

import _util

spt = _util.load_pkg()


def test_header_declares_the_bucket_calls():
    hdr = open(os.path.join(_util.ROOT, "include", "spt_abi.h")).read()
    assert "#define SPT_ABI_VERSION 14" in hdr          # additive: callers detect the calls by symbol
    assert spt.SPT_ABI_VERSION == 14
    assert "spt_status spt_film_buckets(spt_film* film, uint32_t n_buckets);" in hdr
    assert "spt_status spt_film_read_buckets(spt_film* film, float* out);" in hdr
    assert "spt_status spt_film_read_robust(spt_film* film, uint32_t estimator, float* out);" in hdr
    assert re.search(r"enum \{ SPT_ROBUST_MON = 0, SPT_ROBUST_GMON = 1 \};", hdr)
    assert (spt.ROBUST_MON, spt.ROBUST_GMON) == (0, 1)


def test_both_libraries_export_the_bucket_calls():
    for lib in ("libspt_hip.so", "libspt_hip_bez.so"):
        handle = C.CDLL(os.path.join(spt.LIB_DIR, lib))
        for name in ("spt_film_buckets", "spt_film_read_buckets", "spt_film_read_robust"):
            assert hasattr(handle, name), (lib, name)


def test_binding_has_the_methods():
    for name in ("bucket_sums", "robust_mean", "set_buckets"):
        assert callable(getattr(spt.ProgressiveFilm, name, None)), name
    import inspect
    for fn in (spt.PathTracer.progressive, spt.ProgressiveFilm.__init__):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "buckets" and params[-1].default == 0     # new keyword, last
    assert inspect.signature(spt.ProgressiveFilm.robust_mean).parameters["estimator"].default == "gmon"


def test_null_arguments_are_refused():
    lib = spt.hip_lib()
    out = (C.c_float * 3)(7.0, 7.0, 7.0)
    fake = C.c_void_p(0)
    assert lib.spt_film_buckets(None, 5) == 1
    assert "film_buckets" in lib.spt_last_error().decode() and "null" in lib.spt_last_error().decode()
    assert lib.spt_film_read_buckets(None, out) == 1
    assert "film_read_buckets" in lib.spt_last_error().decode() and "null" in lib.spt_last_error().decode()
    assert lib.spt_film_read_buckets(fake, None) == 1
    for estimator in (spt.ROBUST_MON, spt.ROBUST_GMON, 2):
        assert lib.spt_film_read_robust(None, estimator, out) == 1
        assert "film_read_robust" in lib.spt_last_error().decode() and "null" in lib.spt_last_error().decode()
    assert lib.spt_film_read_robust(fake, spt.ROBUST_GMON, None) == 1
    assert list(out) == [7.0, 7.0, 7.0]


@pytest.mark.parametrize("extra,words", [
    (["--robust", "9", "--gpus", "2"], "one device"),
    (["--robust", "9", "--devices", "0,0"], "one device"),
    (["--robust", "4"], "odd"),
    (["--robust", "17"], "3 .. 15"),
    (["--robust-estimator", "mon"], "--robust"),
    (["--mean-out", "MEAN"], "--robust"),
    (["--robust", "9", "--denoise"], "exclude each other"),
], ids=["gpus_2", "devices_0_0", "even", "too_many", "estimator_alone", "mean_out_alone", "with_denoise"])
def test_cli_refuses(tmp_path, extra, words):
    cli = os.path.join(spt.LIB_DIR, "spt")
    mean = tmp_path / "mean.png"
    extra = [str(mean) if a == "MEAN" else a for a in extra]
    args = ["-s", os.path.join(_util.SCENES, "cfg2_cube.json"), "-r", os.path.join(_util.SCENES, "pt.json"), "-o", str(tmp_path / "o.png")]
    r = subprocess.run([cli] + args + extra, capture_output=True, text=True)
    assert r.returncode == 2 and words in r.stderr, (extra, r.stderr)
    assert not (tmp_path / "o.png").exists() and not mean.exists()
