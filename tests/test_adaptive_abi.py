"""Adaptive sampling of a film (spt_film_adapt / spt_film_read_counts, additive to ABI v14) without a GPU: the entry points
exist in the header, both libraries and the binding, null arguments are refused, and the CLI refuses the adaptive flags over
several devices before it touches one."""
import ctypes as C
import os
import re
import subprocess

import _util

spt = _util.load_pkg()
ADAPT_FUNCS = ("spt_film_adapt", "spt_film_read_counts")


def test_header_declares_the_adaptive_calls():
    hdr = open(os.path.join(_util.ROOT, "include", "spt_abi.h")).read()
    assert "#define SPT_ABI_VERSION 14" in hdr          # additive: callers detect the calls by symbol
    assert re.search(r"spt_status spt_film_adapt\(spt_film\* film, float rel_error, float abs_floor, uint32_t min_samples, uint32_t\* active_out\);", hdr)
    assert re.search(r"spt_status spt_film_read_counts\(spt_film\* film, uint32_t\* out\);", hdr)


def test_both_libraries_export_the_adaptive_calls():
    for lib in ("libspt_hip.so", "libspt_hip_bez.so"):
        h = C.CDLL(os.path.join(spt.LIB_DIR, lib))
        for name in ADAPT_FUNCS:
            assert hasattr(h, name), (lib, name)


def test_adaptive_calls_refuse_null_arguments():
    lib = spt.hip_lib()
    active = C.c_uint32(7)
    assert lib.spt_film_adapt(None, 0.1, 0.0, 16, C.byref(active)) == 1
    assert active.value == 7
    assert lib.spt_film_adapt(None, 0.1, 0.0, 16, None) == 1
    assert lib.spt_film_read_counts(None, None) == 1
    assert "null" in lib.spt_last_error().decode()


def test_binding_has_adapt_and_sample_counts():
    for name in ("adapt", "sample_counts"):
        assert callable(getattr(spt.ProgressiveFilm, name, None)), name


def test_cli_refuses_adaptive_flags_on_several_devices(tmp_path):
    cli = os.path.join(spt.LIB_DIR, "spt")
    args = ["-s", os.path.join(_util.SCENES, "cfg2_cube.json"), "-r", os.path.join(_util.SCENES, "pt.json"), "-o", str(tmp_path / "o.png")]
    for extra in (["--gpus", "2", "--adaptive", "0.05"], ["--devices", "0,0", "--adaptive", "0.1", "--adaptive-floor", "0.01"],
                  ["--gpus", "2", "--samples-out", str(tmp_path / "n.exr")]):
        r = subprocess.run([cli] + args + extra, capture_output=True, text=True)
        assert r.returncode == 2 and "one device" in r.stderr, (extra, r.stderr)
        assert not (tmp_path / "o.png").exists()
        assert not (tmp_path / "n.exr").exists()
