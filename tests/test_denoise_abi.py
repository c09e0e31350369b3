"""The film denoiser (spt_film_denoise, additive to ABI v14) without a GPU: the entry point exists in the header, both libraries and
the binding, null arguments are refused with a message, and the CLI refuses --denoise over several devices before it touches one."""
import ctypes as C
import os
import re
import subprocess

import _util

spt = _util.load_pkg()


def test_header_declares_the_denoiser():
    hdr = open(os.path.join(_util.ROOT, "include", "spt_abi.h")).read()
    assert "#define SPT_ABI_VERSION 14" in hdr          # additive: callers detect the call by symbol
    assert re.search(r"spt_status spt_film_denoise\(spt_film\* film, spt_film\* guide, const spt_denoise_params\* params, float\* out\);", hdr)
    m = re.search(r"typedef struct spt_denoise_params \{(.*?)\} spt_denoise_params;", hdr, re.S)
    assert m
    fields = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split()
    assert " ".join(fields) == "uint32_t size; uint32_t iterations; float k_color, k_guide, eps_color, eps_guide;"
    assert C.sizeof(spt.DenoiseParams) == 24
    assert [n for n, _ in spt.DenoiseParams._fields_] == ["size", "iterations", "k_color", "k_guide", "eps_color", "eps_guide"]


def test_both_libraries_export_the_denoiser():
    for lib in ("libspt_hip.so", "libspt_hip_bez.so"):
        assert hasattr(C.CDLL(os.path.join(spt.LIB_DIR, lib)), "spt_film_denoise"), lib


def test_denoiser_refuses_null_arguments():
    lib = spt.hip_lib()
    out = (C.c_float * 3)(7.0, 7.0, 7.0)
    params = spt.DenoiseParams(C.sizeof(spt.DenoiseParams), 5, 2.0, 1.0, 1e-8, 1e-2)
    for film, buf in ((None, out), (None, None)):
        assert lib.spt_film_denoise(film, None, C.byref(params), buf) == 1
        assert "film_denoise" in lib.spt_last_error().decode() and "null" in lib.spt_last_error().decode()
    assert lib.spt_film_denoise(None, None, None, out) == 1
    assert list(out) == [7.0, 7.0, 7.0]


def test_binding_has_denoise_and_guide_film():
    assert callable(getattr(spt.ProgressiveFilm, "denoise", None))
    assert callable(getattr(spt.PathTracer, "guide_film", None))


def test_cli_refuses_denoise_on_several_devices(tmp_path):
    cli = os.path.join(spt.LIB_DIR, "spt")
    args = ["-s", os.path.join(_util.SCENES, "cfg2_cube.json"), "-r", os.path.join(_util.SCENES, "pt.json"), "-o", str(tmp_path / "o.png")]
    for extra in (["--gpus", "2", "--denoise"], ["--devices", "0,0", "--denoise", "--denoise-iterations", "3"],
                  ["--gpus", "2", "--guide-samples", "8"], ["--devices", "0,0", "--noisy-out", str(tmp_path / "n.png")],
                  ["--gpus", "2", "--denoise", "--adaptive", "0.05"]):
        r = subprocess.run([cli] + args + extra, capture_output=True, text=True)
        assert r.returncode == 2 and "one device" in r.stderr, (extra, r.stderr)
        assert not (tmp_path / "o.png").exists()
        assert not (tmp_path / "n.png").exists()
