"""spt_film_denoise_job, SPT_RENDER_AOV_ALBEDO and spt_render_flags_supported (all additive to ABI v14) without a GPU: the header,
both libraries and the binding have them, the struct has one layout in C and in ctypes, null arguments are refused with a message,
and the CLI refuses the new options where they make no sense before it touches a device."""
import ctypes as C
import os
import re
import subprocess

import _util

spt = _util.load_pkg()
HDR = open(os.path.join(_util.ROOT, "include", "spt_abi.h")).read()
JOB_FIELDS = ["size", "flags", "guide", "albedo", "params", "k_albedo", "eps_albedo", "eps_demod", "pad"]


def test_header_declares_the_new_calls_and_keeps_the_old_ones():
    assert "#define SPT_ABI_VERSION 14" in HDR and spt.SPT_ABI_VERSION == 14      # additive: detected by symbol
    assert re.search(r"SPT_RENDER_AOV_ALBEDO = 32u", HDR) and spt.RENDER_AOV_ALBEDO == 32
    assert re.search(r"spt_status spt_render_flags_supported\(uint32_t\* mask\);", HDR)
    assert re.search(r"enum \{ SPT_DENOISE_DEMODULATE = 1u, SPT_DENOISE_OUT_RGB8 = 2u \};", HDR)
    assert (spt.DENOISE_DEMODULATE, spt.DENOISE_OUT_RGB8) == (1, 2)
    assert re.search(r"spt_status spt_film_denoise_job\(spt_film\* film, const spt_denoise_job\* job, void\* out\);", HDR)
    assert re.search(r"spt_status spt_film_denoise\(spt_film\* film, spt_film\* guide, const spt_denoise_params\* params, float\* out\);", HDR)
    assert C.sizeof(spt.DenoiseParams) == 24
    # the albedo rule is spelled out where the flag is declared
    rule = HDR[HDR.index("SPT_RENDER_AOV_ALBEDO = 32u"):HDR.index("spt_status spt_render_flags_supported")]
    for word in ("SPT_BXDF_LAMBERT", "PNDF_PLASTIC", "SPT_FRESNEL_SCHLICK", "(1, 1, 1)", "SPT_RENDER_DEBUG_NORMAL", "SPT_ERR_INVALID_ARG"):
        assert word in rule, word


def test_job_struct_has_one_layout_in_c_and_ctypes(tmp_path):
    assert [n for n, _ in spt.DenoiseJob._fields_] == JOB_FIELDS
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "spt_abi.h"\nint main() {\n'
                   '    std::printf("%zu %zu", sizeof(spt_denoise_job), sizeof(spt_denoise_params));\n' +
                   "".join('    std::printf(" %%zu", offsetof(spt_denoise_job, %s));\n' % f for f in JOB_FIELDS) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-I", os.path.join(_util.ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(spt.DenoiseJob) == 48 and got[1] == C.sizeof(spt.DenoiseParams) == 24
    assert got[2:] == [getattr(spt.DenoiseJob, f).offset for f in JOB_FIELDS]


def test_both_libraries_export_the_new_calls():
    for lib in ("libspt_hip.so", "libspt_hip_bez.so"):
        h = C.CDLL(os.path.join(spt.LIB_DIR, lib))
        for sym in ("spt_film_denoise_job", "spt_render_flags_supported"):
            assert hasattr(h, sym), (lib, sym)
        mask = C.c_uint32()
        assert h.spt_render_flags_supported(C.byref(mask)) == 0        # needs no device
        assert mask.value & 16 and mask.value & 32 and mask.value == 63
        assert h.spt_render_flags_supported(None) == 1
    assert spt.render_flags_supported() == 63


def test_denoise_job_refuses_null_arguments():
    lib = spt.hip_lib()
    out = (C.c_float * 3)(7.0, 7.0, 7.0)
    job = spt.DenoiseJob(C.sizeof(spt.DenoiseJob), 0, None, None, None, 1.0, 1e-2, 1e-2, 0)
    for film, j, buf in ((None, C.byref(job), out), (None, None, out), (None, C.byref(job), None)):
        assert lib.spt_film_denoise_job(film, j, buf) == 1
        assert "film_denoise_job" in lib.spt_last_error().decode() and "null" in lib.spt_last_error().decode()
    assert list(out) == [7.0, 7.0, 7.0]


def test_binding_has_the_albedo_calls():
    assert callable(getattr(spt.ProgressiveFilm, "denoise_job", None))
    assert callable(getattr(spt.PathTracer, "albedo_film", None))
    assert callable(spt.render_flags_supported)


def test_cli_refuses_the_new_options_before_it_touches_a_device(tmp_path):
    cli = os.path.join(spt.LIB_DIR, "spt")
    args = ["-s", os.path.join(_util.SCENES, "cfg2_cube.json"), "-r", os.path.join(_util.SCENES, "pt.json"), "-o", str(tmp_path / "o.png")]
    a_out = str(tmp_path / "a.png")
    for extra, word in ((["--denoise", "--demodulate"], "--guide albedo"), (["--denoise", "--guide", "normal", "--demodulate"], "--guide albedo"),
                        (["--denoise", "--albedo-out", a_out], "--guide albedo"), (["--denoise", "--guide", "depth"], "normal, albedo or both"),
                        (["--gpus", "2", "--guide", "both"], "one device"), (["--devices", "0,0", "--guide", "albedo", "--demodulate"], "one device"),
                        (["--robust", "5", "--guide", "both"], "exclude each other")):
        r = subprocess.run([cli] + args + extra, capture_output=True, text=True)
        assert r.returncode == 2 and word in r.stderr, (extra, r.stderr)
        assert not (tmp_path / "o.png").exists() and not (tmp_path / "a.png").exists()
