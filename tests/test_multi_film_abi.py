"""spt_denoise_image and the multi film (spt_host_multi_film_*), all additive to ABI v14, without a GPU: the headers, the three
libraries and the binding have them, the structs have one layout in C and in ctypes, null arguments are refused with a message,
and the CLI refuses the new option where it makes no sense before it touches a device."""
import ctypes as C
import os
import re
import subprocess

import _util

spt = _util.load_pkg()
ABI = open(os.path.join(_util.ROOT, "include", "spt_abi.h")).read()
HOST = open(os.path.join(_util.ROOT, "include", "spt_host.h")).read()
MULTI_FILM_CALLS = ["create", "render", "samples", "read", "read_counts", "read_robust", "read_rgb8", "adapt", "denoise", "destroy"]
IMAGE_JOB_FIELDS = ["size", "flags", "width", "rows", "mean", "var", "guide_mean", "guide_var", "albedo_mean", "albedo_var", "params",
                    "k_albedo", "eps_albedo", "eps_demod", "pad"]
MULTI_JOB_FIELDS = ["size", "flags", "guide", "albedo", "params", "k_albedo", "eps_albedo", "eps_demod", "pad"]
FILM_API_FIELDS = ["size", "pad", "film_create", "film_destroy", "film_render", "film_samples", "film_read", "film_read_counts", "film_adapt",
                   "film_buckets", "film_read_robust", "film_read_rgb8", "denoise_image", "last_error"]


def test_headers_declare_the_new_calls_and_the_version_stays():
    assert "#define SPT_ABI_VERSION 14" in ABI and spt.SPT_ABI_VERSION == 14      # additive: detected by symbol
    assert re.search(r"spt_status spt_denoise_image\(const spt_scene\* scene, const spt_image_denoise_job\* job, void\* out\);", ABI)
    assert re.search(r"\} spt_image_denoise_job;", ABI) and re.search(r"\} spt_device_film_api;", HOST)
    assert re.search(r"\} spt_host_multi_film_denoise_job;", HOST)
    for call in MULTI_FILM_CALLS:
        assert re.search(r"\bspt_host_multi_film_%s\(" % call, HOST), call
    # the old calls are still declared as they were
    assert re.search(r"spt_status spt_film_denoise_job\(spt_film\* film, const spt_denoise_job\* job, void\* out\);", ABI)
    assert re.search(r"spt_status spt_host_multi_render\(spt_host_multi\* m, const spt_camera\* cam, const spt_render_params\* params, uint32_t strip_rows,", HOST)


def test_libraries_export_the_new_calls():
    for lib in ("libspt_hip.so", "libspt_hip_bez.so"):
        assert hasattr(C.CDLL(os.path.join(spt.LIB_DIR, lib)), "spt_denoise_image"), lib
    host = C.CDLL(os.path.join(spt.LIB_DIR, "libspt_host.so"))
    for call in MULTI_FILM_CALLS:
        assert hasattr(host, "spt_host_multi_film_" + call), call


def test_structs_have_one_layout_in_c_and_ctypes(tmp_path):
    structs = (("spt_image_denoise_job", spt.ImageDenoiseJob, IMAGE_JOB_FIELDS), ("spt_host_multi_film_denoise_job", spt.MultiFilmDenoiseJob, MULTI_JOB_FIELDS),
               ("spt_device_film_api", spt.DeviceFilmApi, FILM_API_FIELDS))
    body = ""
    for name, cls, fields in structs:
        assert [n for n, _ in cls._fields_] == fields
        body += '    std::printf(" %%zu", sizeof(%s));\n' % name
        body += "".join('    std::printf(" %%zu", offsetof(%s, %s));\n' % (name, f) for f in fields)
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "spt_host.h"\nint main() {\n' + body + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-I", os.path.join(_util.ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    for name, cls, fields in structs:
        assert got[0] == C.sizeof(cls), name
        assert got[1:1 + len(fields)] == [getattr(cls, f).offset for f in fields], name
        got = got[1 + len(fields):]
    assert got == []
    assert C.sizeof(spt.ImageDenoiseJob) == 88 and C.sizeof(spt.MultiFilmDenoiseJob) == 48 and C.sizeof(spt.DeviceFilmApi) == 8 + 12 * 8


def test_denoise_image_refuses_null_arguments():
    lib = spt.hip_lib()
    out = (C.c_float * 3)(7.0, 7.0, 7.0)
    img = (C.c_float * 3)(1.0, 1.0, 1.0)
    job = spt.ImageDenoiseJob(C.sizeof(spt.ImageDenoiseJob), 0, 1, 1, C.addressof(img), C.addressof(img), None, None, None, None, None, 1.0, 1e-2, 1e-2, 0)
    for scene, j, buf in ((None, C.byref(job), out), (None, None, out), (None, C.byref(job), None)):
        assert lib.spt_denoise_image(scene, j, buf) == 1
        assert "denoise_image" in lib.spt_last_error().decode() and "null" in lib.spt_last_error().decode()
    assert list(out) == [7.0, 7.0, 7.0]


def test_multi_film_calls_refuse_null_arguments():
    lib = spt.host_lib()
    out = C.c_void_p(0x1234)
    cam, p = spt.Camera(), spt.RenderParams()
    api = spt.DeviceFilmApi(C.sizeof(spt.DeviceFilmApi))
    assert lib.spt_host_multi_film_create(None, C.byref(api), C.byref(cam), C.byref(p), 0, 0, 0, 0, C.byref(out)) == 1
    assert b"multi_film_create" in lib.spt_host_last_error() and b"null" in lib.spt_host_last_error()
    assert out.value == 0x1234
    buf = (C.c_float * 3)(7.0, 7.0, 7.0)
    done = C.c_uint32(77)
    job = spt.MultiFilmDenoiseJob(C.sizeof(spt.MultiFilmDenoiseJob))
    calls = (("render", (None, 1)), ("samples", (None, C.byref(done))), ("read", (None, 0, buf)), ("read_counts", (None, buf)),
             ("read_robust", (None, 0, buf)), ("read_rgb8", (None, 0, buf)), ("adapt", (None, 0.1, 0.0, 2, C.byref(done))),
             ("denoise", (None, C.byref(job), buf)))
    for name, args in calls:
        assert getattr(lib, "spt_host_multi_film_" + name)(*args) == 1, name
        msg = lib.spt_host_last_error().decode()
        assert "multi_film_" + name in msg and "null" in msg, (name, msg)
    assert list(buf) == [7.0, 7.0, 7.0] and done.value == 77
    lib.spt_host_multi_film_destroy(None)     # like free(NULL)


def test_binding_has_the_new_methods():
    assert callable(spt.denoise_image) and callable(spt.hip_device_film_api)
    assert callable(getattr(spt.MultiDevice, "progressive", None))
    for name in ("render", "read", "mean", "sum", "sum_sq", "variance_of_mean", "sample_counts", "adapt", "robust_mean", "read_rgb8",
                 "denoise_job", "close", "__enter__", "__exit__"):
        assert callable(getattr(spt.MultiFilm, name, None)), name
    assert isinstance(spt.MultiFilm.samples, property)


def test_cli_refuses_the_new_option_before_it_touches_a_device(tmp_path):
    cli = os.path.join(spt.LIB_DIR, "spt")
    args = ["-s", os.path.join(_util.SCENES, "cfg2_cube.json"), "-r", os.path.join(_util.SCENES, "pt.json"), "-o", str(tmp_path / "o.png")]
    cases = ((["--film-devices", "", "--preview-every", "4"], "list of device indices"), (["--film-devices", "0,,1", "--preview-every", "4"], "list of device indices"),
             (["--film-devices", "0,x", "--denoise"], "list of device indices"), (["--film-devices", "0,", "--denoise"], "list of device indices"),
             (["--film-devices", "-1", "--denoise"], "list of device indices"),
             (["--film-devices", "0,0", "--gpus", "2", "--preview-every", "4"], "exclude each other"),
             (["--film-devices", "0,0", "--devices", "0", "--denoise"], "exclude each other"),
             (["--film-devices", "0,0"], "progressive option"), (["--film-devices", "0", "--spp", "4"], "progressive option"),
             # the refusals from before stay as they are
             (["--gpus", "2", "--preview-every", "4"], "one device"), (["--robust", "5", "--denoise"], "exclude each other"),
             (["--film-devices", "0,0", "--robust", "5", "--denoise"], "exclude each other"))
    for extra, word in cases:
        r = subprocess.run([cli] + args + extra, capture_output=True, text=True)
        assert r.returncode == 2 and word in r.stderr, (extra, r.returncode, r.stderr)
        assert list(tmp_path.iterdir()) == []
