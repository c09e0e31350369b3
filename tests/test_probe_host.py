"""spt_probe without a device: spt_host_probe_rays (include/spt_probe.h, the header the device kernels include) against
tests/_probe_ref.py, word for word; float64 pins of the basis and of the direction map; sh_irradiance; the structs' layout in C and in
the binding; the stand-alone sanitizer program; the CLI's refusals."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _probe_ref
import _util

spt = _util.load_pkg()
SCENE_NAMES = ["cfg2_cube", "t_materials"]
SAMPLES, SEED = 5, 77


@pytest.fixture(scope="module")
def scenes():
    _util.ensure_cpu_build()
    loaded = {n: spt.load_scene(os.path.join(_util.SCENES, n + ".json")) for n in SCENE_NAMES}
    yield loaded
    for sc in loaded.values():
        sc.close()


def words(a):
    return np.ascontiguousarray(a).view(np.uint8)


def free_points(n, seed):
    return np.random.default_rng(seed).uniform(-4, 4, size=(n, 3)).astype(np.float32)


# ---- host rays

@pytest.mark.parametrize("offsets", [(0, 0), (0xFFFFFFF0, 5)], ids=["first0", "offsets"])
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_host_rays_equal_the_restated_specification(scenes, name, offsets):
    scene = scenes[name]
    p = free_points(40, 5)
    fp, fs = offsets
    got = spt.probe_rays(scene, p, samples=SAMPLES, seed=SEED, first_point=fp, first_sample=fs)
    want = _probe_ref.probe_inputs(spt, scene.array("lights"), p, SAMPLES, SEED, fp, fs)
    assert got["rays"].shape == (40, SAMPLES) and got["weights"].shape == (40, SAMPLES, 9)
    for key in ("weights", "delta_li", "delta_basis"):
        assert np.array_equal(words(got[key]), words(want[key])), key
    for f in ("o", "t_min", "d", "stream_a", "stream_b", "pad"):
        assert np.array_equal(words(got["rays"][f]), words(want["rays"][f])), f
    for f in ("o", "t_min", "d", "t_max"):
        assert np.array_equal(words(got["delta_rays"][f]), words(want["delta_rays"][f])), f
    if fp:   # the stream index wraps at 2^32
        assert got["rays"]["stream_a"][16, 0] == 0 and got["rays"]["stream_a"][15, 0] == 0xFFFFFFFF
        assert got["rays"]["stream_b"][0, 0] == 5
    if name == "t_materials":   # all three delta light types reach the probes, without a cosine: every probe sees the directional one
        types = scene.array("lights")["type"]
        for kind in (0, 1, 2):
            assert np.any(got["delta_li"][:, types == kind] != 0), kind
        assert np.all(np.any(got["delta_li"][:, types == 0] != 0, axis=-1))


def test_records_and_plain_arrays_are_the_same_probes(scenes):
    scene = scenes["cfg2_cube"]
    p = free_points(7, 2)
    rec = np.zeros(7, dtype=spt.PROBE_DTYPE)
    rec["p"], rec["pad"] = p, np.nan      # (pad is not read)
    a, b = spt.probe_rays(scene, p, samples=2), spt.probe_rays(scene, rec, samples=2)
    assert np.array_equal(words(a["rays"]), words(b["rays"]))


def test_a_non_finite_probe_is_refused_by_index(scenes):
    p = free_points(6, 3)
    for bad in (np.nan, np.inf, -np.inf):
        q = p.copy()
        q[4, 2] = bad
        with pytest.raises(spt.SptError) as e:
            spt.probe_rays(scenes["cfg2_cube"], q, samples=1)
        assert e.value.status == 1 and "point 4 " in str(e.value)


def test_sh_basis_is_the_reference_basis():
    d = np.random.default_rng(1).normal(size=(1000, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    assert np.array_equal(words(spt.sh_basis(d)), words(_probe_ref.basis(d)))


# ---- float64 pins

def _basis64(d):
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([np.full_like(x, 0.5 * np.sqrt(1 / np.pi)), np.sqrt(3 / (4 * np.pi)) * y, np.sqrt(3 / (4 * np.pi)) * z, np.sqrt(3 / (4 * np.pi)) * x,
                     0.5 * np.sqrt(15 / np.pi) * x * y, 0.5 * np.sqrt(15 / np.pi) * y * z, 0.25 * np.sqrt(5 / np.pi) * (3 * z * z - 1),
                     0.5 * np.sqrt(15 / np.pi) * x * z, 0.25 * np.sqrt(15 / np.pi) * (x * x - y * y)], axis=-1)


def test_the_basis_is_orthonormal():
    """On a Gauss-Legendre (16 nodes in z) x uniform (32 nodes in phi) grid the integral of Y_i Y_j is delta_ij within 1e-5.  The
    products are polynomials of degree <= 4 in z and trigonometric polynomials of degree <= 4 in phi, which this grid integrates
    exactly, so the grid's own error is float64 rounding (about 1e-15).  The nodes go through the library in f32: a node's direction
    is rounded to f32 (relative 6e-8), each Y takes two or three more f32 roundings and the constants have nine digits, so an entry is
    off by a few 1e-7; 1e-5 leaves two orders of margin."""
    z, wz = np.polynomial.legendre.leggauss(16)
    phi = (np.arange(32) + 0.5) * (2 * np.pi / 32)
    r = np.sqrt(1 - z * z)
    d = np.stack([r[:, None] * np.cos(phi)[None, :], r[:, None] * np.sin(phi)[None, :], np.broadcast_to(z[:, None], (16, 32))], axis=-1)
    w = (wz[:, None] * (2 * np.pi / 32)) * np.ones((16, 32))
    exact = _basis64(d)
    gram64 = np.einsum("ab,abi,abj->ij", w, exact, exact)
    assert np.max(np.abs(gram64 - np.eye(9))) < 1e-12        # the grid's own error
    Y = spt.sh_basis(d.astype(np.float32)).astype(np.float64)
    gram = np.einsum("ab,abi,abj->ij", w, Y, Y)
    assert np.max(np.abs(gram - np.eye(9))) < 1e-5
    assert np.max(np.abs(Y - exact)) < 1e-6                  # the signs and the order of the nine


def test_the_direction_map_is_uniform(scenes):
    """Over N = 10^5 streams every Y_j, j >= 1, of the gather direction has mean 0 and variance 1 / (4 pi) under the uniform
    distribution (orthonormality), so the sample mean has standard deviation sqrt(1 / (4 pi N)) = 0.28 / sqrt(N); 5 / sqrt(N) is 17
    of them.  (A swapped or mirrored axis shows in the test against the reference; this one pins the density.)"""
    N = 100000
    got = spt.probe_rays(scenes["cfg2_cube"], np.zeros((N // 10, 3), dtype=np.float32), samples=10, seed=3)
    Y = got["weights"].reshape(N, 9).astype(np.float64)
    d = got["rays"]["d"].reshape(N, 3).astype(np.float64)
    assert np.max(np.abs(np.linalg.norm(d, axis=1) - 1)) < 1e-6
    mean = Y.mean(axis=0)
    assert np.all(np.abs(mean[1:]) < 5 / np.sqrt(N)), mean
    assert abs(mean[0] - 0.282094792) < 1e-7


# ---- sh_irradiance

def test_sh_irradiance_of_a_constant_radiance_is_pi_l():
    L = np.array([0.5, 2.0, 7.0])
    c = np.zeros((9, 3))
    c[0] = L / 0.282094792        # L = c0 * Y0
    n = np.random.default_rng(4).normal(size=(50, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    E = spt.sh_irradiance(c, n)
    assert E.shape == (50, 3) and E.dtype == np.float64
    assert np.allclose(E, np.pi * L[None, :], rtol=1e-12)


def test_sh_irradiance_of_a_directional_light():
    """Radiance delta(w - w0) * L projects to c_j = L * Y_j(w0).  The order-2 reconstruction of E(n) = L * max(0, cos t) is
    1/4 + cos t / 2 + (5/32) (3 cos^2 t - 1): 17/16 facing the light, 1/16 facing away, and 3/32 at the horizon, its largest error."""
    w0 = np.array([0.0, 0.0, 1.0])
    c = (_basis64(w0)[:, None] * np.ones(3)[None, :])
    th = np.linspace(0, np.pi, 61)
    n = np.stack([np.sin(th), np.zeros_like(th), np.cos(th)], axis=-1)
    E = spt.sh_irradiance(c, n)[:, 0]
    want = 0.25 + np.cos(th) / 2 + (5 / 32) * (3 * np.cos(th) ** 2 - 1)
    assert np.allclose(E, want, atol=1e-8)      # (nine-digit constants)
    assert abs(E[0] - 17 / 16) < 1e-8 and abs(E[30] - 3 / 32) < 1e-8 and abs(E[60] - 1 / 16) < 1e-8
    assert np.max(np.abs(E - np.maximum(0, np.cos(th)))) < 3 / 32 + 1e-6


# ---- layout

@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    cc = shutil.which(os.environ.get("CC", "cc")) or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no C compiler"
    exe = str(tmp_path_factory.mktemp("probe_layout") / "probe_layout_check")
    src = os.path.join(_util.ROOT, "tests", "probe_layout_check.c")
    res = subprocess.run([cc, "-Wall", "-Wextra", "-I", os.path.join(_util.ROOT, "include"), "-o", exe, src], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    return {k: int(v) for k, v in (line.split() for line in out.stdout.splitlines())}


def test_the_binding_declares_the_headers_layout(c_layout):
    assert c_layout["SPT_ABI_VERSION"] == 14
    assert c_layout["sizeof.spt_probe_point"] == spt.PROBE_DTYPE.itemsize == 16
    assert c_layout["sizeof.spt_probe_job"] == C.sizeof(spt.ProbeJob)
    for f in ("p", "pad"):
        assert c_layout["spt_probe_point." + f] == spt.PROBE_DTYPE.fields[f][1]
    for f, _ in spt.ProbeJob._fields_:
        assert c_layout["spt_probe_job." + f] == getattr(spt.ProbeJob, f).offset, f
    assert c_layout["SPT_PROBE_DEVICE_POINTERS"] == spt.PROBE_DEVICE_POINTERS


def test_the_salt_is_a_stream_of_its_own():
    text = open(os.path.join(_util.ROOT, "include", "spt_abi.h")).read()
    assert "#define SPT_PROBE_SEED_SALT 0x%Xull" % _probe_ref.SALT in text
    assert _probe_ref.SALT not in (0x4C454E5343414D31, 0x42414B45504F4E54)   # SPT_CAMERA_SEED_SALT, SPT_BAKE_SEED_SALT


# ---- the CLI's refusals (before any device is touched)

def _cli():
    cli = os.path.join(spt.LIB_DIR, "spt")
    if not os.path.exists(cli):
        subprocess.check_call(["make", "-s", "-C", _util.ROOT, "cli"])
    return cli


def _points_file(tmp_path, text="0 0 0\n1 2 3\n"):
    path = tmp_path / "points.txt"
    path.write_text(text)
    return str(path)


@pytest.mark.parametrize("extra", [
    ["--preview-every", "2"], ["--denoise"], ["--robust", "3"], ["--variance-out", "v.exr"], ["--panorama"], ["--orthographic", "3"],
    ["--animate", "frames.json"], ["--gpus", "2"], ["--devices", "0"], ["--film-devices", "0,0", "--time-limit", "1"],
    ["--bake-lightmap", "cube", "--bake-size", "4x4"], ["--probe-samples", "0"],
], ids=lambda e: e[0])
def test_the_cli_refuses_probes_beside_another_mode(tmp_path, extra):
    out = tmp_path / "probes.txt"
    base = [_cli(), "-s", os.path.join(_util.SCENES, "cfg2_cube.json"), "-r", os.path.join(_util.SCENES, "pt.json"), "-o", str(out)]
    res = subprocess.run(base + ["--bake-probes", _points_file(tmp_path)] + extra, capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and ("--bake-probes" in res.stderr or "--probe-samples" in res.stderr), res.stdout + res.stderr
    assert not out.exists()


@pytest.mark.parametrize("text", ["0 0\n", "0 0 0 0\n", "a b c\n", "0 0 0\n1 2 x\n", "0 0 inf\n", "nan 0 0\n"], ids=["two", "four", "words", "later", "inf", "nan"])
def test_the_cli_refuses_a_malformed_points_file(tmp_path, text):
    out = tmp_path / "probes.txt"
    base = [_cli(), "-s", os.path.join(_util.SCENES, "cfg2_cube.json"), "-r", os.path.join(_util.SCENES, "pt.json"), "-o", str(out)]
    res = subprocess.run(base + ["--bake-probes", _points_file(tmp_path, text)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and "line" in res.stderr, res.stdout + res.stderr
    assert not out.exists()
    res = subprocess.run(base + ["--bake-probes", str(tmp_path / "missing.txt")], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and not out.exists(), res.stdout + res.stderr


# ---- the stand-alone program under AddressSanitizer + UBSan

def test_the_sanitizer_program_runs_clean():
    res = subprocess.run(["make", "-s", "-C", _util.ROOT, "probe-check"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    res = subprocess.run([os.path.join(_util.ROOT, "build", "selftest", "probe_check")], capture_output=True, text=True, timeout=120)
    report = res.stdout + res.stderr
    assert res.returncode == 0, report
    assert "probe_check ok" in res.stdout, report
    for word in ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer", "CHECK failed"):
        assert word not in report, report
