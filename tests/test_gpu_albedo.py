"""First-hit albedo films (SPT_RENDER_AOV_ALBEDO) and the denoiser that takes one (spt_film_denoise_job) on the device.

The albedo film is compared word for word with the emissive stand-in (tests/_albedo_ref.py: the CPU oracle on a derived descriptor
whose surfaces emit their albedo), the filter with its float32 restatement (tests/_denoise_job_ref.py) on what the films themselves
read out.  Images are 50 x 37: partial 16 x 16 tiles in both directions, and the step-16 taps of the fifth iteration leave the image.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _albedo_ref as A
import _denoise_job_ref as J
import _util

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 4
W, H, SPP = 50, 37, 8
SCENES = [
    ("cfg2_cube.json", None),         # the fused pipeline (kSimple)
    ("t_materials.json", "main"),     # every constant BxDF kind, and an environment that must not show
    ("t_textured.json", None),        # recipes: textures per hit
    ("t_plastic.json", None),
    ("t_pndf.json", "main"),          # glints: P-NDF lobes and their fallbacks
    ("t_subsurface.json", None),      # the shade kernels that trace a probe ray
    ("t_medium.json", None),
    ("t_bezier.json", "main"),        # libspt_hip_bez.so
]


@pytest.fixture(scope="module")
def spt():
    pkg = _util.load_pkg()
    _util.ensure_cpu_build()
    return pkg


def _scene(spt, name):
    return spt.load_scene(os.path.join(_util.SCENES, name))


def _tracer(spt, spp=SPP, seed=5, sampler=None, **kw):
    return spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RANDOM if sampler is None else sampler, spp=spp, seed=seed, **kw)


def _words(a, b):
    assert _util.same_words(a, b), int((a.view(np.uint32) != b.view(np.uint32)).sum())


def _check_film(film, s, q, n):
    """S, Q, MEAN and VAR_OF_MEAN of an albedo film that covers n samples against the stand-in's sums."""
    m, v = _util.film_mean_and_variance(s, q, n)
    _words(film.sum(), s)
    _words(film.sum_sq(), q)
    _words(film.mean(), m)
    _words(film.variance_of_mean(), v)
    return m


# ---- 1. the albedo film is the stand-in's --------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene_name,camera", SCENES, ids=[s[0][:-5] for s in SCENES])
def test_albedo_film_equals_stand_in(spt, scene_name, camera):
    sc = _scene(spt, scene_name)
    r = _tracer(spt)
    cfg = spt.OutputConfig(W, H, None, camera)
    s, q = A.albedo_sums(sc, r, W, H, 0, SPP, camera=camera, flags=_util.device_oracle_flags())
    assert (s != 0).any() and (s.reshape(-1, 3) == 0).all(axis=-1).any()          # something is hit, something is missed
    with r.albedo_film(sc, cfg) as film:
        film.render(SPP)
        m = _check_film(film, s, q, SPP)
    _words(_tracer(spt, aov_albedo=True).render_shard(sc, cfg), m)               # spt_render with the flag: the film's mean
    beauty = r.render_shard(sc, cfg)
    assert not _util.same_words(beauty, m)
    sc.close()


@pytest.fixture(scope="module")
def materials(spt):
    sc = _scene(spt, "t_materials.json")
    yield sc
    sc.close()


def test_samplers(spt, materials):
    cfg = spt.OutputConfig(W, H, None, "main")
    for kw in (dict(sampler=spt.SAMPLER_RECURRENCE), dict(sampler=spt.SAMPLER_JITTERED, division_x=4, division_y=2)):   # (random: above)
        r = _tracer(spt, **kw)
        s, q = A.albedo_sums(materials, r, W, H, 0, SPP, camera="main", flags=_util.device_oracle_flags())
        with r.albedo_film(materials, cfg) as film:
            _check_film(film.render(SPP), s, q, SPP)


def test_increments_first_sample_and_shards(spt, materials):
    r = _tracer(spt)
    cfg = spt.OutputConfig(W, H, None, "main")
    flags = _util.device_oracle_flags()
    s, q = A.albedo_sums(materials, r, W, H, 0, SPP, camera="main", flags=flags)
    with r.albedo_film(materials, cfg) as film:
        s3, q3 = A.albedo_sums(materials, r, W, H, 0, 3, camera="main", flags=flags)
        _check_film(film.render(3), s3, q3, 3)
        _check_film(film.render(5), s, q, SPP)                                  # 3 + 5: the bits of 8 at once
    with r.progressive(materials, cfg, first_sample=5, moments=True, flags=spt.RENDER_AOV_ALBEDO) as late:
        s5, q5 = A.albedo_sums(materials, r, W, H, 5, 3, camera="main", flags=flags)
        _check_film(late.render(3), s5, q5, 3)
    layout = dict(shard_index=1, shard_count=2, strip_rows=8)
    with r.progressive(materials, cfg, moments=True, flags=spt.RENDER_AOV_ALBEDO, **layout) as shard:
        ss, qs = A.albedo_sums(materials, r, W, H, 0, SPP, camera="main", flags=flags, **layout)
        assert ss.shape == (16, W, 3)                                           # rows 8 .. 15 and 24 .. 31
        _check_film(shard.render(SPP), ss, qs, SPP)


CHILD = """
import os, sys
import numpy as np
import _util
spt = _util.load_pkg()
sc = spt.load_scene(os.path.join(_util.SCENES, "t_materials.json"))
r = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RANDOM, spp=%d, seed=5)
with r.albedo_film(sc, spt.OutputConfig(%d, %d, None, "main")) as film:
    film.render(%d)
    np.savez(sys.argv[1], s=film.sum(), q=film.sum_sq())
sc.close()
"""


def test_reference_bvh_in_a_child_process(spt, materials, tmp_path):
    """SPT_REFERENCE_BVH=1 (read when the device scene is made): the caller's trees, the oracle's tree-walking configuration."""
    out = tmp_path / "film.npz"
    env = dict(os.environ, SPT_REFERENCE_BVH="1")
    res = subprocess.run([sys.executable, "-c", CHILD % (SPP, W, H, SPP), str(out)], cwd=os.path.dirname(os.path.abspath(__file__)), env=env,
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    got = np.load(out)
    s, q = A.albedo_sums(materials, _tracer(spt), W, H, 0, SPP, camera="main", flags=_util.ORACLE_DEVICE)
    _words(got["s"], s)
    _words(got["q"], q)


# ---- 2. the denoiser with an albedo film is its restatement ----------------------------------------------------------------------

def _read(film):
    return (None, None) if film is None else (film.mean(), film.variance_of_mean())


def _check_job(film, guide, albedo, demodulate=False, **params):
    got = film.denoise_job(guide, albedo, demodulate=demodulate, **params)
    want = J.denoise_job(*_read(film), *_read(guide), *_read(albedo), demodulate=demodulate, **params)
    assert _util.same_words(got, want), (guide is not None, albedo is not None, demodulate, params,
                                         int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    return got


def _state(film):
    return film.sum(), film.sum_sq(), film.samples, film.sample_counts()


def _same_state(a, b):
    return _util.same_words(a[0], b[0]) and _util.same_words(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3])


NON_DEFAULT = dict(iterations=4, k_color=0.75, k_guide=2.5, eps_color=3e-6, eps_guide=0.2, k_albedo=0.5, eps_albedo=3e-3, eps_demod=0.05)


@pytest.mark.parametrize("scene_name,camera", [("t_textured.json", None), ("t_materials.json", "main")], ids=["t_textured", "t_materials"])
def test_denoise_job_equals_restatement(spt, scene_name, camera):
    sc = _scene(spt, scene_name)
    r = _tracer(spt, spp=32)
    cfg = spt.OutputConfig(W, H, None, camera)
    with r.progressive(sc, cfg, moments=True) as film, r.guide_film(sc, cfg) as guide, r.albedo_film(sc, cfg) as albedo, \
            r.progressive(sc, cfg, moments=True) as alone, r.albedo_film(sc, cfg) as albedo_alone:
        for f in (film, guide, albedo, alone, albedo_alone):
            f.render(16)
        before = _state(film), _state(guide), _state(albedo)
        results = []
        for k in (1, 5):
            results += [_check_job(film, None, albedo, iterations=k), _check_job(film, guide, albedo, iterations=k),
                        _check_job(film, guide, albedo, demodulate=True, iterations=k), _check_job(film, None, albedo, demodulate=True, iterations=k)]
        for a in range(len(results)):
            for b in range(a):
                assert not _util.same_words(results[a], results[b]), (a, b)
        assert not _util.same_words(results[5], film.denoise(guide))            # the albedo term does something
        _check_job(film, guide, albedo, demodulate=True, **NON_DEFAULT)
        _check_job(film, guide, albedo, **NON_DEFAULT)
        assert _util.same_words(film.denoise_job(guide, albedo), film.denoise_job(guide, albedo, **J.DEFAULTS))
        # the 8-bit output is the host's conversion of the float result
        for kw in (dict(), dict(demodulate=True)):
            got8 = film.denoise_job(guide, albedo, rgb8=True, **kw)
            assert got8.dtype == np.uint8 and np.array_equal(got8, spt.film_to_rgb8(film.denoise_job(guide, albedo, **kw)))
        # the three films are read only: they are what they were, and go on to the bits of undisturbed films
        assert all(_same_state(_state(f), b) for f, b in zip((film, guide, albedo), before))
        for f in (film, albedo, alone, albedo_alone):
            f.render(8)
        assert _same_state(_state(film), _state(alone)) and _same_state(_state(albedo), _state(albedo_alone))
        _check_job(film, guide, albedo, demodulate=True)                        # the films need not cover the same samples
    sc.close()


def test_denoise_job_on_an_adaptive_film(spt, materials):
    """The colour film's input is each pixel's mean and variance at its own sample count, as in spt_film_denoise."""
    r = _tracer(spt, spp=32)
    cfg = spt.OutputConfig(W, H, None, "main")
    with r.progressive(materials, cfg, moments=True) as film, r.guide_film(materials, cfg) as guide, r.albedo_film(materials, cfg) as albedo:
        for _ in range(4):
            film.render(4)
            m, sd = film.mean().astype(np.float64), np.sqrt(film.variance_of_mean().astype(np.float64))
            with np.errstate(divide="ignore", invalid="ignore"):
                need = np.max(sd / np.abs(m), axis=-1)
            need = need[(film.sample_counts() == film.samples) & np.isfinite(need) & (need > 0)]
            film.adapt(float(np.quantile(need, 0.4)) if need.size else 0.0, 0.0, 4)
        counts = film.sample_counts()
        assert counts.min() < 16 and counts.max() == 16 and len(np.unique(counts)) > 2, np.unique(counts)
        guide.render(16)
        albedo.render(16)
        albedo.adapt(0.0, 0.0, 2)                                               # retires the albedo film's zero-variance pixels
        albedo.render(8)
        assert albedo.sample_counts().min() == 16 and albedo.sample_counts().max() == 24
        _check_job(film, guide, albedo, demodulate=True)
        _check_job(film, None, albedo)


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------------

def _refused(spt, status, film, guide=None, albedo=None, **kw):
    with pytest.raises(spt.SptError) as e:
        film.denoise_job(guide, albedo, **kw)
    assert e.value.status == status, (e.value.status, str(e.value))


def _raw_job(spt, film, job, rgb8=False):
    out = np.zeros((film.rows, film.width, 3), np.uint8 if rgb8 else np.float32)
    return spt.hip_lib().spt_film_denoise_job(film._handle(), C.byref(job), out.ctypes.data), out


def test_refusals_leave_the_films_usable(spt):
    sc, other, bez = _scene(spt, "cfg2_cube.json"), _scene(spt, "cfg2_cube.json"), _scene(spt, "t_bezier.json")
    r = _tracer(spt)
    cfg = spt.OutputConfig(48, 32)
    assert spt.render_flags_supported() & 16 and spt.render_flags_supported() & 32
    # the two first-hit flags exclude each other, in spt_render and in spt_film_create
    both = spt.RENDER_DEBUG_NORMAL | spt.RENDER_AOV_ALBEDO
    for scene, c in ((sc, cfg), (bez, spt.OutputConfig(48, 32, None, "main"))):
        with pytest.raises(spt.SptError) as e:
            r.progressive(scene, c, moments=True, flags=both)
        assert e.value.status == INVALID
        with pytest.raises(spt.SptError) as e:
            _tracer(spt, debug_normal=True, aov_albedo=True).render_shard(scene, c)
        assert e.value.status == INVALID
    with r.progressive(sc, cfg, moments=True) as film, r.guide_film(sc, cfg) as guide, r.albedo_film(sc, cfg) as albedo:
        for f in (film, guide, albedo):
            f.render(4)
        want = film.denoise_job(guide, albedo, demodulate=True)
        state = _state(film), _state(guide), _state(albedo)
        # without an albedo film and without DEMODULATE: spt_film_denoise, with and without a guide
        assert _util.same_words(film.denoise_job(guide), film.denoise(guide)) and _util.same_words(film.denoise_job(), film.denoise())
        assert _util.same_words(film.denoise_job(guide, iterations=2, k_guide=3.0), film.denoise(guide, iterations=2, k_guide=3.0))
        assert np.array_equal(film.denoise_job(guide, rgb8=True), film.read_rgb8("denoised", guide))
        _refused(spt, INVALID, film, guide, None, demodulate=True)              # DEMODULATE needs the albedo film
        _refused(spt, INVALID, film, guide, film)                               # albedo == film
        _refused(spt, INVALID, film, guide, guide)                              # albedo == guide
        _refused(spt, INVALID, film, film, albedo)                              # (the guide's own refusals stay)
        with r.progressive(sc, cfg, flags=spt.RENDER_AOV_ALBEDO) as no_moments:
            no_moments.render(4)
            _refused(spt, INVALID, film, guide, no_moments)
        with r.albedo_film(sc, cfg) as young:
            _refused(spt, INVALID, film, guide, young)                          # no samples
            young.render(1)
            _refused(spt, INVALID, film, guide, young)                          # one sample: no variance
            young.render(1)
            _check_job(film, guide, young)
        with r.albedo_film(other, cfg) as foreign:                              # another scene object of the same file
            foreign.render(4)
            _refused(spt, INVALID, film, guide, foreign)
        for bad_cfg, kw in ((spt.OutputConfig(32, 32), {}), (spt.OutputConfig(48, 48), {}), (cfg, dict(strip_rows=8))):
            with r.progressive(sc, bad_cfg, moments=True, flags=spt.RENDER_AOV_ALBEDO, **kw) as a2:
                a2.render(4)
                _refused(spt, INVALID, film, guide, a2)
        for bad in (dict(k_albedo=0.0), dict(k_albedo=-1.0), dict(k_albedo=float("nan")), dict(eps_albedo=float("inf")), dict(eps_albedo=0.0),
                    dict(eps_demod=0.0), dict(eps_demod=float("nan")), dict(eps_demod=-1e-2), dict(iterations=0), dict(iterations=9),
                    dict(k_color=0.0), dict(eps_guide=float("inf"))):
            _refused(spt, INVALID, film, guide, albedo, **bad)
            _refused(spt, INVALID, film, guide, albedo, demodulate=True, **bad)
            _refused(spt, INVALID, film, guide, None, **bad)                    # (checked without an albedo film too)
        # the struct: a size that ends before k_albedo, unknown flags; a size that ends before the three floats takes their defaults
        dp = spt.DenoiseParams(C.sizeof(spt.DenoiseParams), 5, 2.0, 1.0, 1e-8, 1e-2)
        job = lambda size, flags, **kw: spt.DenoiseJob(size, flags, guide._handle(), albedo._handle(), C.pointer(dp), kw.get("k", 1.0), 1e-2, 1e-2, 0)
        assert _raw_job(spt, film, job(spt.DenoiseJob.k_albedo.offset - 4, spt.DENOISE_DEMODULATE))[0] == INVALID
        assert _raw_job(spt, film, job(C.sizeof(spt.DenoiseJob), 4))[0] == INVALID
        assert _raw_job(spt, film, job(C.sizeof(spt.DenoiseJob), 0x80000001))[0] == INVALID
        st, out = _raw_job(spt, film, job(spt.DenoiseJob.k_albedo.offset, spt.DENOISE_DEMODULATE, k=float("nan")))   # k_albedo is not read
        assert st == 0 and _util.same_words(out, want)
        short = spt.DenoiseParams(C.sizeof(spt.DenoiseParams) - 4, 5, 2.0, 1.0, 1e-8, 1e-2)
        bad_params = spt.DenoiseJob(C.sizeof(spt.DenoiseJob), 0, guide._handle(), albedo._handle(), C.pointer(short), 1.0, 1e-2, 1e-2, 0)
        assert _raw_job(spt, film, bad_params)[0] == INVALID
        no_params = spt.DenoiseJob(C.sizeof(spt.DenoiseJob), spt.DENOISE_DEMODULATE, guide._handle(), albedo._handle(), None, 1.0, 1e-2, 1e-2, 0)
        st, out = _raw_job(spt, film, no_params)                                # params NULL: the defaults
        assert st == 0 and _util.same_words(out, want)
        r_box = _tracer(spt, filter_radius=0.3)
        with r_box.progressive(sc, cfg, moments=True, flags=spt.RENDER_AOV_ALBEDO) as box_albedo:
            box_albedo.render(4)
            _refused(spt, UNSUPPORTED, film, guide, box_albedo)
        layout = dict(shard_index=1, shard_count=3, strip_rows=8)
        with r.progressive(sc, cfg, moments=True, **layout) as shard, r.progressive(sc, cfg, moments=True, flags=spt.RENDER_AOV_ALBEDO, **layout) as shard_albedo:
            shard.render(4)
            shard_albedo.render(4)
            _refused(spt, UNSUPPORTED, shard, None, shard_albedo)
            _refused(spt, INVALID, film, guide, shard_albedo)                   # another shard layout than the film's
        cfg_b = spt.OutputConfig(48, 32, None, "main")
        with r.progressive(bez, cfg_b, moments=True) as f_film, r.guide_film(bez, cfg_b) as f_guide, r.albedo_film(bez, cfg_b) as f_albedo:
            for f in (f_film, f_guide, f_albedo):                               # films of the other library
                f.render(4)
            _refused(spt, INVALID, film, guide, f_albedo)
            _refused(spt, INVALID, film, f_guide, albedo)
            _refused(spt, INVALID, f_film, f_guide, albedo)
            _refused(spt, INVALID, f_film, guide, f_albedo)
            _refused(spt, INVALID, f_film, f_guide, f_film)
            _refused(spt, INVALID, f_film, f_guide, f_guide)
            _refused(spt, INVALID, f_film, f_guide, None, demodulate=True)
            _refused(spt, INVALID, f_film, f_guide, f_albedo, eps_demod=0.0)
            _check_job(f_film, f_guide, f_albedo, demodulate=True)              # forwarded with the three inner handles
            assert _util.same_words(f_film.denoise_job(f_guide), f_film.denoise(f_guide))
        # the films beside every refused call are what they were
        assert _util.same_words(film.denoise_job(guide, albedo, demodulate=True), want)
        assert all(_same_state(_state(f), s) for f, s in zip((film, guide, albedo), state))
        for f in (film, guide, albedo):
            f.render(4)
        _check_job(film, guide, albedo, demodulate=True)
    for s in (sc, other, bez):
        s.close()


# ---- 4. the CLI ------------------------------------------------------------------------------------------------------------------

def test_cli_guides(spt, tmp_path):
    scene, renderer = os.path.join(_util.SCENES, "cfg2_cube.json"), os.path.join(_util.SCENES, "pt.json")
    w, h, spp = 48, 32, 16
    base = ["-s", scene, "-r", renderer, "-w", str(w), "-h", str(h), "--spp", str(spp), "--seed", "3"]
    cli = os.path.join(spt.LIB_DIR, "spt")
    out, a_out, plain, alb_only = tmp_path / "o.png", tmp_path / "a.png", tmp_path / "p.png", tmp_path / "ao.png"
    for args in (["-o", str(out), "--denoise", "--guide", "both", "--demodulate", "--albedo-out", str(a_out)], ["-o", str(plain), "--denoise"],
                 ["-o", str(alb_only), "--guide", "albedo"]):
        res = subprocess.run([cli] + base + args, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
    sc = spt.load_scene(scene)
    ren = spt.load_renderer(renderer, seed=3)
    ren.spp = spp
    cfg = spt.OutputConfig(w, h)
    with ren.progressive(sc, cfg, moments=True) as film, ren.guide_film(sc, cfg) as guide, ren.albedo_film(sc, cfg) as albedo:
        guide.render(16)                                    # the CLI's default --guide-samples, before the first increment
        albedo.render(16)
        film.render(spp)
        assert np.array_equal(spt.read_png(out)[..., :3], film.denoise_job(guide, albedo, demodulate=True, rgb8=True))
        assert np.array_equal(spt.read_png(a_out)[..., :3], albedo.read_rgb8("mean"))
        assert np.array_equal(spt.read_png(alb_only)[..., :3], film.denoise_job(None, albedo, rgb8=True))
        assert np.array_equal(spt.read_png(plain)[..., :3], film.read_rgb8("denoised", guide))      # plain --denoise: the bytes it wrote before
        assert not np.array_equal(spt.read_png(out)[..., :3], spt.read_png(plain)[..., :3])
    sc.close()
