"""The film denoiser on the device (spt_film_denoise) against its float32 restatement (tests/_denoise_ref.py), bit for bit.

The restatement takes what the films themselves read out (mean and variance of the mean of the colour film and of the guide), so
every comparison here is about the filter alone: k_denoise_pack and k_denoise_atrous.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _denoise_ref as D
import _util

pytestmark = pytest.mark.gpu

NON_DEFAULT = dict(iterations=4, k_color=0.75, k_guide=2.5, eps_color=3e-6, eps_guide=0.2)
SCENES = [
    ("cfg2_cube.json", None),
    ("t_materials.json", "main"),
    ("t_textured.json", None),
    ("t_plastic.json", None),
    ("t_medium.json", None),
    ("t_bezier.json", "main"),        # libspt_hip_bez.so: the call is forwarded, both inner films together
]


@pytest.fixture(scope="module")
def spt():
    pkg = _util.load_pkg()
    _util.ensure_cpu_build()          # the restatement's exp is the oracle's spt_exp
    return pkg


def _scene(spt, name):
    return spt.load_scene(os.path.join(_util.SCENES, name))


def _tracer(spt, spp=16, seed=5, **kw):
    return spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RANDOM, spp=spp, seed=seed, **kw)


def _inputs(film, guide=None):
    """What the restatement reads: (m, v) of the film, then (g, u) of the guide."""
    out = [film.mean(), film.variance_of_mean()]
    if guide is not None:
        out += [guide.mean(), guide.variance_of_mean()]
    return out


def _check(film, guide, **params):
    got = film.denoise(guide, **params)
    want = D.denoise(*_inputs(film, guide), **params)
    assert _util.same_words(got, want), (params, guide is not None, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    return got


@pytest.mark.parametrize("scene_name,camera", SCENES, ids=[s[0][:-5] for s in SCENES])
def test_device_equals_restatement(spt, scene_name, camera):
    sc = _scene(spt, scene_name)
    r = _tracer(spt)
    cfg = spt.OutputConfig(70, 50, None, camera)            # no multiple of the 16x16 tile; 5 x 4 blocks
    with r.progressive(sc, cfg, moments=True) as film, r.guide_film(sc, cfg) as guide:
        film.render(16)
        guide.render(16)
        for k in (1, 3, 5, 8):                              # 8: steps up to 128, far wider than the image
            a = _check(film, guide, iterations=k)
            b = _check(film, None, iterations=k)
        assert not _util.same_words(a, b) and not _util.same_words(a, film.mean())
        _check(film, guide, **NON_DEFAULT)
        _check(film, None, **NON_DEFAULT)
        assert _util.same_words(film.denoise(guide), film.denoise(guide, **D.DEFAULTS))
    sc.close()


@pytest.mark.parametrize("w,h", [(24, 20), (96, 72), (16, 16), (17, 3)])
def test_sizes(spt, w, h):
    """An image smaller than the largest step of 5 iterations (16), whole tiles, one tile, a sliver."""
    sc = _scene(spt, "t_materials.json")
    r = _tracer(spt)
    cfg = spt.OutputConfig(w, h, None, "main")
    with r.progressive(sc, cfg, moments=True) as film, r.guide_film(sc, cfg) as guide:
        film.render(8)
        guide.render(4)                                     # the two films need not cover the same samples
        _check(film, guide)
        _check(film, None)
        _check(film, guide, iterations=2)                   # after 5: the workspace is reused
    sc.close()


def test_adaptive_films(spt):
    """The input is each pixel's mean and variance at its own sample count n_p (mask / counts / inv, as k_film_read_counts)."""
    sc = _scene(spt, "t_materials.json")
    r = _tracer(spt, spp=32)
    cfg = spt.OutputConfig(64, 48, None, "main")
    with r.progressive(sc, cfg, moments=True) as film, r.guide_film(sc, cfg) as guide:
        for _ in range(8):
            film.render(4)
            n = film.samples                                # a tolerance that retires about 40 % of the noisy active pixels
            m, sd = film.mean().astype(np.float64), np.sqrt(film.variance_of_mean().astype(np.float64))
            with np.errstate(divide="ignore", invalid="ignore"):
                need = np.max(sd / np.abs(m), axis=-1)
            need = need[(film.sample_counts() == n) & np.isfinite(need) & (need > 0)]
            film.adapt(float(np.quantile(need, 0.4)) if need.size else 0.0, 0.0, 4)
        counts = film.sample_counts()
        assert counts.min() < 32 and counts.max() == 32 and len(np.unique(counts)) > 2, np.unique(counts)
        guide.render(8)
        _check(film, guide)
        _check(film, None)
        guide.adapt(0.0, 0.0, 2)                            # retires the zero-variance pixels of the guide (flat normals)
        guide.render(8)
        g_counts = guide.sample_counts()
        assert g_counts.min() == 8 and g_counts.max() == 16
        _check(film, guide)
    sc.close()


@pytest.fixture(scope="module")
def materials_2048(spt):
    """t_materials, camera main, 96x72, 2048 samples of seed 77: the quality gate's reference plan, whose film has pixels that are
    not finite.  (mean, variance of the mean, denoised with a guide, denoised without, guide inputs)"""
    sc = _scene(spt, "t_materials.json")
    P = D.QUALITY_PLAN
    r = _tracer(spt, spp=P["ref_spp"], seed=P["ref_seed"])
    cfg = spt.OutputConfig(P["width"], P["height"], None, "main")
    with r.progressive(sc, cfg, moments=True) as film, r.guide_film(sc, cfg) as guide:
        film.render(P["ref_spp"])
        guide.render(16)
        res = dict(m=film.mean(), v=film.variance_of_mean(), g=guide.mean(), u=guide.variance_of_mean(),
                   guided=film.denoise(guide), plain=film.denoise())
    sc.close()
    return res


def test_non_finite_pixels_pass_through(materials_2048):
    f = materials_2048
    bad = ~np.isfinite(f["m"]).all(axis=-1)
    assert bad.sum() >= 1                                   # (the oracle's film of this plan has 2)
    assert bad.sum() <= D.MAX_LEFT_OUT * bad.size
    for got, want in ((f["guided"], D.denoise(f["m"], f["v"], f["g"], f["u"])), (f["plain"], D.denoise(f["m"], f["v"]))):
        assert np.array_equal(~np.isfinite(got).all(axis=-1), bad)
        assert _util.same_words(got[bad], f["m"][bad])
        assert _util.same_words(got, want)


@pytest.mark.parametrize("name,camera,bound,bound_no_guide", D.QUALITY_SCENES, ids=[s[0][:-5] for s in D.QUALITY_SCENES])
def test_quality_on_gpu_films(spt, materials_2048, name, camera, bound, bound_no_guide):
    """The gate of test_denoise_reference.py on the device's films and the device's filter: the same thresholds."""
    P = D.QUALITY_PLAN
    sc = _scene(spt, name)
    cfg = spt.OutputConfig(P["width"], P["height"], None, camera)
    ref = materials_2048["m"] if name == "t_materials.json" else _tracer(spt, spp=P["ref_spp"], seed=P["ref_seed"]).render_shard(sc, cfg)
    r = _tracer(spt, spp=P["spp"], seed=P["seed"])
    with r.progressive(sc, cfg, moments=True) as film, r.guide_film(sc, cfg) as guide:
        film.render(P["spp"])
        guide.render(P["spp"])
        noisy, guided, plain = film.mean(), film.denoise(guide), film.denoise()
    sc.close()
    n_pix = P["width"] * P["height"]
    ratio, left_out = D.rmse_ratio(noisy, guided, ref)
    print("%s: with guide %.4f, %d of %d pixels left out" % (name, ratio, left_out, n_pix))
    assert left_out <= D.MAX_LEFT_OUT * n_pix
    assert (ratio < 1.0) if bound == 1.0 else (ratio <= bound), ratio
    if bound_no_guide is not None:
        ratio, left_out = D.rmse_ratio(noisy, plain, ref)
        print("%s: without guide %.4f" % (name, ratio))
        assert left_out <= D.MAX_LEFT_OUT * n_pix
        assert ratio <= bound_no_guide, ratio


def _state(film):
    return film.sum(), film.sum_sq(), film.samples, film.sample_counts()


def _same_state(a, b):
    return _util.same_words(a[0], b[0]) and _util.same_words(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3])


def test_neither_film_changes(spt):
    sc = _scene(spt, "t_materials.json")
    r = _tracer(spt, spp=24)
    cfg = spt.OutputConfig(64, 48, None, "main")
    with r.progressive(sc, cfg, moments=True) as film, r.guide_film(sc, cfg) as guide, \
            r.progressive(sc, cfg, moments=True) as alone, r.guide_film(sc, cfg) as guide_alone:
        for f in (film, guide, alone, guide_alone):
            f.render(8)
        film.adapt(0.1, 1e-3, 4)
        alone.adapt(0.1, 1e-3, 4)
        before = _state(film), _state(guide)
        first = film.denoise(guide)
        film.denoise()
        assert _util.same_words(film.denoise(guide, iterations=3), D.denoise(*_inputs(film, guide), iterations=3))
        assert _same_state(_state(film), before[0]) and _same_state(_state(guide), before[1])
        for f in (film, guide, alone, guide_alone):         # the films go on to the bits of undisturbed ones
            f.render(8)
        assert _same_state(_state(film), _state(alone)) and _same_state(_state(guide), _state(guide_alone))
        assert _util.same_words(film.mean(), alone.mean()) and _util.same_words(guide.variance_of_mean(), guide_alone.variance_of_mean())
        assert not _util.same_words(film.denoise(guide), first)
    sc.close()


def _refused(spt, status, film, guide=None, **params):
    with pytest.raises(spt.SptError) as e:
        film.denoise(guide, **params)
    assert e.value.status == status, (e.value.status, str(e.value))


def test_refusals_leave_both_films_usable(spt):
    INVALID, UNSUPPORTED = 1, 4
    sc, other, bez = _scene(spt, "cfg2_cube.json"), _scene(spt, "cfg2_cube.json"), _scene(spt, "t_bezier.json")
    r = _tracer(spt)
    cfg = spt.OutputConfig(48, 32)
    with r.progressive(sc, cfg, moments=True) as film, r.guide_film(sc, cfg) as guide:
        film.render(4)
        guide.render(4)
        want = film.denoise(guide)
        state = _state(film), _state(guide)
        with r.progressive(sc, cfg) as no_moments:
            no_moments.render(4)
            _refused(spt, INVALID, no_moments)
            _refused(spt, INVALID, no_moments, guide)
            _refused(spt, INVALID, film, no_moments)
        with r.progressive(sc, cfg, moments=True) as young, r.guide_film(sc, cfg) as young_guide:
            _refused(spt, INVALID, young)                   # no samples
            _refused(spt, INVALID, film, young_guide)
            young.render(1)
            young_guide.render(1)
            _refused(spt, INVALID, young, guide)            # one sample: no variance
            _refused(spt, INVALID, film, young_guide)
            young.render(1)
            young_guide.render(1)
            assert _util.same_words(young.denoise(young_guide), D.denoise(*_inputs(young, young_guide)))   # usable afterwards
        _refused(spt, INVALID, film, film)
        with r.guide_film(other, cfg) as foreign:           # another scene object of the same file
            foreign.render(4)
            _refused(spt, INVALID, film, foreign)
        for bad_cfg, kw in ((spt.OutputConfig(32, 32), {}), (spt.OutputConfig(48, 48), {}), (cfg, dict(strip_rows=8))):
            with r.progressive(sc, bad_cfg, moments=True, flags=spt.RENDER_DEBUG_NORMAL, **kw) as g2:
                g2.render(4)
                _refused(spt, INVALID, film, g2)
        for bad in (dict(iterations=0), dict(iterations=9), dict(k_color=0.0), dict(k_color=-1.0), dict(k_color=float("nan")),
                    dict(k_guide=float("inf")), dict(k_guide=0.0), dict(eps_color=0.0), dict(eps_color=float("nan")),
                    dict(eps_guide=-1e-2), dict(eps_guide=float("inf"))):
            _refused(spt, INVALID, film, guide, **bad)
            _refused(spt, INVALID, film, None, **bad)
        short = spt.DenoiseParams(C.sizeof(spt.DenoiseParams) - 4, 5, 2.0, 1.0, 1e-8, 1e-2)     # a struct older than the first
        out = np.zeros((film.rows, film.width, 3), np.float32)
        assert spt.hip_lib().spt_film_denoise(film._handle(), None, C.byref(short), out.ctypes.data) == INVALID
        assert spt.hip_lib().spt_film_denoise(film._handle(), guide._handle(), None, out.ctypes.data) == 0   # NULL: the defaults
        assert _util.same_words(out, want)
        r_box = _tracer(spt, filter_radius=0.3)
        with r_box.progressive(sc, cfg, moments=True) as box, r_box.progressive(sc, cfg, moments=True, flags=spt.RENDER_DEBUG_NORMAL) as box_guide:
            box.render(4)
            box_guide.render(4)
            _refused(spt, UNSUPPORTED, box)
            _refused(spt, UNSUPPORTED, box, guide)
            _refused(spt, UNSUPPORTED, film, box_guide)
        layout = dict(shard_index=1, shard_count=3, strip_rows=8)
        with r.progressive(sc, cfg, moments=True, **layout) as shard, r.progressive(sc, cfg, moments=True, flags=spt.RENDER_DEBUG_NORMAL, **layout) as shard_guide:
            shard.render(4)
            shard_guide.render(4)
            _refused(spt, UNSUPPORTED, shard)
            _refused(spt, UNSUPPORTED, shard, shard_guide)
            _refused(spt, INVALID, film, shard_guide)       # another shard layout than the film's
        cfg_b = spt.OutputConfig(48, 32, None, "main")
        with r.progressive(bez, cfg_b, moments=True) as fwd_film, r.guide_film(bez, cfg_b) as fwd_guide:   # films of the other library
            fwd_film.render(4)
            fwd_guide.render(4)
            _refused(spt, INVALID, film, fwd_guide)
            _refused(spt, INVALID, fwd_film, guide)
            _refused(spt, INVALID, fwd_film, fwd_film)
            _refused(spt, INVALID, fwd_film, fwd_guide, iterations=9)
            assert _util.same_words(fwd_film.denoise(fwd_guide), D.denoise(*_inputs(fwd_film, fwd_guide)))
        assert _util.same_words(film.denoise(guide), want)
        assert _same_state(_state(film), state[0]) and _same_state(_state(guide), state[1])
        film.render(4)
        guide.render(4)
        _check(film, guide)
    for s in (sc, other, bez):
        s.close()


def test_cli_denoise(spt, tmp_path):
    scene, renderer = os.path.join(_util.SCENES, "cfg2_cube.json"), os.path.join(_util.SCENES, "pt.json")
    out, noisy = tmp_path / "o.png", tmp_path / "noisy.png"
    w, h, spp = 64, 64, 16
    args = ["-s", scene, "-r", renderer, "-w", str(w), "-h", str(h), "--spp", str(spp), "--seed", "3", "-o", str(out), "--denoise",
            "--noisy-out", str(noisy)]
    res = subprocess.run([os.path.join(spt.LIB_DIR, "spt")] + args, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert out.exists() and noisy.exists()
    sc = spt.load_scene(scene)
    ren = spt.load_renderer(renderer, seed=3)
    ren.spp = spp
    cfg = spt.OutputConfig(w, h)
    with ren.progressive(sc, cfg, moments=True) as film, ren.guide_film(sc, cfg) as guide:
        guide.render(16)                                    # the CLI's default --guide-samples, before the first increment
        film.render(spp)
        assert np.array_equal(spt.read_png(out)[..., :3], spt.film_to_rgb8(film.denoise(guide)))
        assert np.array_equal(spt.read_png(noisy)[..., :3], spt.film_to_rgb8(film.mean()))
        assert not np.array_equal(spt.read_png(out)[..., :3], spt.read_png(noisy)[..., :3])
    sc.close()
