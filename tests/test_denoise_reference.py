"""The float32 restatement of spt_film_denoise (tests/_denoise_ref.py) on films of the CPU oracle: it removes noise.

The plan is 96x72, 16 samples of the random sampler, seed 5, max_depth 5; the guide is the same plan with debug_normal; the
reference is 2048 samples of seed 77.  Pixels that are not finite in the film or the reference are left out (at most 0.1 %).
RMSE(denoised) / RMSE(noisy), with a normal guide / without a guide, measured with this restatement:
cfg2_cube 0.942 / 1.011 (about 80 % black background; without a guide the cube's edges blur), t_materials 0.558 / 0.448,
t_textured 0.579 / 0.639, t_plastic 0.611 / 0.661, t_medium 0.241 / 0.242.  The values are deterministic; the gates (< 1 on
cfg2 with a guide, <= 0.75 on the others with and without) leave room for a re-ordering of the restatement.
"""
import os

import numpy as np
import pytest

import _denoise_ref as D
import _util

spt = _util.load_pkg()
P = D.QUALITY_PLAN


@pytest.fixture(scope="module")
def films():
    """Per scene, rendered once: the noisy film and its guide (mean, variance of the mean) and the reference image."""
    _util.ensure_cpu_build()
    cache = {}

    def get(name, camera):
        if name not in cache:
            sc = spt.load_scene(os.path.join(_util.SCENES, name))
            plan = dict(max_depth=P["max_depth"], sampler=spt.SAMPLER_RANDOM, spp=P["spp"], seed=P["seed"])
            w, h, flags = P["width"], P["height"], _util.ORACLE_DEVICE
            m, v = D.oracle_film(sc, spt.PathTracer(**plan), w, h, camera, P["spp"], flags)
            g, u = D.oracle_film(sc, spt.PathTracer(debug_normal=True, **plan), w, h, camera, P["spp"], flags)
            r_ref = spt.PathTracer(max_depth=P["max_depth"], sampler=spt.SAMPLER_RANDOM, spp=P["ref_spp"], seed=P["ref_seed"])
            ref, _ = _util.oracle_render(sc, r_ref, w, h, camera=camera, flags=flags)
            sc.close()
            cache[name] = (m, v, g, u, ref)
        return cache[name]
    return get


@pytest.mark.parametrize("name,camera,bound,bound_no_guide", D.QUALITY_SCENES, ids=[s[0][:-5] for s in D.QUALITY_SCENES])
def test_restatement_removes_noise_on_oracle_films(films, name, camera, bound, bound_no_guide):
    m, v, g, u, ref = films(name, camera)
    n_pix = m.shape[0] * m.shape[1]
    guided = D.denoise(m, v, g, u)
    ratio, left_out = D.rmse_ratio(m, guided, ref)
    print("%s: with guide %.4f, %d of %d pixels left out" % (name, ratio, left_out, n_pix))
    assert left_out <= D.MAX_LEFT_OUT * n_pix
    assert np.array_equal(np.isfinite(guided), np.isfinite(m))     # a non-finite pixel passes through and poisons nobody
    assert (ratio < 1.0) if bound == 1.0 else (ratio <= bound), ratio
    if bound_no_guide is not None:
        plain = D.denoise(m, v)
        ratio, left_out = D.rmse_ratio(m, plain, ref)
        print("%s: without guide %.4f" % (name, ratio))
        assert left_out <= D.MAX_LEFT_OUT * n_pix
        assert np.array_equal(np.isfinite(plain), np.isfinite(m))
        assert ratio <= bound_no_guide, ratio


def test_restatement_details():
    """Small hand-checkable properties: a constant image stays constant to rounding, one iteration of a flat-variance image
    without edges is the B3 kernel, a NaN pixel passes through and its neighbours stay finite."""
    _util.ensure_cpu_build()
    f32 = np.float32
    m = np.full((9, 11, 3), f32(0.5))
    v = np.full((9, 11, 3), f32(1e-3))
    out = D.denoise(m, v, iterations=3)
    assert np.abs(out - m).max() < 1e-6
    m2 = m.copy()
    m2[4, 5] = f32(np.nan)
    out = D.denoise(m2, v, iterations=3)
    assert np.isnan(out[4, 5]).all() and np.isfinite(np.delete(out.reshape(-1, 3), 4 * 11 + 5, axis=0)).all()
    # an impulse under a huge variance: every weight is the spline's (d ~ 0), so the centre keeps (3/8)^2 / sum over the window
    imp = np.zeros((9, 9, 3), f32)
    imp[4, 4] = f32(1)
    out = D.denoise(imp, np.full((9, 9, 3), f32(1e12)), iterations=1)
    assert abs(float(out[4, 4, 0]) - 9.0 / 64.0) < 1e-6 and abs(float(out[4, 2, 0]) - (3.0 / 8.0) * (1.0 / 16.0)) < 1e-6
    assert abs(float(out.sum()) / 3 - 1.0) < 1e-5
