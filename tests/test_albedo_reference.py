"""The two references of the albedo tests, checked on the CPU: the float32 restatement of spt_film_denoise_job
(tests/_denoise_job_ref.py) against the restatement of spt_film_denoise, and the emissive stand-in (tests/_albedo_ref.py), the
oracle's albedo film, against the scene's own material records."""
import os

import numpy as np
import pytest

import _albedo_ref as A
import _denoise_job_ref as J
import _denoise_ref as D
import _util

f32 = np.float32
spt = _util.load_pkg()
# the scenes tests/test_gpu_albedo.py compares on the device
STAND_IN_SCENES = ["cfg2_cube.json", "t_materials.json", "t_textured.json", "t_plastic.json", "t_pndf.json", "t_subsurface.json",
                   "t_medium.json", "t_bezier.json"]


@pytest.fixture(scope="module", autouse=True)
def cpu_build():
    _util.ensure_cpu_build()


@pytest.fixture(scope="module")
def films():
    """A noisy colour film, a guide and an albedo film of 37 x 29 pixels (the step-16 taps leave the image), one NaN pixel."""
    rng = np.random.default_rng(11)
    shape = (29, 37, 3)
    base = rng.uniform(0.05, 1.0, size=(1, 37, 3)).astype(f32) * np.linspace(0.2, 1.0, 29, dtype=f32)[:, None, None]
    m = (base + rng.normal(0, 0.05, size=shape)).astype(f32)
    v = rng.uniform(1e-4, 4e-3, size=shape).astype(f32)
    m[7, 9, 1] = np.nan
    g = rng.uniform(0, 1, size=shape).astype(f32)
    u = rng.uniform(0, 1e-3, size=shape).astype(f32)
    al = rng.uniform(0.0, 1.0, size=shape).astype(f32)
    al[3, 4] = 0.0                                          # below the demodulation floor
    ua = rng.uniform(0, 1e-3, size=shape).astype(f32)
    return m, v, g, u, al, ua


@pytest.mark.parametrize("params", [{}, dict(iterations=1), dict(iterations=3, k_color=0.75, k_guide=2.5, eps_color=3e-6, eps_guide=0.2)])
def test_without_albedo_the_restatement_is_the_denoisers(films, params):
    m, v, g, u, _, _ = films
    assert _util.same_words(J.denoise_job(m, v, g, u, **params), D.denoise(m, v, g, u, **params))
    assert _util.same_words(J.denoise_job(m, v, **params), D.denoise(m, v, **params))
    assert _util.same_words(J.denoise_job(m, v, g, u), J.denoise_job(m, v, g, u, **J.DEFAULTS))


def test_a_white_albedo_without_variance_changes_nothing(films):
    """dem = 1, e = 0, 0 / x = 0, c * 1 = c: the words of the call without an albedo film, demodulated or not."""
    m, v, g, u, _, _ = films
    one, zero = np.ones_like(m), np.zeros_like(m)
    for guide in ((g, u), (None, None)):
        want = D.denoise(m, v, *guide)
        assert _util.same_words(J.denoise_job(m, v, *guide, al=one, ua=zero, demodulate=True), want)
        assert _util.same_words(J.denoise_job(m, v, *guide, al=one, ua=zero), want)


def test_the_albedo_terms_do_something(films):
    m, v, g, u, al, ua = films
    plain, guided = J.denoise_job(m, v, g, u), J.denoise_job(m, v, g, u, al, ua)
    dem = J.denoise_job(m, v, g, u, al, ua, demodulate=True)
    assert not _util.same_words(plain, guided) and not _util.same_words(guided, dem)
    assert np.isnan(dem[7, 9, 1]) and np.isfinite(np.delete(dem.reshape(-1), (7 * 37 + 9) * 3 + 1)).all()
    # a constant colour over a textured albedo: demodulation alone (no guide term to speak of) gives the texture back
    flat = np.full_like(m, f32(0.5))
    tex = np.broadcast_to(np.where((np.indices(m.shape[:2]).sum(axis=0) % 2 == 0)[..., None], f32(0.25), f32(1.0)), m.shape).astype(f32)
    out = J.denoise_job(flat * tex, np.full_like(m, f32(1e-3)) * tex * tex, al=tex, ua=np.zeros_like(m), demodulate=True, k_albedo=1e3, eps_albedo=1e6)
    assert np.allclose(out, flat * tex, rtol=1e-5)


def test_stand_in_on_the_cube():
    """cfg2_cube at 48 x 32: every sample is the cube's c0 or black, a pixel whose samples all hit has exactly c0 as its mean."""
    sc = spt.load_scene(os.path.join(_util.SCENES, "cfg2_cube.json"))
    materials, surfaces, instances = sc.array("materials"), sc.array("surfaces"), sc.array("instances")
    assert len(instances) == 1
    mt = materials[int(surfaces[int(instances[0]["surface"])]["material"])]
    c0 = A.constant_albedo(mt)
    assert int(mt["bxdf"]) == A.BXDF_LAMBERT and _util.same_words(c0, np.array(mt["c0"], f32)) and (c0 > 0).all()
    r = spt.PathTracer(max_depth=8, sampler=spt.SAMPLER_RANDOM, spp=8, seed=5)
    plan = spt.PathTracer(max_depth=1, sampler=spt.SAMPLER_RANDOM, spp=8, seed=5)
    x = _util.oracle_render_samples(A.StandIn(sc), plan, 48, 32, 0, 8, flags=_util.ORACLE_EXHAUSTIVE)
    hit = (x.view(np.uint32) != 0).any(axis=-1)             # (8, 32, 48)
    assert _util.same_words(x[hit], np.broadcast_to(c0, x[hit].shape).copy())
    mean, var = A.albedo_film(sc, r, 48, 32, 8, flags=_util.ORACLE_EXHAUSTIVE)
    inside, outside = hit.all(axis=0), ~hit.any(axis=0)
    assert inside[16, 24] and outside[0, 0] and outside[31, 47]
    assert inside.sum() > 100 and outside.sum() > 100 and (~inside & ~outside).sum() > 10      # and an edge between them
    assert _util.same_words(mean[inside], np.broadcast_to(c0, mean[inside].shape).copy())
    assert (mean[outside].view(np.uint32) == 0).all() and (var[outside].view(np.uint32) == 0).all()
    sc.close()


@pytest.mark.parametrize("name", STAND_IN_SCENES, ids=[s[:-5] for s in STAND_IN_SCENES])
def test_scenes_meet_the_stand_ins_preconditions(name):
    """StandIn asserts them; what it derived is checked against the scene's own records."""
    sc = spt.load_scene(os.path.join(_util.SCENES, name))
    st = A.StandIn(sc)
    d = st.desc
    assert d.n_lights == 0 and d.env.width == 0 and d.env.height == 0 and d.n_instances == sc.desc.n_instances
    materials, surfaces, recipes = sc.array("materials"), sc.array("surfaces"), sc.array("material_recipes")
    for k in range(d.n_materials):
        assert d.materials[k].bxdf == A.BXDF_SPECULAR_CONDUCTOR and d.materials[k].recipe == 0
    for k in range(d.n_instances):
        assert d.instances[k].light == -1
    for k in range(d.n_surfaces):
        mt = materials[int(surfaces[k]["material"])]
        e = np.array(list(d.surfaces[k].emissive), dtype=f32)
        if int(mt["recipe"]) == 0:
            assert d.surfaces[k].emissive_map == 0 and _util.same_words(e, A.constant_albedo(mt))
        else:
            r = recipes[int(mt["recipe"]) - 1]
            textured = int(r["type"]) not in (A.MAT_CONDUCTOR, A.MAT_DIELECTRIC)
            assert d.surfaces[k].emissive_map == (int(r["tex"][0]) + 1 if textured else 0)
            assert (e == 1).all() or (int(r["type"]) == A.MAT_PBR_METALLIC and (e == e[0]).all() and 0 <= e[0] < 1)
    sc.close()
