"""Progressive rendering (ABI v14, spt_film_*): a film takes the samples of a fixed plan in increments of any size.

Sample s of pixel p depends only on (seed, p, s) and the plan's spp, and the film is a running sum in sample order, so
increments that add up to spp give the bits of one spt_render; the moments (sum of squares) and the variance of the mean
are checked against sequential float32 numpy over the single samples.
"""
import os
import subprocess

import numpy as np
import pytest

import _util

pytestmark = pytest.mark.gpu

L1_TOL = 1e-3   # the parity suite's gate (BASELINE.json north_star: per-pixel mean L1 < 1e-3)
SAMPLERS = {"random": 0, "jittered": 1, "recurrence": 2}


@pytest.fixture(scope="module")
def spt():
    return _util.load_pkg()


def _scene(spt, name):
    return spt.load_scene(os.path.join(_util.SCENES, name))


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32), equal_nan=True)


def _schedules(spp):
    odd, pattern = [], [3, 7, 5]
    while sum(odd) < spp:
        odd.append(min(pattern[len(odd) % 3], spp - sum(odd)))
    return {"whole": [spp], "ones": [1] * 5 + [spp - 5], "odd": odd, "quarters": [spp // 4] * 4}


def _progressive_mean(spt, r, sc, cfg, schedule, **kw):
    with r.progressive(sc, cfg, **kw) as film:
        for n in schedule:
            film.render(n)
        assert film.samples == sum(schedule)
        return film.mean()


@pytest.mark.parametrize("sampler", ["random", "jittered", "recurrence"])
@pytest.mark.parametrize("scene_name,camera,w,h", [
    ("cfg1_sphere.json", None, 64, 48),
    ("cfg2_cube.json", None, 256, 256),
    ("t_materials.json", "main", 64, 48),     # environment: the chunked primary kernel for single samples too
    ("t_textured.json", None, 64, 48),        # auxiliary rays: 1/sqrt(spp) of the PLAN
    ("t_medium.json", None, 64, 48),
    ("t_bezier.json", "main", 64, 48),        # libspt_hip_bez.so: the film calls are forwarded
    ("t_pndf.json", "main", 64, 48),
])
def test_increments_equal_one_call(spt, scene_name, camera, w, h, sampler):
    sc = _scene(spt, scene_name)
    r = spt.PathTracer(max_depth=6, sampler=SAMPLERS[sampler], spp=16, division_x=4, division_y=4, seed=7)
    cfg = spt.OutputConfig(w, h, None, camera)
    ref = r.render_shard(sc, cfg).copy()
    for name, schedule in _schedules(r.spp).items():
        got = _progressive_mean(spt, r, sc, cfg, schedule)
        assert _same(got, ref), "%s: schedule %s differs from one call" % (scene_name, name)
    sc.close()


@pytest.mark.parametrize("variant", ["radius_0.3", "debug_normal", "shard_1_of_3", "samples_per_pass_5", "max_depth_0"])
def test_increments_equal_one_call_variants(spt, variant):
    sc = _scene(spt, "t_materials.json")
    r = spt.PathTracer(max_depth=0 if variant == "max_depth_0" else 5, sampler=spt.SAMPLER_RANDOM, spp=16, seed=3,
                       filter_radius=0.3 if variant == "radius_0.3" else 0.5, debug_normal=variant == "debug_normal")
    cfg = spt.OutputConfig(72, 56, None, "main")
    kw = {}
    if variant == "shard_1_of_3":
        kw = dict(shard_index=1, shard_count=3, strip_rows=8)
    ref = r.render_shard(sc, cfg, samples_per_pass=5 if variant == "samples_per_pass_5" else 0, **kw).copy()
    if variant == "samples_per_pass_5":
        kw = dict(samples_per_pass=5)
    schedules = [[8, 8]] if variant == "samples_per_pass_5" else list(_schedules(r.spp).values())
    for schedule in schedules:
        got = _progressive_mean(spt, r, sc, cfg, schedule, **kw)
        assert _same(got, ref), (variant, schedule)
    if variant == "max_depth_0":
        assert not ref.any()
    sc.close()


@pytest.mark.parametrize("scene_name,camera", [("cfg2_cube.json", None), ("t_materials.json", "main")])
def test_moments_match_sequential_numpy(spt, scene_name, camera):
    sc = _scene(spt, scene_name)
    spp = 16
    r = spt.PathTracer(max_depth=6, sampler=spt.SAMPLER_RANDOM, spp=spp, seed=11)
    cfg = spt.OutputConfig(48, 32, None, camera)
    xs = []
    for k in range(spp):   # every sample alone: a fresh film at first_sample k, one sample
        with r.progressive(sc, cfg, first_sample=k) as one:
            one.render(1)
            xs.append(one.sum())
    s = np.zeros_like(xs[0])
    q = np.zeros_like(xs[0])
    n = 0
    with r.progressive(sc, cfg, moments=True) as film:
        for inc in (1, 2, 5, 8):
            film.render(inc)
            for x in xs[n:n + inc]:
                s, q = _util.film_add_sample(s, q, x)       # s + x, q + x * x (shared with tools/fuzz_sessions.py)
            n += inc
            assert film.samples == n
            assert _same(film.sum(), s), n
            assert _same(film.sum_sq(), q), n
            m, var = _util.film_mean_and_variance(s, q, n)   # s / n; (q / n - m * m) / (n - 1) clamped at 0, inf at n = 1
            assert _same(film.mean(), m), n
            assert _same(film.variance_of_mean(), var), n
        assert _same(film.mean(), r.render_shard(sc, cfg))
    sc.close()


def test_partial_mean_equals_oracle_at_fewer_samples(spt):
    sc = _scene(spt, "cfg1_sphere.json")
    plan = spt.PathTracer(max_depth=8, sampler=spt.SAMPLER_RANDOM, spp=64, seed=5)
    w, h = 64, 48
    with plan.progressive(sc, spt.OutputConfig(w, h)) as film:
        film.render(16)
        got = film.mean()
    short = spt.PathTracer(max_depth=8, sampler=spt.SAMPLER_RANDOM, spp=16, seed=5)
    flags = _util.device_oracle_flags()
    ref, _ = _util.oracle_render(sc, short, w, h, flags=flags)
    assert float(np.abs(got - ref).mean()) < L1_TOL
    if flags == _util.ORACLE_EXHAUSTIVE:
        assert _same(got, ref)
    assert ref.max() > 0.1
    sc.close()


def test_films_are_isolated(spt):
    sc = _scene(spt, "t_materials.json")
    ra = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RANDOM, spp=12, seed=2)
    rb = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RECURRENCE, spp=9, seed=4)
    ca, cb = spt.OutputConfig(64, 48, None, "main"), spt.OutputConfig(40, 56, None, "top")
    ref_a, ref_b = ra.render_shard(sc, ca).copy(), rb.render_shard(sc, cb).copy()
    rc = spt.PathTracer(max_depth=4, sampler=spt.SAMPLER_RANDOM, spp=6, seed=9)
    cc = spt.OutputConfig(80, 64, None, "main")
    ref_c = rc.render_shard(sc, cc).copy()
    fa, fb = ra.progressive(sc, ca, moments=True), rb.progressive(sc, cb)
    fa.render(5)
    fb.render(2)
    # a synchronous render between increments, then an asynchronous one whose copy-out is still in flight
    assert _same(rc.render_shard(sc, cc).copy(), ref_c)
    fb.render(4)
    async_out = rc.render_shard(sc, cc, reuse_output=True, wait=False)
    fa.render(7)
    fb.render(3)
    rc.wait(sc)
    assert _same(async_out, ref_c)
    assert _same(fa.mean(), ref_a) and _same(fb.mean(), ref_b)
    fa.close()
    fb.close()
    sc.close()


def test_refusals_leave_the_film_unchanged(spt):
    sc = _scene(spt, "cfg2_cube.json")
    r = spt.PathTracer(max_depth=4, sampler=spt.SAMPLER_RANDOM, spp=8, seed=1)
    cfg = spt.OutputConfig(48, 32)
    with r.progressive(sc, cfg) as film:
        for read in (film.mean, film.variance_of_mean):      # nothing covered yet / no moments
            with pytest.raises(spt.SptError) as e:
                read()
            assert e.value.status == 1
        film.render(0)
        assert film.samples == 0 and not film.sum().any()
        film.render(5)
        before = film.sum()
        with pytest.raises(spt.SptError) as e:
            film.render(4)                                   # 5 + 4 > spp
        assert e.value.status == 1
        with pytest.raises(spt.SptError) as e:
            film.variance_of_mean()                          # no moments
        assert e.value.status == 1
        assert film.samples == 5 and _same(film.sum(), before)
        film.render(3)
        assert _same(film.mean(), r.render_shard(sc, cfg))
    for radius in (1.0, 1.5):                                # ceil(radius - 0.5) >= 1: neighbours' samples in one sum
        wide = spt.PathTracer(max_depth=4, sampler=spt.SAMPLER_RANDOM, spp=8, seed=1, filter_radius=radius)
        with pytest.raises(spt.SptError) as e:
            wide.progressive(sc, cfg)
        assert e.value.status == 4
    narrow = spt.PathTracer(max_depth=4, sampler=spt.SAMPLER_RANDOM, spp=8, seed=1, filter_radius=0.3)
    with narrow.progressive(sc, cfg, moments=True) as film:
        film.render(2)
        with pytest.raises(spt.SptError) as e:
            film.variance_of_mean()
        assert e.value.status == 4
        assert film.mean().shape == (32, 48, 3)
    with r.progressive(sc, cfg, moments=True) as film:
        with pytest.raises(spt.SptError) as e:
            film.variance_of_mean()                          # done == 0
        assert e.value.status == 1
    for flag in (spt.RENDER_ASYNC, spt.RENDER_PROFILE, spt.RENDER_COUNT_VISITS):
        with r.progressive(sc, cfg, flags=flag) as film:
            with pytest.raises(spt.SptError) as e:
                film.render(1)
            assert e.value.status == 1
            assert film.samples == 0 and not film.sum().any()
    sc.close()


def test_closing_the_scene_closes_its_films(spt):
    sc = _scene(spt, "cfg1_sphere.json")
    r = spt.PathTracer(max_depth=2, sampler=spt.SAMPLER_RANDOM, spp=4, seed=1)
    film = r.progressive(sc, spt.OutputConfig(16, 16))
    film.render(2)
    sc.close()
    with pytest.raises(spt.SptError):
        film.render(1)


CLI_SCENE = ["-s", os.path.join(_util.SCENES, "cfg2_cube.json"), "-r", os.path.join(_util.SCENES, "pt.json")]


def _cli(spt, args):
    return subprocess.run([os.path.join(spt.LIB_DIR, "spt")] + args, capture_output=True, text=True)


def test_cli_preview_every_writes_the_same_png(spt, tmp_path):
    plain, preview = tmp_path / "plain.png", tmp_path / "preview.png"
    args = CLI_SCENE + ["-w", "96", "-h", "64", "--spp", "80", "--seed", "3"]
    r0 = _cli(spt, args + ["-o", str(plain)])
    assert r0.returncode == 0, r0.stderr
    r1 = _cli(spt, args + ["-o", str(preview), "--preview-every", "32"])
    assert r1.returncode == 0, r1.stderr
    assert plain.read_bytes() == preview.read_bytes()


def test_cli_variance_out(spt, tmp_path):
    out, var = tmp_path / "o.png", tmp_path / "var.exr"
    r = _cli(spt, CLI_SCENE + ["-w", "64", "-h", "48", "--spp", "24", "--seed", "2", "-o", str(out), "--variance-out", str(var)])
    assert r.returncode == 0, r.stderr
    sc = spt.load_scene(CLI_SCENE[1])
    ren = spt.load_renderer(CLI_SCENE[3], seed=2)
    ren.spp = 24
    with ren.progressive(sc, spt.OutputConfig(64, 48), moments=True) as film:
        film.render(24)
        expect = film.variance_of_mean()
        assert np.array_equal(spt.read_png(out)[..., :3], spt.film_to_rgb8(film.mean()))
    assert _same(spt.read_exr(var), expect)
    assert expect.max() > 0
    sc.close()


def test_cli_time_limit(spt, tmp_path):
    out = tmp_path / "o.png"
    scene = os.path.join(_util.SCENES, "t_materials.json")
    args = ["-s", scene, "-r", CLI_SCENE[3], "-c", "main", "-w", "256", "-h", "256", "--spp", "1024", "-o", str(out)]
    r = _cli(spt, args + ["--time-limit", "0.001"])
    assert r.returncode == 0, r.stderr
    line = [l for l in r.stderr.splitlines() if l.startswith("Rendered ")]
    assert line, r.stderr
    done = int(line[0].split()[1])
    assert 64 <= done < 1024 and done % 64 == 0          # whole increments of spp / 16
    sc = spt.load_scene(scene)
    ren = spt.load_renderer(CLI_SCENE[3], seed=1)
    ren.spp = 1024
    with ren.progressive(sc, spt.OutputConfig(256, 256, None, "main")) as film:
        film.render(done)
        assert np.array_equal(spt.read_png(out)[..., :3], spt.film_to_rgb8(film.mean()))
    sc.close()
