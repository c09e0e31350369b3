"""Bucketed films on the device (spt_film_buckets, spt_film_read_buckets, spt_film_read_robust) against their float32 restatement
(tests/_robust_ref.py), bit for bit.

A sample depends only on (seed, pixel, plan index), so a one-sample film at first_sample = s returns sample s alone; the bucket sums
are then sequential float32 additions of those samples, sample s into bucket s % K, and both read-outs are float32 numpy over the
bucket sums.  S, Q and everything read from them must be those of the same film without buckets.
"""
import os
import subprocess

import numpy as np
import pytest

import _robust_ref as R
import _util

pytestmark = pytest.mark.gpu

SAMPLERS = {"random": 0, "jittered": 1, "recurrence": 2}
same = _util.same_words


@pytest.fixture(scope="module")
def spt():
    return _util.load_pkg()


def _scene(spt, name):
    return spt.load_scene(os.path.join(_util.SCENES, name))


def _renderer(spt, sampler, spp, seed=11, **kw):
    return spt.PathTracer(max_depth=5, sampler=SAMPLERS[sampler], spp=spp, division_x=4, division_y=4, seed=seed, **kw)


_single = {}


def _single_samples(spt, sc, scene_name, camera, w, h, sampler, spp, first, count):
    """The samples first .. first + count - 1 of the plan, each from a one-sample plain film; rendered once per plan."""
    key = (scene_name, camera, w, h, sampler, spp, first, count)
    if key not in _single:
        r = _renderer(spt, sampler, spp)
        xs = []
        for k in range(first, first + count):
            with r.progressive(sc, spt.OutputConfig(w, h, None, camera), first_sample=k) as one:
                one.render(1)
                xs.append(one.sum())
        _single[key] = xs
    return _single[key]


def _check_reads(film, b, s, first, done, where):
    assert same(film.bucket_sums(), b), ("bucket_sums",) + where
    for name, est in (("mon", R.MON), ("gmon", R.GMON)):
        assert same(film.robust_mean(name), R.robust(b, s, first, done, est)), (name,) + where


CUBE, MATERIALS = ("cfg2_cube.json", None), ("t_materials.json", "main")   # no environment: un-chunked primary; environment: chunked


@pytest.mark.parametrize("scene,w,h,k,moments,spp_pass,sampler", [
    (CUBE, 48, 32, 5, False, 0, "random"),
    (CUBE, 48, 32, 5, True, 0, "random"),
    (MATERIALS, 48, 32, 5, False, 0, "random"),
    (MATERIALS, 48, 32, 5, True, 0, "random"),
    (CUBE, 256, 256, 5, True, 0, "random"),          # several primary chunks
    (CUBE, 48, 32, 3, False, 0, "random"),
    (CUBE, 48, 32, 15, False, 0, "random"),
    (MATERIALS, 48, 32, 3, True, 0, "random"),
    (MATERIALS, 48, 32, 15, True, 0, "random"),
    (CUBE, 48, 32, 5, True, 5, "random"),            # pass boundaries inside the buckets
    (MATERIALS, 48, 32, 5, True, 5, "random"),
    (CUBE, 48, 32, 5, False, 0, "jittered"),
    (MATERIALS, 48, 32, 5, True, 0, "jittered"),
    (CUBE, 48, 32, 5, True, 0, "recurrence"),
    (MATERIALS, 48, 32, 5, False, 0, "recurrence"),
])
def test_buckets_are_the_sequential_sums(spt, scene, w, h, k, moments, spp_pass, sampler):
    scene_name, camera = scene
    spp, first = (16, 0) if sampler == "jittered" else (24, 3)
    sc = _scene(spt, scene_name)
    xs = _single_samples(spt, sc, scene_name, camera, w, h, sampler, spp, first, 16)
    r = _renderer(spt, sampler, spp)
    cfg = spt.OutputConfig(w, h, None, camera)
    kw = dict(first_sample=first, moments=moments, samples_per_pass=spp_pass)
    with r.progressive(sc, cfg, buckets=k, **kw) as film, r.progressive(sc, cfg, **kw) as plain:
        assert film.n_buckets == k and plain.n_buckets == 0
        assert film.bucket_sums().shape == (k, h, w, 3) and not film.bucket_sums().any()
        done = 0
        for inc in (1, 2, 5, 8):
            film.render(inc)
            plain.render(inc)
            done += inc
            where = (scene_name, k, sampler, done)
            s = plain.sum()
            assert same(film.sum(), s), where
            if moments:
                assert same(film.sum_sq(), plain.sum_sq()), where
            assert same(film.mean(), plain.mean()), where
            _check_reads(film, R.bucket_sums(xs[:done], first, k), s, first, done, where)
    sc.close()


def _schedules(spp):   # (those of test_gpu_progressive.py)
    odd, pattern = [], [3, 7, 5]
    while sum(odd) < spp:
        odd.append(min(pattern[len(odd) % 3], spp - sum(odd)))
    return {"whole": [spp], "ones": [1] * 5 + [spp - 5], "odd": odd, "quarters": [spp // 4] * 4}


@pytest.mark.parametrize("scene_name", ["t_textured.json", "t_medium.json"])
def test_schedule_independence(spt, scene_name):
    sc = _scene(spt, scene_name)
    r = _renderer(spt, "random", 16, seed=7)
    cfg = spt.OutputConfig(64, 48)
    ref = None
    for name, schedule in _schedules(16).items():
        with r.progressive(sc, cfg, buckets=5) as film:
            for n in schedule:
                film.render(n)
            got = film.bucket_sums(), film.robust_mean("mon"), film.robust_mean("gmon")
        if ref is None:
            ref = got
            assert ref[0].any()
        for a, b in zip(got, ref):
            assert same(a, b), (scene_name, name)
    sc.close()


def test_shard_buckets_are_the_rows_of_the_whole(spt):
    sc = _scene(spt, "t_materials.json")
    r = _renderer(spt, "random", 16, seed=3)
    cfg = spt.OutputConfig(72, 56, None, "main")
    with r.progressive(sc, cfg, buckets=5) as whole, r.progressive(sc, cfg, buckets=5, shard_index=1, shard_count=3, strip_rows=8) as shard:
        for n in (7, 9):
            whole.render(n)
            shard.render(n)
        rows = spt.shard_rows(56, 1, 3, 8)
        assert shard.rows == len(rows) and 0 < len(rows) < 56
        assert same(shard.bucket_sums(), whole.bucket_sums()[:, rows])
        for est in ("mon", "gmon"):
            assert same(shard.robust_mean(est), whole.robust_mean(est)[rows])
    sc.close()


def test_forwarded_library(spt):
    sc = _scene(spt, "t_bezier.json")
    xs = _single_samples(spt, sc, "t_bezier.json", "main", 64, 48, "random", 16, 0, 16)
    r = _renderer(spt, "random", 16)
    with r.progressive(sc, spt.OutputConfig(64, 48, None, "main"), buckets=5) as film:
        done = 0
        for inc in (3, 13):
            film.render(inc)
            done += inc
            _check_reads(film, R.bucket_sums(xs[:done], 0, 5), film.sum(), 0, done, ("t_bezier", done))
        with pytest.raises(spt.SptError) as e:
            film.set_buckets(5)                                  # the refusal comes back through the forwarding table
        assert e.value.status == 1 and "film_buckets" in str(e.value)
    sc.close()


def _auto_rel(s, q, n, active):   # (test_gpu_adaptive.py's: a tolerance that retires about 40 % of the noisy active pixels)
    m = s.astype(np.float64) / n
    v = np.maximum((q.astype(np.float64) / n - m * m) / (n - 1), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        need = np.max(np.sqrt(v) / np.abs(m), axis=-1)
    need = need[active & np.isfinite(need) & (need > 0)]
    return float(np.quantile(need, 0.4)) if need.size else 0.0


def test_adaptive_film_keeps_each_pixels_buckets(spt):
    """test_gpu_adaptive.py's t_materials case (64x48, 32 samples of seed 5 in eight increments of 4, the tolerance that retires
    about 40 % of the noisy active pixels at every step, min_samples 8): a retired pixel keeps the buckets of its n_p samples."""
    sc = _scene(spt, "t_materials.json")
    r = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RANDOM, spp=32, seed=5)
    cfg = spt.OutputConfig(64, 48, None, "main")
    k = 5
    with r.progressive(sc, cfg, moments=True, buckets=k) as ad, r.progressive(sc, cfg, moments=True, buckets=k) as plain:
        active = np.ones((48, 64), bool)
        n_p = np.zeros((48, 64), np.uint32)
        snaps, done = {}, 0
        for inc in [4] * 8:
            ad.render(inc)
            plain.render(inc)
            done += inc
            snaps[done] = plain.bucket_sums()
            s, q = plain.sum(), plain.sum_sq()                   # (those of the adaptive film at its active pixels)
            rel = _auto_rel(s, q, done, active)
            left = ad.adapt(rel, 0.0, 8)
            if done >= 8:
                retire = active & _util.film_criterion(s, q, done, rel, 0.0)
                n_p[retire] = done
                active &= ~retire
            assert left == int(active.sum()), (done, left, int(active.sum()))
            counts = np.where(active, np.uint32(done), n_p)
            assert np.array_equal(ad.sample_counts(), counts), done
            expect = np.empty_like(snaps[done])
            for n in np.unique(counts):
                expect[:, counts == n] = snaps[int(n)][:, counts == n]
            b = ad.bucket_sums()
            assert same(b, expect), done
            for name, est in (("mon", R.MON), ("gmon", R.GMON)):
                assert same(ad.robust_mean(name), R.robust(b, ad.sum(), 0, counts, est)), (name, done)
        assert active.any() and (~active).any()                  # both retired and active pixels at the end
        assert (n_p[~active] >= 8).all()
    sc.close()


def test_a_bad_sample_spoils_a_bucket_not_the_pixel(spt):
    """t_materials, 96x72, 2048 samples of seed 77: a few pixels take one sample that is not finite (the reference's arithmetic,
    reproduced bit for bit), which the plain mean never recovers from."""
    sc = _scene(spt, "t_materials.json")
    r = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RANDOM, spp=2048, seed=77)
    with r.progressive(sc, spt.OutputConfig(96, 72, None, "main"), buckets=9) as film:
        for _ in range(4):
            film.render(512)
        mean, b, s = film.mean(), film.bucket_sums(), film.sum()
        bad = ~np.isfinite(mean).all(axis=-1)
        print("pixels whose plain mean is not finite: %d" % bad.sum())
        assert bad.any()
        for name, est in (("mon", R.MON), ("gmon", R.GMON)):
            out = film.robust_mean(name)
            assert np.isfinite(out).all(), name
            assert same(out, R.robust(b, s, 0, 2048, est)), name
    sc.close()


def test_refusals_leave_the_film_usable(spt):
    sc = _scene(spt, "cfg2_cube.json")
    r = _renderer(spt, "random", 12, seed=1)
    cfg = spt.OutputConfig(48, 32)
    lib = spt.hip_lib()
    out = np.full((32, 48, 3), 7.0, dtype=np.float32)
    big = np.full((15, 32, 48, 3), 7.0, dtype=np.float32)

    def refused(call, status=1):
        with pytest.raises(spt.SptError) as e:
            call()
        assert e.value.status == status, str(e.value)

    with r.progressive(sc, cfg, buckets=5) as ref:
        ref.render(12)
        ref_b, ref_mon, ref_gmon, ref_s = ref.bucket_sums(), ref.robust_mean("mon"), ref.robust_mean("gmon"), ref.sum()
    with r.progressive(sc, cfg) as film:
        assert lib.spt_film_read_buckets(film._handle(), big.ctypes.data) == 1      # a film without buckets
        assert "film_read_buckets" in lib.spt_last_error().decode()
        assert lib.spt_film_read_robust(film._handle(), spt.ROBUST_GMON, out.ctypes.data) == 1
        for n in (4, 8, 1, 17, 0, 2):
            refused(lambda: film.set_buckets(n))
        assert film.n_buckets == 0
        film.set_buckets(5)
        refused(lambda: film.set_buckets(5))                                        # a second time
        refused(lambda: film.set_buckets(7))
        refused(lambda: film.robust_mean("gmon"))                                   # done == 0
        assert lib.spt_film_read_robust(film._handle(), 2, out.ctypes.data) == 1    # (an unknown estimator, before and after samples)
        assert not film.bucket_sums().any()
        film.render(5)
        assert lib.spt_film_read_robust(film._handle(), 2, out.ctypes.data) == 1
        assert "film_read_robust" in lib.spt_last_error().decode()
        refused(lambda: film.set_buckets(5))
        assert (out == 7.0).all() and (big == 7.0).all()
        film.render(7)
        assert same(film.bucket_sums(), ref_b) and same(film.sum(), ref_s)
        assert same(film.robust_mean("mon"), ref_mon) and same(film.robust_mean("gmon"), ref_gmon)
    with r.progressive(sc, cfg) as film:                                            # buckets only before the first sample
        film.render(5)
        refused(lambda: film.set_buckets(5))
        assert film.n_buckets == 0
        film.render(7)
        assert same(film.sum(), ref_s)
    narrow = _renderer(spt, "random", 12, seed=1, filter_radius=0.3)
    with narrow.progressive(sc, cfg) as film:
        refused(lambda: film.set_buckets(5), status=4)
        film.render(12)
        assert film.mean().shape == (32, 48, 3)
    with pytest.raises(spt.SptError) as e:
        narrow.progressive(sc, cfg, buckets=5)
    assert e.value.status == 4
    sc.close()


def test_nothing_else_moves(spt):
    sc = _scene(spt, "t_materials.json")
    r = _renderer(spt, "random", 16, seed=9)
    cfg = spt.OutputConfig(64, 48, None, "main")
    with r.progressive(sc, cfg, moments=True, buckets=5) as film, r.progressive(sc, cfg, moments=True) as plain:
        film.render(6)
        plain.render(6)
        film.robust_mean("gmon")
        film.robust_mean("mon")
        assert same(film.denoise(), plain.denoise())
        assert same(film.variance_of_mean(), plain.variance_of_mean())
        film.render(10)                                           # after read_robust and denoise: on to the bits of an undisturbed film
        plain.render(10)
        assert same(film.sum(), plain.sum()) and same(film.sum_sq(), plain.sum_sq())
        assert same(film.denoise(), plain.denoise())
        b = film.bucket_sums()
    with r.progressive(sc, cfg, moments=True, buckets=5) as undisturbed:
        undisturbed.render(16)
        assert same(undisturbed.bucket_sums(), b)
        assert same(undisturbed.mean(), r.render_shard(sc, cfg))
    sc.close()


def test_cli_robust(spt, tmp_path):
    out, mean = tmp_path / "o.png", tmp_path / "mean.png"
    scene, renderer = os.path.join(_util.SCENES, "cfg2_cube.json"), os.path.join(_util.SCENES, "pt.json")
    res = subprocess.run([os.path.join(spt.LIB_DIR, "spt"), "-s", scene, "-r", renderer, "-w", "96", "-h", "72", "--spp", "36", "--seed", "3",
                          "-o", str(out), "--robust", "9", "--mean-out", str(mean)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    sc = spt.load_scene(scene)
    ren = spt.load_renderer(renderer, seed=3)
    ren.spp = 36
    with ren.progressive(sc, spt.OutputConfig(96, 72), buckets=9) as film:
        film.render(36)
        assert np.array_equal(spt.read_png(out)[..., :3], spt.film_to_rgb8(film.robust_mean("gmon")))
        assert np.array_equal(spt.read_png(mean)[..., :3], spt.film_to_rgb8(film.mean()))
        assert not np.array_equal(spt.film_to_rgb8(film.robust_mean("gmon")), spt.film_to_rgb8(film.mean()))
    sc.close()
