"""Adaptive sampling of a progressive film (spt_film_adapt / spt_film_read_counts).

A sample depends only on (seed, pixel, plan index) and a film sums in sample order, so a pixel retired after n_p samples holds
exactly the bits of a plain film stopped at n_p.  Every test here runs an adaptive film next to a plain moments film of the
same plan and schedule and checks the retired set against the float32 numpy criterion on the plain film's snapshots, then the
sums, the moments, the mean and the variance of the mean of every pixel against the snapshot at its own n_p, bit for bit.
"""
import os
import subprocess

import numpy as np
import pytest

import _util

pytestmark = pytest.mark.gpu

ENV_SWITCHES = ("SPT_NO_LDS_GEO", "SPT_STREAM_MASK", "SPT_PRIMARY_CHUNKS", "SPT_NO_EYE_BLOB")


@pytest.fixture(scope="module")
def spt():
    return _util.load_pkg()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _scene(spt, name):
    return spt.load_scene(os.path.join(_util.SCENES, name))


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


_criterion = _util.film_criterion   # spt_abi.h's retirement test in float32 (shared with tools/fuzz_sessions.py)


def _auto_rel(s, q, n, active):
    """A relative tolerance that retires about 40 % of the noisy active pixels at this snapshot."""
    m = s.astype(np.float64) / n
    v = np.maximum((q.astype(np.float64) / n - m * m) / (n - 1), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        need = np.max(np.sqrt(v) / np.abs(m), axis=-1)
    need = need[active & np.isfinite(need) & (need > 0)]
    return float(np.quantile(need, 0.4)) if need.size else 0.0


def _side_by_side(spt, r, sc, cfg, schedule, rel, floor=0.0, min_samples=8, **kw):
    """Renders `schedule` into an adaptive and a plain film; checks every step; returns (active count, counts) at the end."""
    with r.progressive(sc, cfg, moments=True, **kw) as ad, r.progressive(sc, cfg, moments=True, **kw) as plain:
        active = np.ones((ad.rows, ad.width), bool)
        n_p = np.zeros((ad.rows, ad.width), np.uint32)
        snaps = {}
        done, got = 0, ad.rows * ad.width
        for inc in schedule:
            ad.render(inc)
            plain.render(inc)
            done += inc
            assert ad.samples == done
            counts = ad.sample_counts()
            assert int((counts == done).sum()) == got        # the active pixels of the last adapt took every sample since
            s, q = plain.sum(), plain.sum_sq()
            snaps[done] = (s, q, plain.mean(), plain.variance_of_mean())
            rel_now = _auto_rel(s, q, done, active) if rel == "auto" else rel
            got = ad.adapt(rel_now, floor, min_samples)
            if done >= max(min_samples, 2):
                retire = active & _criterion(s, q, done, rel_now, floor)
                n_p[retire] = done
                active &= ~retire
            assert got == int(active.sum()), (done, got, int(active.sum()))
            counts = np.where(active, np.uint32(done), n_p)
            assert np.array_equal(ad.sample_counts(), counts), done
            for k, read in enumerate((ad.sum, ad.sum_sq, ad.mean, ad.variance_of_mean)):
                expect = np.empty_like(s)
                for n in np.unique(counts):
                    sel = counts == n
                    expect[sel] = snaps[int(n)][k][sel]
                assert _same(read(), expect), ("sum", "sum_sq", "mean", "variance_of_mean")[k] + " at %d samples" % done
        return got, counts


SCENES = [
    ("cfg2_cube.json", None, 64, 64),
    ("t_materials.json", "main", 64, 48),     # environment: retired pixels would otherwise still look it up
    ("t_textured.json", None, 64, 48),
    ("t_medium.json", None, 64, 48),
    ("t_bezier.json", "main", 48, 32),        # libspt_hip_bez.so: the adaptive calls are forwarded
]


@pytest.mark.parametrize("scene_name,camera,w,h", SCENES)
def test_adaptive_film_equals_plain_film_at_each_pixels_count(spt, scene_name, camera, w, h):
    sc = _scene(spt, scene_name)
    r = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RANDOM, spp=32, seed=5)
    cfg = spt.OutputConfig(w, h, None, camera)
    active, counts = _side_by_side(spt, r, sc, cfg, [4] * 8, "auto")
    n_pix = w * h
    assert 0 < active < n_pix, (scene_name, active)       # some retired, some not
    assert (counts < 32).any() and (counts == 32).any()
    sc.close()


@pytest.mark.parametrize("switch", [{"SPT_NO_LDS_GEO": "1"}, {"SPT_NO_LDS_GEO": "1", "SPT_STREAM_MASK": "7"},
                                    {"SPT_PRIMARY_CHUNKS": "1"}, {"SPT_NO_EYE_BLOB": "1"}, {}],
                         ids=["no_lds_geo", "primary_stream", "primary_chunks_1", "no_eye_blob", "shard_1_of_3"])
def test_adaptive_film_kernel_paths(spt, switch, monkeypatch):
    for k, v in switch.items():
        monkeypatch.setenv(k, v)
    kw = {} if switch else dict(shard_index=1, shard_count=3, strip_rows=8)
    for scene_name, camera in (("cfg2_cube.json", None), ("t_materials.json", "main")):
        sc = _scene(spt, scene_name)
        r = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RECURRENCE, spp=32, seed=9)
        active, _ = _side_by_side(spt, r, sc, spt.OutputConfig(72, 56, None, camera), [4] * 8, "auto", **kw)
        assert active > 0
        sc.close()


def test_fixed_tolerances(spt):
    sc = _scene(spt, "t_materials.json")
    r = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RANDOM, spp=24, seed=2)
    cfg = spt.OutputConfig(48, 40, None, "main")
    # 0 / 0: exactly the zero-variance pixels; a floor and min_samples below 2 (counts as 2); a schedule of uneven steps
    _side_by_side(spt, r, sc, cfg, [2, 2, 4, 8, 8], 0.0, 0.0, min_samples=0)
    _side_by_side(spt, r, sc, cfg, [1, 3, 4, 16], 0.05, 1e-3, min_samples=1)
    active, counts = _side_by_side(spt, r, sc, cfg, [6, 6, 6, 6], 1e9, 0.0, min_samples=12)   # everything at 12
    assert active == 0 and (counts == 12).all()
    sc.close()


def test_retired_film_stops_changing(spt):
    sc = _scene(spt, "cfg2_cube.json")
    r = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RANDOM, spp=32, seed=4)
    with r.progressive(sc, spt.OutputConfig(64, 48), moments=True) as film:
        film.render(8)
        assert film.adapt(1e30, 1e30, 2) == 0
        s, q, m = film.sum(), film.sum_sq(), film.mean()
        for _ in range(3):
            film.render(8)
            assert film.adapt(0.0) == 0
        assert film.samples == 32
        assert _same(film.sum(), s) and _same(film.sum_sq(), q) and _same(film.mean(), m)
        assert (film.sample_counts() == 8).all()
    sc.close()


def test_isolation(spt):
    """spt_render and a plain film on the same scene, interleaved with an adaptive film's increments, keep their bits."""
    sc = _scene(spt, "t_materials.json")
    r = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RANDOM, spp=16, seed=6)
    cfg = spt.OutputConfig(64, 48, None, "main")
    ref = r.render_shard(sc, cfg).copy()
    with r.progressive(sc, cfg) as alone:
        for _ in range(4):
            alone.render(4)
        ref_film = alone.mean()
    with r.progressive(sc, cfg, moments=True) as ad, r.progressive(sc, cfg) as plain:
        for _ in range(4):
            ad.render(4)
            assert _same(r.render_shard(sc, cfg), ref)
            plain.render(4)
            ad.adapt(0.2, 0.0, 4)
        assert _same(plain.mean(), ref_film)
        assert ad.sample_counts().min() < 16
    assert _same(r.render_shard(sc, cfg), ref)
    sc.close()


def test_refusals_leave_the_film_unchanged(spt):
    sc = _scene(spt, "cfg2_cube.json")
    r = spt.PathTracer(max_depth=4, sampler=spt.SAMPLER_RANDOM, spp=16, seed=1)
    cfg = spt.OutputConfig(48, 32)
    with r.progressive(sc, cfg) as film:                     # no moments
        film.render(4)
        with pytest.raises(spt.SptError) as e:
            film.adapt(0.1)
        assert e.value.status == 1
        assert (film.sample_counts() == 4).all()
    r_box = spt.PathTracer(max_depth=4, sampler=spt.SAMPLER_RANDOM, spp=16, seed=1, filter_radius=0.3)
    with r_box.progressive(sc, cfg, moments=True) as film:   # radius other than 0.5
        film.render(4)
        with pytest.raises(spt.SptError) as e:
            film.adapt(0.1, 0.0, 2)
        assert e.value.status == 4   # SPT_ERR_UNSUPPORTED
    with r.progressive(sc, cfg, moments=True) as film:
        film.render(4)
        s, q, m = film.sum(), film.sum_sq(), film.mean()
        for bad in ((-0.1, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (0.1, -1.0), (0.1, float("nan")), (0.1, float("inf"))):
            with pytest.raises(spt.SptError) as e:
                film.adapt(bad[0], bad[1], 2)
            assert e.value.status == 1, bad
        assert film.adapt(1e30, 1e30, 8) == 48 * 32              # done < min_samples: nothing retires
        film.render(4)
        assert (film.sample_counts() == 8).all()
        assert film.samples == 8
    with r.progressive(sc, cfg, moments=True) as film:
        film.render(4)
        s, q, m = film.sum(), film.sum_sq(), film.mean()
        for bad in ((-1.0, 0.0), (0.1, float("nan"))):
            with pytest.raises(spt.SptError):
                film.adapt(bad[0], bad[1], 2)
        assert _same(film.sum(), s) and _same(film.sum_sq(), q) and _same(film.mean(), m)
        assert (film.sample_counts() == 4).all() and film.samples == 4
    sc.close()


CLI_SCENE = ["-s", os.path.join(_util.SCENES, "cfg2_cube.json"), "-r", os.path.join(_util.SCENES, "pt.json")]


def test_cli_adaptive(spt, tmp_path):
    out, counts_path = tmp_path / "o.png", tmp_path / "n.exr"
    w, h, spp = 64, 48, 64
    args = CLI_SCENE + ["-w", str(w), "-h", str(h), "--spp", str(spp), "--seed", "2", "-o", str(out), "--adaptive", "0.08",
                        "--adaptive-floor", "0.002", "--adaptive-min-samples", "8", "--samples-out", str(counts_path)]
    res = subprocess.run([os.path.join(spt.LIB_DIR, "spt")] + args, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    line = [l for l in res.stderr.splitlines() if l.startswith("Rendered ")]
    assert line and "pixels active" in line[0], res.stderr
    sc = spt.load_scene(CLI_SCENE[1])
    ren = spt.load_renderer(CLI_SCENE[3], seed=2)
    ren.spp = spp
    with ren.progressive(sc, spt.OutputConfig(w, h), moments=True) as film:
        while film.samples < spp:                   # the CLI's schedule: increments of spp / 16, an adapt after each
            film.render(spp // 16)
            if film.adapt(0.08, 0.002, 8) == 0:
                break
        assert line[0].split()[1] == str(film.samples)
        counts = film.sample_counts()
        assert np.array_equal(spt.read_png(out)[..., :3], spt.film_to_rgb8(film.mean()))
    got = spt.read_exr(counts_path)
    assert np.array_equal(got, np.repeat(counts[..., None].astype(np.float32), 3, axis=-1))
    assert counts.min() < spp
    sc.close()
