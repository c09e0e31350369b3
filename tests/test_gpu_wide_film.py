"""Films that keep their samples (SPT_FILM_KEEP_SAMPLES): progressive rendering under box filters that reach neighbouring pixels.

Such a film owns the radiance of every covered sample of its stored rows (own rows + R halo rows) and reads out
Film::filter_pixel over them, so the mean after increments that cover the plan has the bits of one spt_render at any radius;
partial films are checked against the float32 numpy restatement of the specification (tests/_wide_film_ref.py) fed with the
film's own kept() samples and the oracle's sample offsets.
"""
import os
import subprocess

import numpy as np
import pytest

import _rgb8_values as V
import _util
import _wide_film_ref as ref

pytestmark = pytest.mark.gpu

SAMPLERS = {"random": 0, "jittered": 1, "recurrence": 2}
SCHEDULES = {"whole": [16], "ones": [1] * 5 + [11], "odd": [3, 7, 5, 1], "quarters": [4] * 4}
INVALID, UNSUPPORTED = 1, 4


@pytest.fixture(scope="module")
def spt():
    pkg = _util.load_pkg()
    _util.ensure_cpu_build()
    return pkg


@pytest.fixture(scope="module")
def scenes(spt):
    """Every scene once for the module."""
    loaded = {}

    def get(name):
        if name not in loaded:
            loaded[name] = spt.load_scene(os.path.join(_util.SCENES, name))
        return loaded[name]

    yield get
    for sc in loaded.values():
        sc.close()


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32), equal_nan=True)


def _mean(r, sc, cfg, schedule, **kw):
    with r.progressive(sc, cfg, keep_samples=True, **kw) as film:
        for n in schedule:
            film.render(n)
        assert film.samples == sum(schedule)
        return film.mean()


# ---- 1. increments equal one call ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("radius", [1.0, 1.5, 2.2])
@pytest.mark.parametrize("sampler", ["random", "jittered", "recurrence"])
@pytest.mark.parametrize("scene_name,camera", [
    ("cfg1_sphere.json", None),
    ("t_materials.json", "main"),     # environment: the chunked primary kernel
    ("t_bezier.json", "main"),        # libspt_hip_bez.so: the film calls are forwarded
])
def test_increments_equal_one_call(spt, scenes, scene_name, camera, sampler, radius):
    sc = scenes(scene_name)
    r = spt.PathTracer(max_depth=6, sampler=SAMPLERS[sampler], spp=16, division_x=4, division_y=4, seed=7, filter_radius=radius)
    cfg = spt.OutputConfig(64, 48, None, camera)
    want = r.render_shard(sc, cfg).copy()
    assert np.nanmax(want) > 0.1
    for name, schedule in SCHEDULES.items():
        assert _same(_mean(r, sc, cfg, schedule), want), "%s: schedule %s differs from one call" % (scene_name, name)
    for schedule in ([16], [3, 7, 5, 1]):          # samples_per_pass 5: an increment spans several chunks
        assert _same(_mean(r, sc, cfg, schedule, samples_per_pass=5), want), (scene_name, "samples_per_pass 5", schedule)


# ---- 2. the flag at R <= 0 -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("radius", [0.5, 0.3, -0.75])
def test_flag_within_one_pixel(spt, scenes, radius):
    sc = scenes("cfg1_sphere.json")
    r = spt.PathTracer(max_depth=6, sampler=spt.SAMPLER_RANDOM, spp=16, seed=7, filter_radius=radius)
    cfg = spt.OutputConfig(64, 48)
    want = r.render_shard(sc, cfg).copy()
    with r.progressive(sc, cfg, keep_samples=True) as film:
        for n in (3, 7, 5, 1):
            film.render(n)
        assert _same(film.mean(), want)
        if radius == 0.5:
            with r.progressive(sc, cfg) as plain:
                plain.render(16)
                assert _same(film.mean(), plain.mean()) and _same(film.sum(), plain.sum())
            assert want.max() > 0.1
    if radius == -0.75:
        assert np.isnan(want).all()                 # both loops empty: 0 * (1 / 0)


# ---- 3. shards -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shard_count,strip_rows", [(3, 4), (2, 1)])
def test_shards_trace_their_own_halo(spt, scenes, shard_count, strip_rows):
    sc = scenes("cfg1_sphere.json")
    h = 50                                          # no multiple of the strips
    r = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RANDOM, spp=8, seed=5, filter_radius=2.2)
    cfg = spt.OutputConfig(40, h)
    full = r.render_shard(sc, cfg).copy()
    covered = np.zeros(h, dtype=bool)
    for k in range(shard_count):
        kw = dict(shard_index=k, shard_count=shard_count, strip_rows=strip_rows)
        want = r.render_shard(sc, cfg, **kw).copy()
        got = _mean(r, sc, cfg, [3, 5], **kw)
        rows = spt.shard_rows(h, k, shard_count, strip_rows)
        assert _same(got, want), (shard_count, strip_rows, k)
        assert _same(got, full[rows]), (shard_count, strip_rows, k)
        covered[rows] = True
    assert covered.all() and full.max() > 0.1


# ---- 4. prefixes and first_sample -------------------------------------------------------------------------------------------------

def test_a_prefix_of_a_random_plan(spt, scenes):
    sc = scenes("cfg1_sphere.json")
    cfg = spt.OutputConfig(64, 48)
    plan = spt.PathTracer(max_depth=6, sampler=spt.SAMPLER_RANDOM, spp=64, seed=5, filter_radius=1.0)
    short = spt.PathTracer(max_depth=6, sampler=spt.SAMPLER_RANDOM, spp=16, seed=5, filter_radius=1.0)
    with plan.progressive(sc, cfg, keep_samples=True) as film:
        film.render(16)
        assert _same(film.mean(), short.render_shard(sc, cfg))     # the random sampler does not read the plan's spp


@pytest.mark.parametrize("radius,sampler", [(1.0, "random"), (1.0, "recurrence"), (1.5, "random")])
def test_first_sample_against_the_restatement(spt, scenes, radius, sampler):
    sc = scenes("cfg1_sphere.json")
    w, h, seed, first = 32, 24, 5, 5
    r = spt.PathTracer(max_depth=6, sampler=SAMPLERS[sampler], spp=16, seed=seed, filter_radius=radius)
    with r.progressive(sc, spt.OutputConfig(w, h), first_sample=first, keep_samples=True) as film:
        film.render(3)
        film.render(8)
        kept = film.kept()
        assert kept.shape == (11, h, w, 3)
        off = ref.offsets(spt, seed, w, h, 16, SAMPLERS[sampler], first, 11)
        color, wsum, mean = ref.filter_film(kept, off, radius)
        if radius == 1.0:
            assert len(np.unique(wsum)) > 3        # the weights really depend on the offsets
        assert mean.max() > 0.1
        assert _same(film.sum(), color)
        assert _same(film.mean(), mean)


# ---- 5. kept() -------------------------------------------------------------------------------------------------------------------

def test_kept_samples_add_up_to_the_sum(spt, scenes):
    sc = scenes("t_materials.json")
    r = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RANDOM, spp=12, seed=11)
    cfg = spt.OutputConfig(48, 32, None, "main")
    with r.progressive(sc, cfg, first_sample=2, keep_samples=True, samples_per_pass=4) as film, r.progressive(sc, cfg, first_sample=2) as plain:
        for n in (1, 6, 3):
            film.render(n)
            plain.render(n)
        kept = film.kept()
        assert kept.shape == (10, 32, 48, 3) and kept.dtype == np.float32
        s = np.zeros((32, 48, 3), dtype=np.float32)
        for x in kept:
            s = s + x
        assert _same(film.sum(), s) and _same(plain.sum(), s)
        assert s.max() > 0.1
        for first, count in ((2, 1), (4, 5), (11, 1), (7, 0)):
            assert _same(film.kept(first, count), kept[first - 2:first - 2 + count]), (first, count)
        assert _same(film.kept(first=6), kept[4:])
    black = spt.PathTracer(max_depth=0, sampler=spt.SAMPLER_RANDOM, spp=4, seed=11, filter_radius=1.0)
    with black.progressive(sc, cfg, keep_samples=True) as film:
        film.render(3)
        assert film.kept().shape == (3, 32, 48, 3) and not film.kept().any()
        assert not film.sum().any()


# ---- 6. isolation ----------------------------------------------------------------------------------------------------------------

def test_films_are_isolated(spt, scenes):
    sc = scenes("t_materials.json")
    ra = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RANDOM, spp=12, seed=2, filter_radius=1.5)
    rb = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RECURRENCE, spp=9, seed=4)
    ca, cb = spt.OutputConfig(64, 48, None, "main"), spt.OutputConfig(40, 56, None, "top")
    ref_a, ref_b = ra.render_shard(sc, ca).copy(), rb.render_shard(sc, cb).copy()
    rc = spt.PathTracer(max_depth=4, sampler=spt.SAMPLER_RANDOM, spp=6, seed=9)
    cc = spt.OutputConfig(80, 64, None, "main")
    ref_c = rc.render_shard(sc, cc).copy()
    fa, fb = ra.progressive(sc, ca, keep_samples=True), rb.progressive(sc, cb)
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


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_film_unchanged(spt, scenes):
    sc = scenes("cfg2_cube.json")
    cfg = spt.OutputConfig(48, 32)
    wide = spt.PathTracer(max_depth=4, sampler=spt.SAMPLER_RANDOM, spp=8, seed=1, filter_radius=1.0)
    with pytest.raises(spt.SptError) as e:
        wide.progressive(sc, cfg)                                   # without the flag: as before
    assert e.value.status == UNSUPPORTED
    with pytest.raises(spt.SptError) as e:
        wide.progressive(sc, cfg, moments=True, keep_samples=True)
    assert e.value.status == INVALID
    lib = spt.hip_lib()
    spare = np.zeros(48 * 32 * 3 * 8, dtype=np.float32)
    assert lib.spt_film_read_samples(None, 0, 1, spare.ctypes.data) == INVALID
    plain = spt.PathTracer(max_depth=4, sampler=spt.SAMPLER_RANDOM, spp=8, seed=1)
    with plain.progressive(sc, cfg) as film:
        film.render(2)
        with pytest.raises(spt.SptError) as e:
            film.kept()                                             # a film without the flag
        assert e.value.status == INVALID
    with wide.progressive(sc, cfg, first_sample=2, keep_samples=True) as film:
        film.render(3)
        samples, mean, kept = film.samples, film.mean(), film.kept()

        def unchanged():
            return film.samples == samples and _same(film.mean(), mean) and _same(film.kept(), kept)

        assert lib.spt_film_read_samples(film._handle(), 2, 1, None) == INVALID and unchanged()
        assert lib.spt_film_read_samples(film._handle(), 4, 0xffffffff, spare.ctypes.data) == INVALID and unchanged()   # first + count wraps in 32 bits
        for first, count in ((1, 2), (2, 4), (5, 1), (0, 0)):       # outside [2, 5)
            with pytest.raises(spt.SptError) as e:
                film.kept(first, count)
            assert e.value.status == INVALID and unchanged(), (first, count)
        assert film.kept(5, 0).shape == (0, 32, 48, 3)              # an empty range at the end is inside
        refused = [lambda: film.set_buckets(5), lambda: film.adapt(0.05), lambda: film.denoise(), lambda: film.sum_sq(),
                   lambda: film.variance_of_mean(), lambda: film.robust_mean("mon"), lambda: film.render(4)]   # the last: 3 + 4 > 8 - 2
        for call in refused:
            with pytest.raises(spt.SptError) as e:
                call()
            assert e.value.status == INVALID and unchanged()
        film.render(3)
        assert film.samples == 6 and _same(film.kept(2, 3), kept)
    # more than 2^31 - 1 stored pixels: the own rows fit, the halo rows of the two runs do not (nothing is allocated for the check)
    huge = spt.PathTracer(max_depth=1, sampler=spt.SAMPLER_RANDOM, spp=1, seed=1, filter_radius=2.2)
    with pytest.raises(spt.SptError) as e:
        huge.progressive(sc, spt.OutputConfig(65536, 49150), shard_index=0, shard_count=2, strip_rows=16384, keep_samples=True)
    assert e.value.status == UNSUPPORTED and "stored" in e.value.message


# (8. the in-box count table was measured no faster than deriving the offsets again and deleted: nothing to compare)


# ---- 9. RGB8 and several devices -------------------------------------------------------------------------------------------------

def test_rgb8_and_two_workers(spt, scenes):
    sc = scenes("cfg2_cube.json")
    r = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RANDOM, spp=12, seed=9, filter_radius=1.0)
    cfg = spt.OutputConfig(48, 32)
    single = r.render_shard(sc, cfg).copy()
    with r.progressive(sc, cfg, keep_samples=True) as film:
        film.render(5)
        mean = film.mean()
        assert np.array_equal(film.read_rgb8("mean"), V.rgb8_numpy(mean).reshape(mean.shape))
        film.render(7)
        assert np.array_equal(film.read_rgb8("mean"), V.rgb8_numpy(single).reshape(single.shape))
        assert film.read_rgb8("mean").max() > 25
    md = spt.MultiDevice(sc, [0, 0])
    try:
        multi = md.progressive(r, cfg, strip_rows=4, keep_samples=True)
        multi.render(5)
        multi.render(7)
        assert _same(multi.mean(), single)
        assert np.array_equal(multi.read_rgb8("mean"), V.rgb8_numpy(single).reshape(single.shape))
    finally:
        md.close()


# ---- 10. CLI ---------------------------------------------------------------------------------------------------------------------

def test_cli_previews_under_a_wide_radius(spt, tmp_path):
    renderer = tmp_path / "pt_wide.json"
    renderer.write_text('{"type": "pt", "max_depth": 5, "sampler": {"type": "random", "spp": 12}, "filter": {"type": "box", "radius": 1.0}}')
    exe = os.path.join(spt.LIB_DIR, "spt")
    args = [exe, "-s", os.path.join(_util.SCENES, "cfg2_cube.json"), "-r", str(renderer), "-w", "48", "-h", "32", "--seed", "3"]
    plain, preview, devices = tmp_path / "plain.png", tmp_path / "preview.png", tmp_path / "devices.png"
    for out, extra in ((plain, []), (preview, ["--preview-every", "4"]), (devices, ["--preview-every", "4", "--film-devices", "0,0"])):
        res = subprocess.run(args + ["-o", str(out)] + extra, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr
    assert len(plain.read_bytes()) > 100
    assert plain.read_bytes() == preview.read_bytes() == devices.read_bytes()
    res = subprocess.run(args + ["-o", str(tmp_path / "dn.png"), "--denoise"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 2, res.stderr
    assert "radius 1" in res.stderr and len(res.stderr.strip().splitlines()[-1]) > 0
    assert not (tmp_path / "dn.png").exists()                       # refused before any sample was traced
