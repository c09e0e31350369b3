"""Weighted reconstruction filters of sample-keeping films (spt_film_filter): tent, truncated Gaussian, Mitchell-Netravali.

The read-out under a filter is checked bit for bit against the float32 numpy restatement of the specification (tests/_filter_ref.py)
fed with the film's own kept() samples and the oracle's sample offsets; the rest checks that the read-out depends on nothing but the
kept samples: not on the increments, the passes, the shard, the plan's halo or the filters the film was read under before.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _filter_ref as ref
import _rgb8_values as V
import _util
from test_gpu_wide_film import SCHEDULES

pytestmark = pytest.mark.gpu

SAMPLERS = {"random": 0, "jittered": 1, "recurrence": 2}
INVALID = 1
THIRD = 1.0 / 3.0
FILTERS = {
    "tent1": ("tent", 1.0, {}),
    "gauss1p5": ("gaussian", 1.5, {"alpha": 2.0}),
    "mitchell2": ("mitchell", 2.0, {"b": THIRD, "c": THIRD}),
    "tent0p5": ("tent", 0.5, {}),                     # Rf = 0: the pixel's own samples, weighted
}


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


@pytest.fixture(scope="module")
def offsets(spt):
    """The oracle's offsets of the samples 5 .. 15 of a 32 x 24 image, seed 5, once per sampler and plan spp."""
    made = {}

    def get(sampler, spp, first, count):
        key = (sampler, spp, first, count)
        if key not in made:
            made[key] = ref.offsets(spt, 5, 32, 24, spp, SAMPLERS[sampler], first, count)
            made[key].setflags(write=False)
        return made[key]

    return get


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32), equal_nan=True)


def _tracer(spt, sampler, radius, kind="box", spp=16, seed=5, max_depth=6, **params):
    return spt.PathTracer(max_depth=max_depth, sampler=SAMPLERS[sampler], spp=spp, division_x=4, division_y=4, seed=seed, filter_radius=radius,
                          filter_type=kind, filter_params=params)


# ---- 1. against the restatement -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(FILTERS))
@pytest.mark.parametrize("sampler", ["random", "recurrence"])
def test_against_the_restatement(spt, scenes, offsets, sampler, name):
    kind, radius, params = FILTERS[name]
    sc = scenes("cfg1_sphere.json")
    w, h, first = 32, 24, 5
    r = _tracer(spt, sampler, radius, kind, **params)
    with r.progressive(sc, spt.OutputConfig(w, h), first_sample=first, keep_samples=True) as film:
        film.render(3)
        film.render(8)
        kept = film.kept()
        assert kept.shape == (11, h, w, 3)
        color, wsum, mean = ref.filter_film(kept, offsets(sampler, 16, first, 11), kind, radius, **params)
        got_sum, got_mean = film.sum(), film.mean()
        assert mean.max() > 0.1
        assert len(np.unique(wsum)) > 3                 # the weights really depend on the offsets
        assert _same(got_sum, color)
        assert _same(got_mean, mean)
        film.set_filter("box")
        assert not _same(film.mean(), got_mean)         # the box of the same film is another image


# ---- 2. increments and passes do not matter -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("sampler", ["random", "jittered", "recurrence"])
def test_increments_and_passes_do_not_matter(spt, scenes, sampler):
    sc = scenes("cfg1_sphere.json")
    r = _tracer(spt, sampler, 1.5, "gaussian", seed=7, alpha=2.0)
    cfg = spt.OutputConfig(64, 48)

    def mean(schedule, **kw):
        with r.progressive(sc, cfg, keep_samples=True, **kw) as film:
            for n in schedule:
                film.render(n)
            assert film.samples == 16
            return film.mean()

    want = mean([16])
    assert np.nanmax(want) > 0.1 and np.isfinite(want).all()
    for name, schedule in SCHEDULES.items():
        assert _same(mean(schedule), want), "schedule %s differs" % name
    for schedule in ([16], [3, 7, 5, 1]):               # samples_per_pass 5: an increment spans several chunks
        assert _same(mean(schedule, samples_per_pass=5), want), ("samples_per_pass 5", schedule)


# ---- 3. read-only -------------------------------------------------------------------------------------------------------------------

def test_filters_only_read(spt, scenes):
    sc = scenes("cfg1_sphere.json")
    cfg = spt.OutputConfig(40, 30)
    wide = _tracer(spt, "random", 2.2, spp=8)
    with wide.progressive(sc, cfg, keep_samples=True) as film:
        film.render(3)
        film.render(5)
        kept, box = film.kept(), film.mean()
        assert _same(box, wide.render_shard(sc, cfg))
        film.set_filter("tent", radius=1.0)
        tent = film.mean()
        assert not _same(tent, box) and tent.max() > 0.1
        film.set_filter("box")
        assert _same(film.mean(), box) and _same(film.kept(), kept) and film.samples == 8
        film.set_filter("tent", radius=1.0)
        assert _same(film.mean(), tent)
    # the same tent on a film whose plan stores one halo row instead of two: every copy of a row has the same bits
    narrow = _tracer(spt, "random", 1.0, "tent", spp=8)
    with narrow.progressive(sc, cfg, keep_samples=True) as film:
        film.render(8)
        assert _same(film.mean(), tent)


# ---- 4. shards ----------------------------------------------------------------------------------------------------------------------

def test_shards(spt, scenes):
    sc = scenes("cfg1_sphere.json")
    h, shard_count, strip_rows = 50, 3, 4               # no multiple of the strips
    r = _tracer(spt, "random", 2.0, "mitchell", spp=8, max_depth=5, b=THIRD, c=THIRD)
    cfg = spt.OutputConfig(40, h)
    with r.progressive(sc, cfg, keep_samples=True) as film:
        full = film.render(8).mean()
    assert _same(full, r.render_shard(sc, cfg))         # render_shard goes through such a film too
    covered = np.zeros(h, dtype=bool)
    for k in range(shard_count):
        kw = dict(shard_index=k, shard_count=shard_count, strip_rows=strip_rows)
        with r.progressive(sc, cfg, keep_samples=True, **kw) as film:
            film.render(3)
            film.render(5)
            got = film.mean()
        rows = spt.shard_rows(h, k, shard_count, strip_rows)
        assert _same(got, full[rows]), k
        covered[rows] = True
    assert covered.all() and full.max() > 0.1


# ---- 5. forwarding ------------------------------------------------------------------------------------------------------------------

def test_forwarded_to_the_bezier_library(spt, scenes):
    sc = scenes("t_bezier.json")
    w, h = 32, 24
    r = _tracer(spt, "random", 1.0, "tent", spp=4)
    with r.progressive(sc, spt.OutputConfig(w, h, None, "main"), keep_samples=True) as film:
        film.render(4)
        off = ref.offsets(spt, 5, w, h, 4, SAMPLERS["random"], 0, 4)
        color, wsum, mean = ref.filter_film(film.kept(), off, "tent", 1.0)
        assert mean.max() > 0.1
        assert _same(film.sum(), color) and _same(film.mean(), mean)


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_film_and_its_filter_unchanged(spt, scenes):
    sc = scenes("cfg2_cube.json")
    cfg = spt.OutputConfig(48, 32)
    lib = spt.hip_lib()
    D = spt.FilterDesc
    nan, inf = float("nan"), float("inf")
    good = spt.filter_desc("tent", 1.0)
    assert lib.spt_film_filter(None, C.byref(good)) == INVALID
    plain = _tracer(spt, "random", 0.5, spp=8, seed=1, max_depth=4)
    with plain.progressive(sc, cfg) as film:            # a film without SPT_FILM_KEEP_SAMPLES
        film.render(2)
        before = film.mean()
        for desc in (spt.filter_desc("tent", 0.5), spt.filter_desc("box")):
            assert lib.spt_film_filter(film._handle(), C.byref(desc)) == INVALID
        assert "KEEP_SAMPLES" in lib.spt_last_error().decode()
        assert _same(film.mean(), before)
    with pytest.raises(spt.SptError):
        _tracer(spt, "random", 1.0, "tent", spp=8).progressive(sc, cfg)          # the binding: a weighted filter needs keep_samples
    wide = _tracer(spt, "random", 1.0, spp=8, seed=1, max_depth=4)
    with wide.progressive(sc, cfg, first_sample=2, keep_samples=True) as film:
        film.render(3)
        film.set_filter("gaussian", radius=1.2, alpha=1.5)
        samples, mean, kept = film.samples, film.mean(), film.kept()
        refused = [
            None,                                                   # a null desc
            D(20, 1, 1.0, 0.0, 0.0, 0),                             # size below the struct's
            D(0, 1, 1.0, 0.0, 0.0, 0),
            D(24, 4, 1.0, 0.0, 0.0, 0),                             # an unknown type
            D(24, 0xffffffff, 1.0, 0.0, 0.0, 0),
            D(24, 1, nan, 0.0, 0.0, 0), D(24, 1, inf, 0.0, 0.0, 0), D(24, 1, 0.0, 0.0, 0.0, 0), D(24, 1, -1.0, 0.0, 0.0, 0),
            D(24, 2, nan, 2.0, 0.0, 0), D(24, 3, -0.5, THIRD, THIRD, 0),
            D(24, 1, 1.6, 0.0, 0.0, 0),                             # Rf = 2, the film stores one halo row
            D(24, 3, 2.0, THIRD, THIRD, 0), D(24, 1, 1e30, 0.0, 0.0, 0),
            D(24, 2, 1.0, 0.0, 0.0, 0), D(24, 2, 1.0, -2.0, 0.0, 0), D(24, 2, 1.0, nan, 0.0, 0), D(24, 2, 1.0, inf, 0.0, 0),   # alpha
            D(24, 3, 1.0, nan, THIRD, 0), D(24, 3, 1.0, THIRD, inf, 0), D(24, 3, 1.0, -inf, THIRD, 0),                          # B, C
        ]
        for desc in refused:
            what = None if desc is None else (desc.size, desc.type, desc.radius, desc.p0, desc.p1)
            assert lib.spt_film_filter(film._handle(), None if desc is None else C.byref(desc)) == INVALID, what
            assert len(lib.spt_last_error()) > 0
            if what == (24, 1, np.float32(1.6), 0.0, 0.0):
                assert "1.6" in lib.spt_last_error().decode()       # the plan radius that would do
            assert film.samples == samples and _same(film.mean(), mean) and _same(film.kept(), kept), what
        with pytest.raises(spt.SptError) as e:
            film.set_filter("mitchell")                             # radius 2 by default
        assert e.value.status == INVALID and _same(film.mean(), mean)
        film.set_filter("box")                                      # radius, p0 and p1 are ignored for the box
        box = film.mean()
        assert not _same(box, mean)
        assert lib.spt_film_filter(film._handle(), C.byref(D(24, 0, nan, nan, nan, 7))) == 0 and _same(film.mean(), box)
    md = spt.MultiDevice(sc, [0, 0])
    try:
        with pytest.raises(spt.SptError):
            md.progressive(_tracer(spt, "random", 1.0, "tent", spp=8), cfg, strip_rows=4, keep_samples=True)
    finally:
        md.close()


# ---- 7. RGB8 ------------------------------------------------------------------------------------------------------------------------

def test_rgb8(spt, scenes):
    sc = scenes("cfg2_cube.json")
    r = _tracer(spt, "random", 1.5, "gaussian", spp=12, seed=9, max_depth=5, alpha=2.0)
    with r.progressive(sc, spt.OutputConfig(48, 32), keep_samples=True) as film:
        film.render(5)
        film.render(7)
        mean = film.mean()
        got = film.read_rgb8("mean")
        assert np.array_equal(got, V.rgb8_numpy(mean).reshape(mean.shape))
        assert got.max() > 25
        film.set_filter("box")
        assert not np.array_equal(film.read_rgb8("mean"), got)


# ---- 8. CLI -------------------------------------------------------------------------------------------------------------------------

def test_cli(spt, tmp_path):
    renderer = tmp_path / "pt_gauss.json"
    renderer.write_text('{"type": "pt", "max_depth": 5, "sampler": {"type": "random", "spp": 8}, "filter": {"type": "gaussian", "radius": 1.5}}')
    scene = os.path.join(_util.SCENES, "cfg2_cube.json")
    exe = os.path.join(spt.LIB_DIR, "spt")
    args = [exe, "-s", scene, "-r", str(renderer), "-w", "48", "-h", "32", "--seed", "3"]
    plain, preview = tmp_path / "plain.png", tmp_path / "preview.png"
    for out, extra in ((plain, []), (preview, ["--preview-every", "3"])):
        res = subprocess.run(args + ["-o", str(out)] + extra, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr
    ren = spt.load_renderer(str(renderer), seed=3)
    assert (ren.filter_type, ren.filter_radius, ren.filter_params) == ("gaussian", 1.5, {"alpha": 2.0})
    sc = spt.load_scene(scene)
    with ren.progressive(sc, spt.OutputConfig(48, 32), keep_samples=True) as film:
        want = film.render(8).read_rgb8("mean")
    sc.close()
    assert want.max() > 25
    assert np.array_equal(spt.read_png(str(plain))[..., :3], want)
    expected = tmp_path / "want.png"
    spt.write_png(str(expected), want)
    assert plain.read_bytes() == expected.read_bytes() == preview.read_bytes()
    for extra in (["--film-devices", "0,0"], ["--preview-every", "3", "--film-devices", "0,0"], ["--denoise"], ["--robust", "5"],
                  ["--variance-out", str(tmp_path / "v.exr")], ["--adaptive", "0.05"], ["--samples-out", str(tmp_path / "n.exr")]):
        out = tmp_path / "refused.png"
        res = subprocess.run(args + ["-o", str(out)] + extra, capture_output=True, text=True, timeout=300)
        assert res.returncode == 2, (extra, res.stderr)
        assert "weighted" in res.stderr and not out.exists()          # the refusal that names the cause, whatever else is missing
