"""The overlapped schedule of asynchronous renders: tail launch, resolve, finish and copy-out of pass p on the scene's film
stream next to pass p + 1's k_primary on the main stream, from two sets of pass buffers.

Every film is compared bit for bit with the synchronous render_shard of the same parameters - that call returns stats, so it
stays on the single-stream path - and, on cfg2_cube, with the oracle.  The expected films come from a scene object of their
own, so that the scene under test only sees the calls a case lists."""
import functools
import os

import numpy as np
import pytest

import _util

pytestmark = pytest.mark.gpu

spt = _util.load_pkg()

SWITCHES = ("SPT_NO_FILM_STREAM", "SPT_NO_TAIL_LOOP", "SPT_NO_FUSED", "SPT_PRIMARY_CHUNKS")
CUBE, MATERIALS = "cfg2_cube.json", "t_materials.json"


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


@functools.lru_cache(maxsize=None)
def _reference_scene(name):
    return spt.load_scene(os.path.join(_util.SCENES, name))


def _tracer(sampler, spp, seed):
    return spt.PathTracer(max_depth=8, sampler=sampler, spp=spp, seed=seed)


@functools.lru_cache(maxsize=None)
def _expected(name, cam, w, h, sampler, spp, spp_pass, seed):
    """The synchronous film (read-only); for the cube it is checked against the oracle's bits once, here."""
    scene = _reference_scene(name)
    r = _tracer(sampler, spp, seed)
    film = r.render_shard(scene, spt.OutputConfig(w, h, None, cam), samples_per_pass=spp_pass).copy()
    if name == CUBE:
        ref, _ = _util.oracle_render(scene, r, w, h, camera=cam, flags=_util.device_oracle_flags())
        assert np.array_equal(film.view(np.uint32), ref.view(np.uint32)), "the synchronous film differs from the oracle"
    film.setflags(write=False)
    return film


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _fresh(name):
    return spt.load_scene(os.path.join(_util.SCENES, name))


def _many_passes(sampler):
    """Case 1: 96 x 80, depth 8, 24 spp in six passes of 4 (each buffer set three times), three frames queued back to back."""
    w, h, spp, spp_pass, seeds = 96, 80, 24, 4, (11, 12, 13)
    cfg = spt.OutputConfig(w, h)
    want = [_expected(CUBE, None, w, h, sampler, spp, spp_pass, s) for s in seeds]
    scene = _fresh(CUBE)
    try:
        ds = scene.device_scene(0)
        r = _tracer(sampler, spp, seeds[0])
        before = ds.render_info(0)
        for s in seeds:
            r.seed = s
            out = r.render_shard(scene, cfg, samples_per_pass=spp_pass, reuse_output=True, wait=False)
        r.wait(scene)
        assert _same(out, want[-1])
        queued = ds.render_info(0) - before
        films = [np.zeros((h, w, 3), dtype=np.float32) for _ in seeds]
        for s, film in zip(seeds, films):
            r.seed = s
            r.render_shard(scene, cfg, samples_per_pass=spp_pass, film=film, wait=False)
        r.wait(scene)
        for k, film in enumerate(films):
            assert _same(film, want[k]), "frame %d of three" % k
        return queued
    finally:
        scene.close()


@pytest.mark.parametrize("sampler", [spt.SAMPLER_RECURRENCE, spt.SAMPLER_RANDOM], ids=["recurrence", "random"])
def test_many_passes_reuse_both_buffer_sets(sampler):
    assert _many_passes(sampler) == 3 * 6


@pytest.mark.parametrize("switch", [None, "SPT_NO_TAIL_LOOP", "SPT_NO_FUSED"], ids=["default", "no-tail-loop", "no-fused"])
def test_both_bounce_schedules_on_a_fresh_scene(monkeypatch, switch):
    """Case 2: without the tail-loop hint every bounce is a launch on the main stream; after one synchronous render the hint
    exists and the tail-loop kernel runs on the film stream (unless the switch forbids it)."""
    w, h, spp, spp_pass = 96, 80, 24, 4
    cfg = spt.OutputConfig(w, h)
    want = [_expected(CUBE, None, w, h, spt.SAMPLER_RECURRENCE, spp, spp_pass, s) for s in (21, 22)]
    if switch:
        monkeypatch.setenv(switch, "1")
    scene = _fresh(CUBE)
    try:
        r = _tracer(spt.SAMPLER_RECURRENCE, spp, 21)
        films = [np.zeros((h, w, 3), dtype=np.float32) for _ in range(4)]
        for k in (0, 1):                       # no hint yet
            r.seed = 21 + k
            r.render_shard(scene, cfg, samples_per_pass=spp_pass, film=films[k], wait=False)
        r.wait(scene)
        r.seed = 21
        sync = r.render_shard(scene, cfg, samples_per_pass=spp_pass)      # leaves the hint
        for k in (0, 1):
            r.seed = 21 + k
            r.render_shard(scene, cfg, samples_per_pass=spp_pass, film=films[2 + k], wait=False)
        r.wait(scene)
        assert _same(sync, want[0])
        for k, film in enumerate(films):
            assert _same(film, want[k & 1]), "film %d" % k
    finally:
        scene.close()


def test_unfused_pipeline_with_a_short_last_pass():
    """Case 3: t_materials (general shade kernels, shadow rays on the side stream), 12 spp in passes of 5, 5 and 2."""
    w, h, spp, spp_pass = 64, 48, 12, 5
    cfg = spt.OutputConfig(w, h, None, "main")
    want = [_expected(MATERIALS, "main", w, h, spt.SAMPLER_RECURRENCE, spp, spp_pass, s) for s in (5, 6)]
    scene = _fresh(MATERIALS)
    try:
        ds = scene.device_scene(0)
        r = _tracer(spt.SAMPLER_RECURRENCE, spp, 5)
        films = [np.zeros((h, w, 3), dtype=np.float32) for _ in range(3)]
        for k, film in enumerate(films):
            r.seed = 5 + (k & 1)
            r.render_shard(scene, cfg, samples_per_pass=spp_pass, film=film, wait=False)
        r.wait(scene)
        assert ds.render_info(0) == 3 * 3
        for k, film in enumerate(films):
            assert _same(film, want[k & 1]), "film %d" % k
    finally:
        scene.close()


def test_unchunked_primary_inside_an_overlapped_render(monkeypatch):
    """Case 4: SPT_PRIMARY_CHUNKS=1 makes k_primary add into the film itself, behind the film stream's memset and resolves."""
    monkeypatch.setenv("SPT_PRIMARY_CHUNKS", "1")
    assert _many_passes(spt.SAMPLER_RECURRENCE) == 3 * 6


def test_workspace_growth_in_flight():
    """Case 5: three sizes queued without a wait between them; the third outgrows the workspace the first two are using."""
    sizes, spp, spp_pass = ((96, 80), (64, 48), (128, 96)), 24, 4
    want = [_expected(CUBE, None, w, h, spt.SAMPLER_RECURRENCE, spp, spp_pass, 31 + k) for k, (w, h) in enumerate(sizes)]
    scene = _fresh(CUBE)
    try:
        r = _tracer(spt.SAMPLER_RECURRENCE, spp, 31)
        films = [np.zeros((h, w, 3), dtype=np.float32) for w, h in sizes]
        for k, (w, h) in enumerate(sizes):
            r.seed = 31 + k
            r.render_shard(scene, spt.OutputConfig(w, h), samples_per_pass=spp_pass, film=films[k], wait=False)
        r.wait(scene)
        for k, film in enumerate(films):
            assert _same(film, want[k]), "size %d x %d" % sizes[k]
    finally:
        scene.close()


def test_shards_into_one_strided_film():
    """Case 6: three shards of 16-row strips, queued one after the other into one full-image film."""
    w, h, spp, spp_pass = 96, 80, 24, 4
    want = _expected(CUBE, None, w, h, spt.SAMPLER_RECURRENCE, spp, spp_pass, 11)
    scene = _fresh(CUBE)
    try:
        r = _tracer(spt.SAMPLER_RECURRENCE, spp, 11)
        film = np.zeros((h, w, 3), dtype=np.float32)
        for k in range(3):
            r.render_shard(scene, spt.OutputConfig(w, h), shard_index=k, shard_count=3, strip_rows=16, samples_per_pass=spp_pass, film=film,
                           wait=False)
        r.wait(scene)
        assert _same(film, want)
    finally:
        scene.close()


def test_the_seam_counts_where_passes_were_resolved(monkeypatch):
    """Case 7: spt_debug_render_info.  Counter 0 grows by the passes of an overlapped render only; the switch and a synchronous
    render grow counter 1 instead."""
    w, h, spp, spp_pass = 96, 80, 24, 4
    cfg = spt.OutputConfig(w, h)
    want = _expected(CUBE, None, w, h, spt.SAMPLER_RECURRENCE, spp, spp_pass, 11)
    scene = _fresh(CUBE)
    try:
        ds = scene.device_scene(0)
        r = _tracer(spt.SAMPLER_RECURRENCE, spp, 11)
        assert (ds.render_info(0), ds.render_info(1)) == (0, 0)
        out = r.render_shard(scene, cfg, samples_per_pass=spp_pass, reuse_output=True)            # synchronous
        assert (ds.render_info(0), ds.render_info(1)) == (0, 6)
        r.render_shard(scene, cfg, samples_per_pass=spp_pass, reuse_output=True, wait=False)
        assert (ds.render_info(0), ds.render_info(1)) == (6, 6)
        monkeypatch.setenv("SPT_NO_FILM_STREAM", "1")
        r.render_shard(scene, cfg, samples_per_pass=spp_pass, reuse_output=True, wait=False)      # behind the overlapped frame
        assert (ds.render_info(0), ds.render_info(1)) == (6, 12)
        monkeypatch.delenv("SPT_NO_FILM_STREAM")
        r.render_shard(scene, cfg, samples_per_pass=spp_pass, reuse_output=True, wait=False)      # and overlapped again
        r.wait(scene)
        assert (ds.render_info(0), ds.render_info(1)) == (12, 12)
        assert _same(out, want)
    finally:
        scene.close()
