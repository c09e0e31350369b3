"""The pass pipeline of overlapped renders: the bounce launches of pass p on the scene's second stream beside
k_primary of pass p + 1 on the main stream, from two sets of path and hit queues; tail launch, resolve and finish on the film stream.

96 x 64 pixels (6 x 4 tiles, the cube crosses tile edges), cfg2_cube.json, pt.json (depth 8, recurrence sampler) unless a case says
otherwise.  Every film under test is rendered asynchronously (wait=False, then wait) and compared bit for bit with the film of
SPT_NO_PASS_PIPELINE=1 and with the synchronous render, which returns stats and so stays on the main stream; the expected films come
from scene objects of their own.  spt_debug_render_info counter 7 says whether the passes took the pipeline: no case passes without it."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import _scene_update_scenes as S
import _util
import test_gpu_origin_candidates as OC

pytestmark = pytest.mark.gpu

spt = _util.load_pkg()
f32 = np.float32

W, H = 96, 64
SWITCH = "SPT_NO_PASS_PIPELINE"
SWITCHES = (SWITCH, "SPT_NO_FILM_STREAM", "SPT_NO_TAIL_LOOP", "SPT_NO_FUSED", "SPT_PRIMARY_CHUNKS", "SPT_NO_ORIGIN_CANDIDATES")
CUBE, MATERIALS = "cfg2_cube.json", "t_materials.json"
STATS_FIELDS = ("samples", "segments_closest", "segments_shadow", "primary_hits", "path_vertices", "shadow_first", "vertices_second")


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def tris64(tmp_path_factory):
    """The 64-triangle scene of test_gpu_origin_candidates.py (five cubes over two planes), written by that module's writer."""
    d = str(tmp_path_factory.mktemp("pass_pipeline"))
    os.makedirs(os.path.join(d, "models"))
    cam, inst = OC.SCENES["tris64"]
    for k, (kind, _) in enumerate(inst):
        with open(os.path.join(d, "models", "%s_%d.obj" % (kind, k)), "w") as f:
            f.write({"cube": S.CUBE_OBJ, "plane": S.PLANE_OBJ}[kind])
    path = os.path.join(d, "tris64.json")
    with open(path, "w") as f:
        json.dump(OC._scene_dict(cam, inst), f)
    return path


def _cube_path():
    return os.path.join(_util.SCENES, CUBE)


def _tracer(spp, seed=1, sampler=spt.SAMPLER_RECURRENCE, max_depth=None):
    r = spt.load_renderer(os.path.join(_util.SCENES, "pt.json"), seed=seed)
    assert r.max_depth == 8 and r.sampler == spt.SAMPLER_RECURRENCE
    r.spp, r.sampler = spp, sampler
    if max_depth is not None:
        r.max_depth = max_depth
    return r


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@functools.lru_cache(maxsize=None)
def _sync_film(path, cam, w, h, sampler, spp, spp_pass, seed, max_depth=None):
    """The synchronous film of a scene object of its own (read-only)."""
    scene = spt.load_scene(path)
    try:
        film = _tracer(spp, seed, sampler, max_depth).render_shard(scene, spt.OutputConfig(w, h, None, cam), samples_per_pass=spp_pass).copy()
    finally:
        scene.close()
    film.setflags(write=False)
    return film


def _async_film(scene, r, cfg, spp_pass):
    """One asynchronous render into a film of its own, waited for.  Returns the film and by how much counters 0 and 7 rose."""
    ds = scene.device_scene(0)
    before = (ds.render_info(0), ds.render_info(7))
    film = np.zeros((cfg.height, cfg.width, 3), dtype=f32)
    r.render_shard(scene, cfg, samples_per_pass=spp_pass, film=film, wait=False)
    r.wait(scene)
    return film, (ds.render_info(0) - before[0], ds.render_info(7) - before[1])


class _Pinned:
    """n page-locked (h, w, 3) f32 films."""

    def __init__(self, n, h, w):
        self.ptrs, self.films = [], []
        for _ in range(n):
            ptr = C.c_void_p()
            spt._check_hip(spt.hip_lib().spt_alloc_pinned(h * w * 12, C.byref(ptr)))
            self.ptrs.append(ptr)
            film = np.ctypeslib.as_array((C.c_float * (h * w * 3)).from_address(ptr.value)).reshape(h, w, 3)
            film[:] = 0
            self.films.append(film)

    def free(self):
        self.films = []
        for ptr in self.ptrs:
            spt.hip_lib().spt_free_pinned(ptr)
        self.ptrs = []


# ---- 1 and 2: set reuse, and the path taken -----------------------------------------------------------------------------------

# Passes of 8 or fewer samples are one chunk per tile at this size: such a k_primary adds into the film itself and first waits for
# everything queued on the film stream, so its pass runs BEHIND the previous pass's shade stage and only the ordering and the buffer
# binding are under test.  Passes of 16 are two chunks per tile: their k_primary is queued beside the previous pass's bounce launches,
# and a pass that read or wrote the other set's queues would show.  Every case that the sets matter for runs in both shapes.
SHAPES = [(20, 8), (40, 16)]
SHAPE_IDS = ["passes-of-8", "passes-of-16"]


@pytest.mark.parametrize("spp, spp_pass", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("sampler", [spt.SAMPLER_RECURRENCE, spt.SAMPLER_RANDOM], ids=["recurrence", "random"])
def test_three_passes_reuse_set_0_with_a_short_pass(sampler, spp, spp_pass, monkeypatch):
    """20 spp in passes of 8, 8 and 4 (40 in passes of 16, 16 and 8): the third pass takes set 0 again and is short.  Pipeline on, off,
    synchronous and the exhaustive oracle are the same words; counter 7 rises by 3 with the pipeline and by 0 without, counter 0 by 3
    both times."""
    cfg = spt.OutputConfig(W, H)
    want = _sync_film(_cube_path(), None, W, H, sampler, spp, spp_pass, 1)
    scene = spt.load_scene(_cube_path())
    try:
        r = _tracer(spp, 1, sampler)
        on, rose_on = _async_film(scene, r, cfg, spp_pass)
        monkeypatch.setenv(SWITCH, "1")
        off, rose_off = _async_film(scene, r, cfg, spp_pass)
        monkeypatch.delenv(SWITCH)
        again, rose_again = _async_film(scene, r, cfg, spp_pass)     # (and on again, after the switch-off frame)
        _util.ensure_cpu_build()
        ref, _ = _util.oracle_render(scene, r, W, H, flags=_util.ORACLE_EXHAUSTIVE)
    finally:
        scene.close()
    assert rose_on == (3, 3), "the passes did not take the pipeline"
    assert rose_off == (3, 0)
    assert rose_again == (3, 3)
    assert float(want.max()) > 0.01, "the camera sees nothing"
    assert _same(on, off), "pipeline on against off"
    assert _same(on, want), "pipeline on against the synchronous render"
    assert _same(again, want)
    assert _same(on, ref), "pipeline on against the exhaustive oracle"


# ---- 3: frames back to back ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spp, spp_pass, passes, sampler", [(20, 8, 3, spt.SAMPLER_RECURRENCE), (8, 8, 1, spt.SAMPLER_RECURRENCE), (40, 16, 3, spt.SAMPLER_RANDOM)],
                         ids=["three-passes", "one-pass", "chunked-random"])
def test_five_frames_back_to_back(spp, spp_pass, passes, sampler):
    """Five renders queued without a wait, seeds 1 to 5, into five pinned films: the sets alternate across renders (with one pass per
    frame every frame takes the other set).  A pass of 8 samples at this size is one chunk per tile, and such a k_primary adds into the
    film itself, behind the film stream; passes of 16 are two chunks, the kind that runs beside the previous pass's shade kernels.
    (On the cube under one directional light a film depends on the seed through the random sampler's offsets only: the third case
    has five different films.)"""
    cfg = spt.OutputConfig(W, H)
    seeds = (1, 2, 3, 4, 5)
    want = [_sync_film(_cube_path(), None, W, H, sampler, spp, spp_pass, s) for s in seeds]
    scene = spt.load_scene(_cube_path())
    pinned = _Pinned(len(seeds), H, W)
    try:
        ds = scene.device_scene(0)
        r = _tracer(spp, 1, sampler)
        for s, film in zip(seeds, pinned.films):
            r.seed = s
            r.render_shard(scene, cfg, samples_per_pass=spp_pass, film=film, wait=False)
        r.wait(scene)
        assert (ds.render_info(0), ds.render_info(7)) == (5 * passes, 5 * passes)
        for k, film in enumerate(pinned.films):
            assert _same(film, want[k]), "frame %d of five" % k
        if sampler == spt.SAMPLER_RANDOM:
            assert all(not _same(want[0], w) for w in want[1:]), "the seeds give one film"
    finally:
        scene.close()
        pinned.free()


# ---- 4: later bounces through the per-set queues ------------------------------------------------------------------------------

@pytest.mark.parametrize("spp, spp_pass", [(12, 4), (48, 16)], ids=["passes-of-4", "passes-of-16"])
@pytest.mark.parametrize("origin", [True, False], ids=["origin-candidates", "tree-walks"])
def test_later_bounces_ping_pong_on_the_shade_stage(tris64, origin, spp, spp_pass, monkeypatch):
    """The 64-triangle scene, 12 spp in passes of 4 (48 in passes of 16: k_primary of the next pass beside them, see SHAPES), on a scene
    without the tail-loop hint: bounces 1 to 7 are launches of their own that ping-pong through the set's qa and qb on the second stream."""
    if not origin:
        monkeypatch.setenv("SPT_NO_ORIGIN_CANDIDATES", "1")
    cfg = spt.OutputConfig(W, H)
    want = _sync_film(tris64, None, W, H, spt.SAMPLER_RECURRENCE, spp, spp_pass, 1)
    scene = spt.load_scene(tris64)
    try:
        r = _tracer(spp)
        on, rose_on = _async_film(scene, r, cfg, spp_pass)          # no synchronous render before it: no hint, no tail loop
        monkeypatch.setenv(SWITCH, "1")
        off, rose_off = _async_film(scene, r, cfg, spp_pass)
        monkeypatch.delenv(SWITCH)
        sync = r.render_shard(scene, cfg, samples_per_pass=spp_pass).copy()
        assert r.last_stats.vertices_second > 0, "no path goes on after bounce 0"
    finally:
        scene.close()
    assert rose_on == (3, 3), "the passes did not take the pipeline"
    assert rose_off == (3, 0)
    assert float(want.max()) > 0.01
    assert _same(on, off) and _same(on, sync) and _same(on, want)


# ---- 5: stats -----------------------------------------------------------------------------------------------------------------

def test_stats_of_the_synchronous_render_after_asynchronous_ones(monkeypatch):
    """A synchronous render behind two queued asynchronous ones (a benchmark's warm-up order): its stats are the same with the
    pipeline on, off and on a scene that never rendered asynchronously."""
    spp, spp_pass = 20, 8
    cfg = spt.OutputConfig(W, H)

    def stats_after_async(frames):
        scene = spt.load_scene(_cube_path())
        try:
            ds = scene.device_scene(0)
            r = _tracer(spp)
            for _ in range(frames):
                r.render_shard(scene, cfg, samples_per_pass=spp_pass, reuse_output=True, wait=False)
            film = r.render_shard(scene, cfg, samples_per_pass=spp_pass).copy()
            return film, r.last_stats, ds.render_info(7)
        finally:
            scene.close()

    film_on, st_on, pipe_on = stats_after_async(2)
    monkeypatch.setenv(SWITCH, "1")
    film_off, st_off, pipe_off = stats_after_async(2)
    monkeypatch.delenv(SWITCH)
    film_sync, st_sync, pipe_sync = stats_after_async(0)
    assert (pipe_on, pipe_off, pipe_sync) == (6, 0, 0)
    assert _same(film_on, film_off) and _same(film_on, film_sync)
    assert st_sync.samples == W * H * spp and st_sync.primary_hits > 0
    for field in STATS_FIELDS:
        assert getattr(st_on, field) == getattr(st_off, field) == getattr(st_sync, field), field


# ---- 6: joins -----------------------------------------------------------------------------------------------------------------

def _moved(scene):
    fwd = S.fwd_by_name(scene, ["cube"])["cube"]
    fwd[9:12] += np.array([0.4, -0.3, 0.5], dtype=f32)
    scene.set_transforms({"cube": fwd})


def _squeezed(scene):
    pos = scene.mesh_positions("cube").copy()
    pos[:, 0] *= f32(0.5)
    scene.set_mesh_positions("cube", pos)


@pytest.mark.parametrize("spp, spp_pass", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("edit", [_moved, _squeezed], ids=["update", "deform"])
def test_a_scene_edit_behind_a_pipelined_render(edit, spp, spp_pass):
    """Render asynchronously, edit the scene without waiting (spt_scene_update / spt_scene_deform), render again, wait: the first
    film is the old state's, the second that of a fresh scene in the new state."""
    cfg = spt.OutputConfig(W, H)
    fresh = spt.load_scene(_cube_path())
    try:
        edit(fresh)
        want = _tracer(spp).render_shard(fresh, cfg, samples_per_pass=spp_pass).copy()
    finally:
        fresh.close()
    before = _sync_film(_cube_path(), None, W, H, spt.SAMPLER_RECURRENCE, spp, spp_pass, 1)
    scene = spt.load_scene(_cube_path())
    try:
        ds = scene.device_scene(0)
        r = _tracer(spp)
        films = [np.zeros((H, W, 3), dtype=f32) for _ in range(2)]
        r.render_shard(scene, cfg, samples_per_pass=spp_pass, film=films[0], wait=False)
        edit(scene)
        ds.update()
        r.render_shard(scene, cfg, samples_per_pass=spp_pass, film=films[1], wait=False)
        r.wait(scene)
        assert ds.render_info(7) == 6, "the passes did not take the pipeline"
    finally:
        scene.close()
    assert not _same(want, before), "the edit changed nothing"
    assert _same(films[0], before), "the first frame saw the edit"
    assert _same(films[1], want), "the second frame against a fresh scene in the new state"


@pytest.mark.parametrize("spp, spp_pass", SHAPES, ids=SHAPE_IDS)
def test_workspace_growth_behind_a_pipelined_render(spp, spp_pass):
    """The second render is larger: its workspace (both queue sets) grows while the first is in flight on three streams."""
    sizes = ((W, H), (160, 112))
    want = [_sync_film(_cube_path(), None, w, h, spt.SAMPLER_RECURRENCE, spp, spp_pass, 1) for w, h in sizes]
    scene = spt.load_scene(_cube_path())
    try:
        ds = scene.device_scene(0)
        r = _tracer(spp)
        films = [np.zeros((h, w, 3), dtype=f32) for w, h in sizes]
        for (w, h), film in zip(sizes, films):
            r.render_shard(scene, spt.OutputConfig(w, h), samples_per_pass=spp_pass, film=film, wait=False)
        r.wait(scene)
        assert ds.render_info(7) == 6, "the passes did not take the pipeline"
    finally:
        scene.close()
    for k, film in enumerate(films):
        assert _same(film, want[k]), "size %d x %d" % sizes[k]


# ---- the tail-loop launch on the film stream, and the refused second set --------------------------------------------------------

@pytest.mark.parametrize("which", ["cube", "tris64"])
def test_frames_behind_a_synchronous_render_take_the_tail_loop(which, tris64):
    """A synchronous render first: it leaves the tail-loop hint, so the asynchronous frames behind it run bounce 1 and everything after
    it as ONE launch on the film stream, which reads the set's qb / hits_next while bounce 0 of the next pass writes the other set's
    (the headline's configuration; on the cube no path goes on, on the 64-triangle scene many do).  Three frames of three passes of 16,
    queued back to back."""
    spp, spp_pass = 48, 16
    path = _cube_path() if which == "cube" else tris64
    cfg = spt.OutputConfig(W, H)
    want = _sync_film(path, None, W, H, spt.SAMPLER_RECURRENCE, spp, spp_pass, 1)
    scene = spt.load_scene(path)
    try:
        ds = scene.device_scene(0)
        r = _tracer(spp)
        sync = r.render_shard(scene, cfg, samples_per_pass=spp_pass).copy()
        films = [np.zeros((H, W, 3), dtype=f32) for _ in range(3)]
        for film in films:
            r.render_shard(scene, cfg, samples_per_pass=spp_pass, film=film, wait=False)
        r.wait(scene)
        assert (ds.render_info(0), ds.render_info(7)) == (9, 9), "the passes did not take the pipeline"
    finally:
        scene.close()
    assert _same(sync, want)
    for k, film in enumerate(films):
        assert _same(film, want), "frame %d of three" % k


def test_a_refused_second_set_keeps_the_two_stream_schedule(monkeypatch):
    """SPT_PASS_PIPELINE_MAX_BYTES stands in for a device without memory for the second queue set: 4 MB admit the first of its fourteen
    buffers at this size and refuse the second.  A pipelined frame is queued, then - without a wait - two frames under the limit: the set is released behind
    the frame that uses it, the frames take the two-stream schedule (counter 7 stays, counter 0 rises), every film is right.  A scene
    that meets the limit at its first render never makes the set."""
    spp, spp_pass = 40, 16
    cfg = spt.OutputConfig(W, H)
    want = _sync_film(_cube_path(), None, W, H, spt.SAMPLER_RECURRENCE, spp, spp_pass, 1)
    scene = spt.load_scene(_cube_path())
    try:
        ds = scene.device_scene(0)
        r = _tracer(spp)
        films = [np.zeros((H, W, 3), dtype=f32) for _ in range(3)]
        r.render_shard(scene, cfg, samples_per_pass=spp_pass, film=films[0], wait=False)
        assert (ds.render_info(0), ds.render_info(7)) == (3, 3)
        monkeypatch.setenv("SPT_PASS_PIPELINE_MAX_BYTES", str(4 << 20))
        for film in films[1:]:
            r.render_shard(scene, cfg, samples_per_pass=spp_pass, film=film, wait=False)
        r.wait(scene)
        assert (ds.render_info(0), ds.render_info(7)) == (9, 3)
    finally:
        scene.close()
    for k, film in enumerate(films):
        assert _same(film, want), "frame %d of three" % k
    scene = spt.load_scene(_cube_path())
    try:
        ds = scene.device_scene(0)
        sync = _tracer(spp).render_shard(scene, cfg, samples_per_pass=spp_pass).copy()
        film, rose = _async_film(scene, _tracer(spp), cfg, spp_pass)
    finally:
        scene.close()
    assert rose == (3, 0)
    assert _same(sync, want) and _same(film, want)


# ---- 7: plans that keep their schedule ----------------------------------------------------------------------------------------

def test_an_unfused_scene_keeps_the_two_stream_schedule(monkeypatch):
    """t_materials (general shade kernels, shadow rays on the second stream), 12 spp in passes of 5, 5 and 2."""
    w, h, spp, spp_pass = 64, 48, 12, 5
    cfg = spt.OutputConfig(w, h, None, "main")
    path = os.path.join(_util.SCENES, MATERIALS)
    want = _sync_film(path, "main", w, h, spt.SAMPLER_RECURRENCE, spp, spp_pass, 5)
    scene = spt.load_scene(path)
    try:
        r = _tracer(spp, 5)
        on, rose_on = _async_film(scene, r, cfg, spp_pass)
        monkeypatch.setenv(SWITCH, "1")
        off, rose_off = _async_film(scene, r, cfg, spp_pass)
    finally:
        scene.close()
    assert rose_on == (3, 0) and rose_off == (3, 0)
    assert _same(on, off) and _same(on, want)


def test_a_film_increment_and_a_synchronous_render_keep_the_main_stream(monkeypatch):
    spp, spp_pass = 20, 8
    cfg = spt.OutputConfig(W, H)
    want = _sync_film(_cube_path(), None, W, H, spt.SAMPLER_RECURRENCE, spp, spp_pass, 1)

    def run():
        scene = spt.load_scene(_cube_path())
        try:
            ds = scene.device_scene(0)
            r = _tracer(spp)
            with r.progressive(scene, cfg, samples_per_pass=spp_pass) as pf:
                first = pf.render(12).mean().copy()
                whole = pf.render(8).mean().copy()
            sync = r.render_shard(scene, cfg, samples_per_pass=spp_pass).copy()
            return first, whole, sync, ds.render_info(7)
        finally:
            scene.close()

    on = run()
    monkeypatch.setenv(SWITCH, "1")
    off = run()
    assert on[3] == 0 and off[3] == 0
    for a, b in zip(on[:3], off[:3]):
        assert _same(a, b)
    assert _same(on[1], want) and _same(on[2], want)
    assert not _same(on[0], want)
