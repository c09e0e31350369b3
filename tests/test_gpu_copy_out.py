"""The finish kernel that stores the image into the caller's page-locked buffer itself (k_finish_host) instead of
leaving it to the runtime's device-to-host copy: packed films, ragged rows, misaligned bases, strided shards, buffer reuse, and
every case that must still take the copy.

Every film is compared bit for bit (uint32 views) with the synchronous render of the same plan into a pageable array - which
takes the runtime's copy by construction - from a scene object of its own; that film is checked against the oracle once.
Counter 3 of spt_debug_render_info says how many frames went without the copy."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import _util

pytestmark = pytest.mark.gpu

spt = _util.load_pkg()

CUBE = "cfg2_cube.json"
SPP, SPP_PASS = 24, 4
PATTERN = np.uint32(0x7fc0beef)   # (a NaN no render produces)


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in ("SPT_NO_DIRECT_OUT", "SPT_NO_FILM_STREAM"):
        monkeypatch.delenv(name, raising=False)


@functools.lru_cache(maxsize=None)
def _reference_scene():
    return spt.load_scene(os.path.join(_util.SCENES, CUBE))


def _tracer(seed, radius=0.5):
    return spt.PathTracer(max_depth=8, sampler=spt.SAMPLER_RECURRENCE, spp=SPP, seed=seed, filter_radius=radius)


@functools.lru_cache(maxsize=None)
def _expected(w, h, seed, radius=0.5):
    """The synchronous film into a pageable array (read-only), checked against the oracle's bits once, here."""
    scene = _reference_scene()
    r = _tracer(seed, radius)
    before = scene.device_scene(0).render_info(3)
    film = r.render_shard(scene, spt.OutputConfig(w, h), samples_per_pass=SPP_PASS).copy()
    assert scene.device_scene(0).render_info(3) == before, "a pageable film went without the copy"
    ref, _ = _util.oracle_render(scene, r, w, h, flags=_util.device_oracle_flags())
    assert np.array_equal(film.view(np.uint32), ref.view(np.uint32)), "the synchronous film differs from the oracle"
    film.setflags(write=False)
    return film


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


class Pinned:
    """Page-locked bytes (spt_alloc_pinned), filled with PATTERN; float views at any byte offset."""

    def __init__(self, nbytes):
        self.ptr = C.c_void_p()
        self.nbytes = (nbytes + 3) // 4 * 4
        spt._check_hip(spt.hip_lib().spt_alloc_pinned(self.nbytes, C.byref(self.ptr)))
        self.words = np.ctypeslib.as_array((C.c_uint32 * (self.nbytes // 4)).from_address(self.ptr.value))
        self.words[:] = PATTERN

    def floats(self, byte_offset, shape):
        n = int(np.prod(shape))
        assert byte_offset % 4 == 0 and byte_offset + 4 * n <= self.nbytes
        return self.words[byte_offset // 4: byte_offset // 4 + n].view(np.float32).reshape(shape)

    def free(self):
        self.words = None
        spt.hip_lib().spt_free_pinned(self.ptr)


class Case:
    """A fresh scene and the pinned allocations of one test: the scene is closed first (its destroy drains the streams)."""

    def __init__(self):
        self.scene = spt.load_scene(os.path.join(_util.SCENES, CUBE))
        self.ds = self.scene.device_scene(0)
        self.pins = []

    def pinned(self, nbytes):
        self.pins.append(Pinned(nbytes))
        return self.pins[-1]

    def direct(self):
        return self.ds.render_info(3)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.scene.close()
        for p in self.pins:
            p.free()


def test_packed_film_reused_and_three_separate_films():
    """Case 1: 96 x 80, three seeds queued back to back into the scene's pinned buffer, then into three pinned films."""
    w, h, seeds = 96, 80, (11, 12, 13)
    cfg = spt.OutputConfig(w, h)
    want = [_expected(w, h, s) for s in seeds]
    with Case() as c:
        r = _tracer(seeds[0])
        before = c.direct()
        for s in seeds:
            r.seed = s
            out = r.render_shard(c.scene, cfg, samples_per_pass=SPP_PASS, reuse_output=True, wait=False)
        r.wait(c.scene)
        assert _same(out, want[-1])
        assert c.direct() - before == 3
        films = [c.pinned(w * h * 12).floats(0, (h, w, 3)) for _ in seeds]
        for s, film in zip(seeds, films):
            r.seed = s
            r.render_shard(c.scene, cfg, samples_per_pass=SPP_PASS, film=film, wait=False)
        r.wait(c.scene)
        for k, film in enumerate(films):
            assert _same(film, want[k]), "frame %d of three" % k
        assert c.direct() - before == 6


@pytest.mark.parametrize("wait", [False, True], ids=["async", "sync"])
@pytest.mark.parametrize("offset", [0, 4], ids=["base+0", "base+4"])
def test_ragged_rows_and_a_misaligned_base(offset, wait):
    """Case 2: 97 x 33 (rows of 1164 bytes, no multiple of 16), the image `offset` bytes into a pinned allocation with one guard
    row either side; the guards keep their pattern.  The synchronous render keeps the copy (the kernel is for overlapped frames) and
    must leave the same bytes."""
    w, h = 97, 33
    want = _expected(w, h, 21)
    with Case() as c:
        pin = c.pinned(offset + (h + 2) * w * 12)
        frame = pin.floats(offset, (h + 2, w, 3))
        film = frame[1:h + 1]
        assert film.flags["C_CONTIGUOUS"] and film.ctypes.data == pin.ptr.value + offset + w * 12
        before = c.direct()
        r = _tracer(21)
        r.render_shard(c.scene, spt.OutputConfig(w, h), samples_per_pass=SPP_PASS, film=film, wait=wait)
        if not wait:
            r.wait(c.scene)
        assert c.direct() - before == (0 if wait else 1)
        assert _same(film, want)
        assert (frame[0].view(np.uint32) == PATTERN).all() and (frame[h + 1].view(np.uint32) == PATTERN).all(), "a guard row was written"
        assert (pin.words[:offset // 4] == PATTERN).all()


def test_strided_shards_into_one_pinned_film():
    """Case 3: shards 0 - 2 of 3, strips of 4 rows, into one pinned 96 x 80 film (20 strips: the shards own 7, 7 and 6, so the
    film's last strip belongs to shard 1); rows keep their pattern until their owner writes them."""
    w, h, strip, shards = 96, 80, 4, 3
    want = _expected(w, h, 11)
    with Case() as c:
        film = c.pinned(w * h * 12).floats(0, (h, w, 3))
        owner = (np.arange(h) // strip) % shards
        r = _tracer(11)
        before = c.direct()
        for k in range(shards):
            r.render_shard(c.scene, spt.OutputConfig(w, h), shard_index=k, shard_count=shards, strip_rows=strip, samples_per_pass=SPP_PASS,
                           film=film, wait=False)
            r.wait(c.scene)
            assert _same(film[owner <= k], want[owner <= k]), "rows of shards 0 .. %d" % k
            assert (film[owner > k].view(np.uint32) == PATTERN).all(), "shard %d wrote rows it does not own" % k
        assert _same(film, want)
        assert c.direct() - before == shards


def test_short_last_strip_of_a_strided_shard():
    """Case 3, the short strip: 96 x 78 in strips of 4 is 19 full strips and one of 2 rows, which shard 1 of 3 owns."""
    w, h, strip, shards = 96, 78, 4, 3
    want = _expected(w, h, 12)
    with Case() as c:
        film = c.pinned(w * h * 12).floats(0, (h, w, 3))
        r = _tracer(12)
        for k in (1, 2, 0):
            r.render_shard(c.scene, spt.OutputConfig(w, h), shard_index=k, shard_count=shards, strip_rows=strip, samples_per_pass=SPP_PASS,
                           film=film, wait=False)
        r.wait(c.scene)
        assert _same(film, want)
        assert c.direct() == shards


@pytest.mark.parametrize("wait", [False, True], ids=["async", "sync"])
def test_pageable_film_takes_the_copy(wait):
    """Case 4a."""
    w, h = 96, 80
    want = _expected(w, h, 11)
    with Case() as c:
        film = np.zeros((h, w, 3), dtype=np.float32)
        r = _tracer(11)
        r.render_shard(c.scene, spt.OutputConfig(w, h), samples_per_pass=SPP_PASS, film=film, wait=wait)
        r.wait(c.scene)
        assert c.direct() == 0
        assert _same(film, want)


def test_film_straddling_the_end_of_a_pinned_region_takes_the_copy():
    """Case 4b: only the first half of the film is page-locked (spt_pin_host); afterwards the whole of it is, and the next frame
    goes without the copy - the check is made per call."""
    w, h = 96, 80
    want = _expected(w, h, 11)
    with Case() as c:
        film = np.zeros((h, w, 3), dtype=np.float32)
        r = _tracer(11)
        lib = spt.hip_lib()
        spt._check_hip(lib.spt_pin_host(film.ctypes.data, film.nbytes // 2))
        try:
            r.render_shard(c.scene, spt.OutputConfig(w, h), samples_per_pass=SPP_PASS, film=film, wait=False)
            r.wait(c.scene)
        finally:
            lib.spt_unpin_host(film.ctypes.data)
        assert c.direct() == 0
        assert _same(film, want)
        film[:] = 0
        spt._check_hip(lib.spt_pin_host(film.ctypes.data, film.nbytes))
        try:
            r.render_shard(c.scene, spt.OutputConfig(w, h), samples_per_pass=SPP_PASS, film=film, wait=False)
            r.wait(c.scene)
        finally:
            lib.spt_unpin_host(film.ctypes.data)
        assert c.direct() == 1
        assert _same(film, want)


def test_the_switch_restores_the_copy(monkeypatch):
    """Case 4c: SPT_NO_DIRECT_OUT=1, read per render."""
    w, h = 96, 80
    want = _expected(w, h, 11)
    with Case() as c:
        r = _tracer(11)
        monkeypatch.setenv("SPT_NO_DIRECT_OUT", "1")
        out = r.render_shard(c.scene, spt.OutputConfig(w, h), samples_per_pass=SPP_PASS, reuse_output=True, wait=False)
        r.wait(c.scene)
        assert c.direct() == 0
        assert _same(out, want)
        out[:] = 0
        monkeypatch.delenv("SPT_NO_DIRECT_OUT")
        r.render_shard(c.scene, spt.OutputConfig(w, h), samples_per_pass=SPP_PASS, reuse_output=True, wait=False)
        r.wait(c.scene)
        assert c.direct() == 1
        assert _same(out, want)


def test_the_single_stream_schedule_keeps_the_copy(monkeypatch):
    """Case 4, one more: SPT_NO_FILM_STREAM=1 puts the finish kernel on the main stream, where the slow kernel has no place."""
    w, h = 96, 80
    want = _expected(w, h, 11)
    with Case() as c:
        r = _tracer(11)
        monkeypatch.setenv("SPT_NO_FILM_STREAM", "1")
        out = r.render_shard(c.scene, spt.OutputConfig(w, h), samples_per_pass=SPP_PASS, reuse_output=True, wait=False)
        r.wait(c.scene)
        assert c.direct() == 0
        assert _same(out, want)


@pytest.mark.parametrize("radius", [0.4, 1.2], ids=["radius-0.4", "radius-1.2"])
def test_other_box_radii_take_the_copy(radius):
    """Case 4d: k_finish_box (a radius below 0.5) and k_filter_box (one that reaches the neighbours) keep their copies."""
    w, h = 96, 80
    want = _expected(w, h, 11, radius)
    with Case() as c:
        r = _tracer(11, radius)
        out = r.render_shard(c.scene, spt.OutputConfig(w, h), samples_per_pass=SPP_PASS, reuse_output=True, wait=False)
        r.wait(c.scene)
        assert c.direct() == 0
        assert _same(out, want)


def test_asynchronous_and_synchronous_frames_mixed():
    """Case 5: an asynchronous frame, a synchronous render of another seed, an asynchronous frame into a different pinned film."""
    w, h = 96, 80
    cfg = spt.OutputConfig(w, h)
    want = [_expected(w, h, s) for s in (11, 12, 13)]
    with Case() as c:
        films = [c.pinned(w * h * 12).floats(0, (h, w, 3)) for _ in range(2)]
        r = _tracer(11)
        r.render_shard(c.scene, cfg, samples_per_pass=SPP_PASS, film=films[0], wait=False)
        r.seed = 12
        sync = r.render_shard(c.scene, cfg, samples_per_pass=SPP_PASS).copy()                 # pageable: the copy
        r.seed = 13
        r.render_shard(c.scene, cfg, samples_per_pass=SPP_PASS, film=films[1], wait=False)
        r.wait(c.scene)
        assert _same(films[0], want[0]) and _same(sync, want[1]) and _same(films[1], want[2])
        assert c.direct() == 2
