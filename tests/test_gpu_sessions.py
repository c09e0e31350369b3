"""Long-lived scenes: sequences of different calls on ONE device scene, every call against the oracle (tools/fuzz_sessions.py).

The scene object carries its workspace (grown, never cleared as a whole), three caches keyed by the camera, tail_vertices, the
copy stream of asynchronous frames and any number of films from call to call; a fixed list of drawn sessions, two threads on
one scene and on two scenes, and a few sequences written out by hand pin what the host code passes to the kernels on the
fifth call.  Seeds that ever failed a campaign (profiles/sessions_fuzz_campaign.txt) stay in the lists with their cause."""
import importlib.util
import os
import shutil
import threading

import numpy as np
import pytest

import _util

pytestmark = pytest.mark.gpu

# every scene of the pool, every step kind and every refused call between them (tests/test_session_generator.py asserts it)
SEEDS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12]
SEEDS_SWITCHES = [13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25]
CALL_SWITCHES = ("SPT_NO_FUSED", "SPT_NO_CLASS_QUEUES", "SPT_NO_LDS_TABLES", "SPT_NO_TAIL_LOOP", "SPT_NO_PACK_FIRST", "SPT_NO_PIXEL_CULL",
                 "SPT_NO_ROW_SPANS", "SPT_NO_EYE_BLOB", "SPT_NO_OVERLAP", "SPT_NO_DYN_SHADOW", "SPT_NO_DYN_EXTEND", "SPT_PRIMARY_CHUNKS",
                 "SPT_BOX_BAND_BYTES")


@pytest.fixture(scope="module")
def sessions():
    spec = importlib.util.spec_from_file_location("fuzz_sessions", os.path.join(_util.ROOT, "tools", "fuzz_sessions.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    work = mod.stage_assets()
    yield mod, work
    shutil.rmtree(work, ignore_errors=True)


@pytest.fixture(autouse=True)
def _no_call_switches(monkeypatch):
    for name in CALL_SWITCHES:
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("seed,switches", [(s, False) for s in SEEDS] + [(s, True) for s in SEEDS_SWITCHES],
                         ids=["%d" % s for s in SEEDS] + ["%d-switches" % s for s in SEEDS_SWITCHES])
def test_session_matches_oracle(sessions, seed, switches):
    mod, work = sessions
    ok, info = mod.run_session(seed, work, switches=switches)
    assert ok, info


def _open(mod, scene_name):
    """A session on a committed scene with the camera pool of the tool (0: the scene's own; 1, 5 and 6: one eye, three views)."""
    path = os.path.join(_util.SCENES, scene_name)
    sc = mod.spt.load_scene(path)
    cams = mod.camera_pool(sc, np.random.default_rng(5))
    sc.close()
    return mod.Session(path, cams)       # opens the device scene


def _run(mod, session, steps, errors, tag):
    try:
        for k, st in enumerate(steps):
            try:
                mod.run_step(session, st)
            except (mod.Mismatch, mod.spt.SptError) as e:
                raise AssertionError("%s step %d (%s): %s" % (tag, k, st["kind"], e))
    except BaseException as e:      # handed to the main thread
        errors.append(e)


def _thread_steps(mod, variant):
    """Two different fixed step lists (renders, rays, film increments; no switches, no asynchronous frames); every render
    writes a fresh array of its own."""
    R, F = mod.render_step, mod.film_step_create
    if variant == 0:
        return [R(200, 150, 1, depth=8), {"kind": "trace", "n": 20000, "ray_seed": 1}, F(10, 48, 32, 2, sampler=2),
                R(9, 7, 5, spp_pass=1), {"kind": "film_render", "film": 10, "n": 3}, R(160, 120, 0, radius=1.2, spp=2),
                {"kind": "film_render", "film": 10, "n": 5}, {"kind": "film_read", "film": 10, "what": ["sum", "sum_sq", "mean", "variance_of_mean", "counts"]},
                {"kind": "trace", "n": 1, "ray_seed": 2}, R(64, 48, 1, depth=1), {"kind": "film_close", "film": 10}, R(200, 150, 5, depth=8)]
    return [{"kind": "trace", "n": 257, "ray_seed": 3}, R(17, 33, 4, depth=0), F(11, 40, 24, 0, moments=False, radius=0.3),
            R(240, 180, 3, spp=2, shard_count=2, strip_rows=4), {"kind": "film_render", "film": 11, "n": 8}, R(33, 17, 2, sampler=1, dx=2, dy=2, depth=8),
            {"kind": "film_read", "film": 11, "what": ["sum", "mean", "counts"]}, {"kind": "trace", "n": 40000, "ray_seed": 4},
            R(120, 90, 4, radius=1.6, spp=3, spp_pass=2), {"kind": "film_close", "film": 11}, R(16, 16, 0), R(100, 100, 1, out="film", shard_count=3, strip_rows=16)]


@pytest.mark.parametrize("scene_name", ["t_materials.json", "cfg2_cube.json"])
def test_two_threads_one_scene(sessions, scene_name):
    """The scene's mutex: two threads make different calls on the same device scene at the same time and every result is
    the oracle's, that is, what a serial run gives."""
    mod, _ = sessions
    session = _open(mod, scene_name)
    errors = []
    threads = [threading.Thread(target=_run, args=(mod, session, _thread_steps(mod, v), errors, "thread %d" % v)) for v in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    session.close()
    if errors:
        raise errors[0]


def test_two_threads_two_scenes(sessions):
    """One scene per thread; a refused call on thread A leaves spt_last_error() of thread B as it was (the message is per thread)."""
    mod, _ = sessions
    lib = mod.spt.hip_lib()
    sess = [_open(mod, "t_materials.json"), _open(mod, "t_textured.json")]
    errors, seen = [], {}
    a_refused, b_has_message = threading.Event(), threading.Event()

    def last():
        msg = lib.spt_last_error()
        return msg.decode() if isinstance(msg, bytes) else str(msg)

    def thread_a():
        steps = _thread_steps(mod, 0)
        _run(mod, sess[0], steps[:4], errors, "thread A")
        b_has_message.wait(120)
        _run(mod, sess[0], [{"kind": "refused", "which": "max_depth_256"}], errors, "thread A")
        seen["a"] = last()
        a_refused.set()
        _run(mod, sess[0], steps[4:], errors, "thread A")

    def thread_b():
        steps = _thread_steps(mod, 1)
        _run(mod, sess[1], steps[:3] + [{"kind": "refused", "which": "zero_width"}], errors, "thread B")
        seen["b_before"] = last()
        b_has_message.set()
        a_refused.wait(120)
        seen["b_after"] = last()
        _run(mod, sess[1], steps[3:], errors, "thread B")
        seen["b_end"] = last()

    threads = [threading.Thread(target=thread_a), threading.Thread(target=thread_b)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for s in sess:
        s.close()
    if errors:
        raise errors[0]
    assert "max_depth" in seen["a"] and "width" in seen["b_before"]
    assert seen["b_after"] == seen["b_before"] == seen["b_end"] != seen["a"]


def test_hand_written_regressions(sessions, monkeypatch):
    mod, _ = sessions
    R, F = mod.render_step, mod.film_step_create

    def play(scene_name, steps):
        session = _open(mod, scene_name)
        try:
            for k, st in enumerate(steps):
                if callable(st):
                    st(session)
                    continue
                try:
                    mod.run_step(session, st)
                except (mod.Mismatch, mod.spt.SptError) as e:
                    raise AssertionError("%s step %d (%s): %s" % (scene_name, k, st, e))
        finally:
            session.close()

    for scene_name in ("t_materials.json", "cfg2_cube.json", "cfg1_sphere.json"):
        # (a) the camera caches: A small, A large (spans of another size), B with A's eye (eye copy kept, spans remade), A small again
        # (camera 6: A's eye and fov, turned - its row spans differ from A's by the axes alone)
        play(scene_name, [R(64, 48, 1), R(200, 150, 1), R(200, 150, 5), R(64, 48, 1), R(64, 48, 2), R(64, 48, 1), R(64, 48, 6), R(64, 48, 1),
                          R(200, 150, 6), R(200, 150, 1), R(200, 150, 6, debug_normal=True), R(200, 150, 1, debug_normal=True)])
        # (b) the wide box filter keeps every sample in `rad`: wide and large, narrow and tiny, wide again in narrow bands
        play(scene_name, [R(160, 120, 0, radius=1.2, spp=3), R(16, 16, 0), lambda s: monkeypatch.setenv("SPT_BOX_BAND_BYTES", "20000"),
                          R(40, 30, 0, radius=1.2, spp=3), lambda s: monkeypatch.delenv("SPT_BOX_BAND_BYTES"), R(40, 30, 4, radius=1.6, spp=2)])
        # (c) max_depth 8 -> 0 -> 1 -> 8: counts_words and the class queues follow the depth; tail_vertices is the previous call's
        play(scene_name, [R(96, 64, 0, depth=8), R(96, 64, 0, depth=0), R(96, 64, 0, depth=1), R(96, 64, 0, depth=8)])
        # (d) a film with moments beside a large unrelated render, an adapt, an asynchronous pair with another camera
        pair = R(80, 60, 3, out="reuse")
        pair["kind"] = "async_pair"
        play(scene_name, [F(0, 48, 32, 0), R(240, 180, 1, spp=2), {"kind": "film_render", "film": 0, "n": 4},
                          {"kind": "film_adapt", "film": 0, "quantile": 0.4, "floor": 0.0, "min_samples": 2}, pair,
                          {"kind": "film_render", "film": 0, "n": 4},
                          {"kind": "film_read", "film": 0, "what": ["sum", "sum_sq", "mean", "variance_of_mean", "counts"]},
                          {"kind": "film_close", "film": 0}])

        # (e) an asynchronous frame, a refused call while it is in flight, the wait, a render
        def async_refused_wait(session):
            plan = R(120, 90, 1, out="reuse")
            r, cam = mod._renderer(plan), session.cams[1]
            got = r.render_shard(session.sc, mod.spt.OutputConfig(120, 90, None, cam), reuse_output=True, wait=False)
            session.refused({"kind": "refused", "which": "jittered_mismatch"})
            session.refused({"kind": "refused", "which": "pass_too_large"})
            r.wait(session.sc)
            assert _util.same_words(got.copy(), mod.oracle_film(session.sc, plan, cam, 0)), "the asynchronous frame after a refused call"

        play(scene_name, [R(32, 24, 0), async_refused_wait, R(120, 90, 2), R(32, 24, 0, radius=1.2)])
