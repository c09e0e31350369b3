"""The session generator of tools/fuzz_sessions.py, without a GPU: for every seed tests/test_gpu_sessions.py commits, the draw
is deterministic, the step list satisfies every ordering constraint the tool promises (large -> tiny -> large in pixels, samples
per pass, depth and ray-batch size, a narrow filter after a wide one, cameras revisited, a film increment right after a larger
unrelated render), the committed seeds together cover every scene of the pool, every step kind and every refused call, and the
oracle accepts the arguments of the render, ray and film steps (the first steps of a few seeds, at reduced size)."""
import importlib.util
import os
import shutil

import numpy as np
import pytest

import _util


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_util.ROOT, *name.split("/")) + ".py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def sessions():
    mod = _load("tools/fuzz_sessions")
    work = mod.stage_assets()
    yield mod, work
    shutil.rmtree(work, ignore_errors=True)


def _committed_seeds():
    src = open(os.path.join(_util.ROOT, "tests", "test_gpu_sessions.py")).read()
    scope = {}
    for name in ("SEEDS", "SEEDS_SWITCHES"):      # the two lists are plain literals: no import of a module marked gpu
        line = [l for l in src.splitlines() if l.startswith(name + " = ")][0]
        exec(line, scope)
    return scope["SEEDS"], scope["SEEDS_SWITCHES"]


def test_committed_seeds_are_deterministic_constrained_and_cover_the_pool(sessions):
    mod, work = sessions
    plain, switched = _committed_seeds()
    assert len(plain) >= 10 and len(switched) >= 10
    scenes, kinds, refusals, film_kinds, closed_with_film, switch_names = set(), set(), set(), set(), 0, set()
    for seed in sorted(set(plain + switched)):
        plan, why = mod.plan_session(seed, work)
        assert plan is not None, (seed, why)                  # no committed seed is a scene the loader rejects
        path, name, heavy, cams, steps = plan
        again = mod.plan_session(seed, work)[0]
        assert again[1:] == plan[1:], seed                    # same seed, same scene, cameras and steps
        assert mod.check_constraints(steps) == [], seed
        assert cams[1]["eye"] == cams[5]["eye"] == cams[6]["eye"] and cams[1]["fov"] != cams[5]["fov"] and cams[1]["forward"] != cams[5]["forward"]
        assert cams[1]["fov"] == cams[6]["fov"] and cams[1]["forward"] != cams[6]["forward"]      # the same eye and fov, turned
        assert steps[-1]["kind"] == "close_scene" and 20 <= len(steps) <= 60, (seed, len(steps))
        scenes.add(os.path.basename(path) if name != "generated" else name)
        kinds |= {st["kind"] for st in steps}
        refusals |= {st["which"] for st in steps if st["kind"] == "refused"}
        for st in steps:
            if st["kind"] == "film_create":
                film_kinds |= {"moments" if st["moments"] else "plain"} | ({"shard"} if st["shard_count"] > 1 else set()) | \
                              ({"first_sample"} if st["first_sample"] else set()) | ({"radius_0.3"} if st["radius"] == 0.3 else set())
            if st["kind"] == "render":
                kinds |= {"out_" + st["out"]} | ({"wide"} if st["radius"] > 1 else set()) | ({"twin"} if st["count_visits"] or st["profile"] else set())
                kinds |= {"more_shards_than_strips"} if st["shard_count"] > (st["h"] + st["strip_rows"] - 1) // st["strip_rows"] else set()
        closed_with_film += bool(steps[-1]["open_films"])
        # the films of the generator's own bookkeeping never pass their plan, never adapt without moments, never read a mean of nothing
        done, films = {}, {}
        for st in steps:
            if st["kind"] == "film_create":
                films[st["film"]], done[st["film"]] = st, 0
                assert len(films) <= 3 and len(mod.spt.shard_rows(st["h"], st["shard_index"], st["shard_count"], st["strip_rows"])) > 0
            elif st["kind"] == "film_render":
                done[st["film"]] += st["n"]
                assert films[st["film"]]["first_sample"] + done[st["film"]] <= films[st["film"]]["spp"]
            elif st["kind"] == "film_adapt":
                assert films[st["film"]]["moments"] and films[st["film"]]["radius"] == 0.5 and done[st["film"]] >= 2
            elif st["kind"] == "film_read":
                assert done[st["film"]] > 0 or not ({"mean", "variance_of_mean"} & set(st["what"]))
            elif st["kind"] == "film_close":
                del films[st["film"]]
        if seed in switched:
            envs = mod.draw_switches(seed, steps)
            assert envs == mod.draw_switches(seed, steps) and len(envs) == len(steps)
            switch_names |= {k for env in envs for k in env}
            rs = [env for env, st in zip(envs, steps) if st["kind"] in ("render", "async_pair", "async_then_sync")]
            cq, eye = ["SPT_NO_CLASS_QUEUES" in env for env in rs], ["SPT_NO_EYE_BLOB" in env for env in rs]
            assert any(cq[k] and not cq[k + 1] for k in range(len(rs) - 1)), seed                        # class queues off, then on
            assert any(not eye[k] and eye[k + 1] and not eye[k + 2] for k in range(len(rs) - 2)), seed   # eye copy used, skipped, used
    assert scenes == {os.path.basename(s) for s in mod.COMMITTED} | {"generated"}
    assert kinds >= {"render", "async_pair", "async_then_sync", "trace", "film_create", "film_render", "film_adapt", "film_read", "film_close",
                     "refused", "close_scene", "out_fresh", "out_reuse", "out_film", "wide", "twin", "more_shards_than_strips"}
    assert refusals == {"jittered_mismatch", "max_depth_256", "zero_width", "film_wide_box", "increment_past_plan", "adapt_without_moments",
                        "pass_too_large"}
    assert film_kinds == {"plain", "moments", "shard", "first_sample", "radius_0.3"}
    assert closed_with_film >= 1
    assert switch_names == {n for n, _ in mod.CALL_SWITCHES}


def test_constraint_checker_notices_what_is_missing(sessions):
    mod, work = sessions
    steps = mod.plan_session(1, work)[0][4]
    assert mod.check_constraints(steps) == []
    flat = [dict(st, depth=4) if st["kind"] == "render" else st for st in steps]
    assert any("max_depth" in m for m in mod.check_constraints(flat))
    narrow = [dict(st, radius=0.5) if st["kind"] == "render" else st for st in steps]
    assert any("filter" in m for m in mod.check_constraints(narrow))
    one_cam = [dict(st, cam=0) if "cam" in st else st for st in steps]
    assert len([m for m in mod.check_constraints(one_cam) if "camera" in m]) == 3
    no_rays = [st for st in steps if st["kind"] != "trace"]
    assert any("ray batch" in m for m in mod.check_constraints(no_rays))
    small = [dict(st, w=8, h=8, size_class="tiny") if st["kind"] == "render" else st for st in steps]
    assert any("pixels" in m for m in mod.check_constraints(small)) and any("film increment" in m for m in mod.check_constraints(small))
    one_pass = [dict(st, spp_pass=0) if st["kind"] == "render" else st for st in steps]
    assert any("samples per pass" in m for m in mod.check_constraints(one_pass))


@pytest.mark.parametrize("seed", [0, 3, 10])
def test_the_oracle_accepts_the_drawn_arguments(sessions, seed):
    """The first steps of a session through the oracle side of the tool (reduced to 24 x 18 pixels and 500 rays)."""
    mod, work = sessions
    path, name, heavy, cams, steps = mod.plan_session(seed, work)[0]
    sc = mod.spt.load_scene(path)
    placed = [mod.make_camera(c) for c in cams]
    models, n_checked = {}, 0
    for st in steps[:14]:
        small = dict(st, w=min(st.get("w", 1), 24), h=min(st.get("h", 1), 18))
        if st["kind"] in ("render", "async_pair", "async_then_sync"):
            for k in range(st["shard_count"]):
                ref = mod.oracle_film(sc, small, placed[st["cam"]], k)
                assert ref.shape == (len(mod.spt.shard_rows(small["h"], k, st["shard_count"], st["strip_rows"])), small["w"], 3)
            n_checked += 1
        elif st["kind"] == "trace":
            rays = _util.random_rays(sc, min(st["n"], 500), seed=st["ray_seed"])
            assert len(_util.oracle_trace_closest(sc, rays)) == len(rays) == len(_util.oracle_trace_any(sc, rays))
            n_checked += 1
        elif st["kind"] == "film_create":
            models[st["film"]] = mod.FilmModel(sc, small, placed[st["cam"]])
        elif st["kind"] == "film_render":
            model = models[st["film"]]
            model.add(st["n"])
            assert model.done <= model.st["spp"] and (model.counts == model.done).all()
            m, var = _util.film_mean_and_variance(model.s, model.q, model.counts)
            assert m.dtype == np.float32 and m.shape == model.s.shape
            n_checked += 1
        elif st["kind"] == "film_adapt":
            model = models[st["film"]]
            left = model.adapt(model.rel_for(st["quantile"]), st["floor"], st["min_samples"])
            assert 0 <= left <= model.active.size
    assert n_checked >= 4
    sc.close()


def test_single_samples_of_the_oracle_add_up_to_its_film():
    """oracle_render_samples gives the samples oracle_render sums: same plan, summed in order, times 1 / spp."""
    spt = _util.load_pkg()
    sc = spt.load_scene(os.path.join(_util.SCENES, "t_textured.json"))      # image textures: the auxiliary rays follow the PLAN's spp
    for sampler in (spt.SAMPLER_RANDOM, spt.SAMPLER_JITTERED, spt.SAMPLER_RECURRENCE):
        r = spt.PathTracer(max_depth=4, sampler=sampler, spp=6, division_x=3, division_y=2, seed=3)
        kw = dict(shard_index=1, shard_count=2, strip_rows=4)
        film, _ = _util.oracle_render(sc, r, 20, 14, **kw)
        xs = np.concatenate([_util.oracle_render_samples(sc, r, 20, 14, 0, 4, **kw), _util.oracle_render_samples(sc, r, 20, 14, 4, 2, **kw)])
        s = q = np.zeros_like(film)
        for x in xs:
            s, q = _util.film_add_sample(s, q, x)
        m, _ = _util.film_mean_and_variance(s, q, 6)
        assert film.max() > 0 and _util.same_words(m, film), sampler
    sc.close()
