#!/usr/bin/env python3
"""Random call SEQUENCES on one long-lived scene, every call against the oracle, bit for bit.

tools/fuzz_scenes.py opens a fresh scene per seed and makes one call.  Here a seed opens one scene ONCE and then runs 20 - 30
drawn steps on that one device scene: renders of changing size / samples per pass / depth / filter / shard layout / camera
(fresh array, the scene's pinned buffer, an in-place film), asynchronous frames, ray batches of changing size, up to three
progressive films with their increments, adapts, reads and closes interleaved, and calls the ABI must refuse.  What is under
test is the state the scene carries from call to call (workspace, camera caches, tail_vertices, copy stream, the films
beside it), so the draw is constrained: every session has large -> tiny -> large in pixels, samples per pass, depth and
ray-batch size, a narrow filter after a wide one, cameras revisited (A -> B -> A, same eye / other axes, same camera at another
size) and a film increment right after a larger unrelated render (check_constraints).

Every step is compared with the oracle on the step's own arguments (films: the oracle's single samples summed in float32,
tests/_util.py); render statistics, which the oracle does not have, with the same call on a scene opened fresh for it.

    python tools/fuzz_sessions.py --seeds 0:40                   (needs the GPU; exit code 1, the seed and the step on any mismatch)
    FUZZ_SWITCHES=1 ...                                          (the per-call A/B switches change between the steps)

The scene and the step list of a failing seed are left in FUZZ_SESSIONS_OUT (default scenes_amd/generated/sessions/, which git
ignores; set it to whatever directory the GPU runner brings back).  tests/test_gpu_sessions.py runs a fixed list of seeds; tests/test_session_generator.py checks the draw itself without a GPU."""
import argparse
import importlib.util
import json
import os
import shutil
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _util  # noqa: E402

spt = _util.load_pkg()
SCENES = os.path.join(ROOT, "scenes_amd")
COMMITTED = ["cfg1_sphere.json", "cfg2_cube.json", "t_materials.json", "t_medium.json", "t_textured.json", "t_plastic.json",
             "t_subsurface.json", "t_pndf.json", "t_bezier.json", "t_gltf.gltf"]
N_POOL = len(COMMITTED) + 3          # three draws in thirteen: a scene of fuzz_scenes.make_scene
# the switches spt_hip.hip reads once per CALL (run_setup); the ones read at scene creation are left alone
CALL_SWITCHES = (("SPT_NO_FUSED", ["1"]), ("SPT_NO_CLASS_QUEUES", ["1"]), ("SPT_NO_LDS_TABLES", ["1"]), ("SPT_NO_TAIL_LOOP", ["1"]),
                 ("SPT_NO_PACK_FIRST", ["1"]), ("SPT_NO_PIXEL_CULL", ["1"]), ("SPT_NO_ROW_SPANS", ["1"]), ("SPT_NO_EYE_BLOB", ["1"]),
                 ("SPT_NO_OVERLAP", ["1"]), ("SPT_NO_DYN_SHADOW", ["1"]), ("SPT_NO_DYN_EXTEND", ["1"]), ("SPT_PRIMARY_CHUNKS", ["1", "2", "7"]),
                 ("SPT_BOX_BAND_BYTES", ["20000", "300000"]))
TRACE_SIZES = [0, 1, 255, 256, 257, 3000, 20000, 40000]
ORACLE_THREADS = 16
STAT_FIELDS = ("samples", "segments_closest", "segments_shadow", "primary_hits", "path_vertices", "shadow_first", "vertices_second",
               "live_samples")
VISIT_FIELDS = ("node_visits", "tri_tests", "instance_visits")

_fuzz_scenes = None


def fuzz_scenes():
    global _fuzz_scenes
    if _fuzz_scenes is None:
        spec = importlib.util.spec_from_file_location("fuzz_scenes", os.path.join(ROOT, "tools", "fuzz_scenes.py"))
        _fuzz_scenes = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_fuzz_scenes)
    return _fuzz_scenes


def stage_assets():
    return fuzz_scenes().stage_assets()


# ---- the draw ---------------------------------------------------------------------------------------------------------

def draw_scene(seed, work):
    """-> (path of the scene file, its name in the pool); a generated scene is written into `work`."""
    rng = np.random.default_rng(31000 + seed)
    k = seed % N_POOL if seed < 2 * N_POOL else int(rng.integers(0, N_POOL))     # the first seeds walk the pool in order
    if k < len(COMMITTED):
        return os.path.join(SCENES, COMMITTED[k]), COMMITTED[k].split(".")[0]
    scene = fuzz_scenes().make_scene(rng, work)
    path = os.path.join(work, "session_%d.json" % seed)
    with open(path, "w") as fh:
        json.dump(scene, fh, indent=1)
    return path, "generated"


def camera_pool(sc, rng):
    """Five placed cameras as test_screen_space_bound_with_arbitrary_cameras places them (outside, inside the bounds, looking
    past the scene, very wide) - pool entry 0 is the scene's own camera (by name).  Entries 1, 5 and 6 share the eye: the eye-relative geometry is reused,
    the row spans are not (5 differs from 1 in axes and fov, 6 in the axes alone)."""
    inst = sc.array("instances")
    lo, hi = inst["bmin"].min(axis=0).astype(np.float64), inst["bmax"].max(axis=0).astype(np.float64)
    lo, hi = np.maximum(lo, -50.0), np.minimum(hi, 50.0)       # (a huge floor plane does not push the cameras away)
    centre, ext = (lo + hi) * 0.5, float((hi - lo).max())
    try:
        sc.get_camera(None)
        pool = [{"name": None}]
    except spt.SptError:         # several cameras: the committed scenes call theirs "main"
        pool = [{"name": "main"}]

    def place(radius, aim_spread, fov, eye=None):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        e = centre + d * ext * radius if eye is None else np.asarray(eye)
        fwd = centre + rng.normal(size=3) * ext * aim_spread - e
        up = [0.0, 1.0, 0.0] if abs(fwd[1]) < 0.95 * np.linalg.norm(fwd) else [1.0, 0.0, 0.0]
        pool.append({"eye": [float(x) for x in e], "forward": [float(x) for x in fwd], "up": up, "fov": fov})

    place(2.5, 0.0, 45.0)        # 1: outside, at the scene
    place(0.15, 0.3, 90.0)       # 2: inside the bounds
    place(1.0, 1.5, 20.0)        # 3: looking past it
    place(0.6, 0.3, 150.0)       # 4: very wide
    place(0.0, 0.3, 70.0, eye=pool[1]["eye"])    # 5: the eye of 1, other axes and fov
    # 6: the eye and fov of 1, turned by a quarter of the image width: the scene stays in view at other pixels, and only the axes
    # tell the two cameras' row spans apart
    f = np.asarray(pool[1]["forward"])
    right = np.cross(f, pool[1]["up"])
    turned = f + right / np.linalg.norm(right) * np.linalg.norm(f) * 0.22
    pool.append({"eye": pool[1]["eye"], "forward": [float(x) for x in turned], "up": pool[1]["up"], "fov": 45.0})
    return pool


def make_camera(entry):
    return entry["name"] if "name" in entry else spt.make_camera(entry["eye"], entry["forward"], entry["up"], entry["fov"])


def _size(rng, cls, heavy):
    if cls == "tiny":
        return int(rng.integers(1, 21)), int(rng.integers(1, 21))
    if cls == "mid":
        return (int(rng.integers(17, 64)), int(rng.integers(9, 48))) if heavy else (int(rng.integers(17, 120)), int(rng.integers(9, 90)))
    # large: above the mid class; capped where the exhaustive oracle is slow (media, many patches)
    return (int(rng.integers(64, 97)), int(rng.integers(48, 73))) if heavy else (int(rng.integers(121, 321)), int(rng.integers(91, 241)))


def _render_plan(rng, cls, heavy, n_cams):
    w, h = _size(rng, cls, heavy)
    sampler = int(rng.integers(0, 3))
    dx, dy = int(rng.integers(1, 4)), int(rng.integers(1, 4))
    top = 3 if (heavy and cls != "tiny") else (5 if cls == "large" else 9)
    spp = dx * dy if sampler == spt.SAMPLER_JITTERED else int(rng.integers(1, top))
    if sampler == spt.SAMPLER_JITTERED and spp >= top:
        dx, dy, spp = 2, 1, 2
    divisors = [d for d in range(1, spp + 1) if spp % d == 0]
    non_divisors = [d for d in range(1, spp + 1) if spp % d] or [spp]
    spp_pass = [0, 1, divisors[int(rng.integers(0, len(divisors)))], non_divisors[int(rng.integers(0, len(non_divisors)))],
                spp + int(rng.integers(1, 5))][int(rng.integers(0, 5))]
    depth = [0, 1, int(rng.integers(2, 9)), int(rng.integers(2, 9)), int(rng.integers(2, 9))][int(rng.integers(0, 5))]
    shard_count = int(rng.choice([1, 1, 2, 3]))
    return {"kind": "render", "size_class": cls, "w": w, "h": h, "cam": int(rng.integers(0, n_cams)), "sampler": sampler, "dx": dx, "dy": dy,
            "spp": spp, "spp_pass": spp_pass, "depth": depth, "radius": float(rng.choice([0.5, 0.5, 0.5, 0.3, 1.2, 1.6])),
            "seed": int(rng.integers(0, 1 << 30)), "shard_count": shard_count, "strip_rows": int(rng.choice([1, 4, 16])),
            "debug_normal": bool(rng.random() < 0.1), "count_visits": bool(rng.random() < 0.12), "profile": bool(rng.random() < 0.08),
            "out": ["fresh", "reuse", "film"][int(rng.integers(0, 3))]}


def _pass_of(st):
    """The samples one pass of the step covers, as grow_workspace sizes it for these small images."""
    return min(st["spp_pass"] or st["spp"], st["spp"])


def draw_steps(seed, heavy, n_cams=7):
    """The step list of a seed (plain dicts; a pure function of the seed and `heavy`)."""
    for attempt in range(100):
        steps = _draw_steps(np.random.default_rng([seed, attempt, 77]), heavy, n_cams, seed)
        if not check_constraints(steps):
            return steps
    raise RuntimeError("seed %d: no step list satisfies the constraints: %s" % (seed, check_constraints(steps)))


def _draw_steps(rng, heavy, n_cams, seed):
    # renders first: their classes and the attributes the constraints speak of follow forced patterns at drawn positions,
    # everything else about them is random
    n_r = int(rng.integers(9, 12))
    classes = [["tiny", "mid", "mid", "large"][int(rng.integers(0, 4))] for _ in range(n_r)]
    a, b, c = sorted(rng.choice(n_r, 3, replace=False))
    classes[a], classes[b], classes[c] = "large", "tiny", "large"
    renders = [_render_plan(rng, cls, heavy, n_cams) for cls in classes]

    def force_spp(st, spp):
        if st["sampler"] == spt.SAMPLER_JITTERED:
            st["dx"], st["dy"] = (spp, 1) if spp < 6 else (3, 2)
            spp = st["dx"] * st["dy"]
        st["spp"] = spp

    others = [k for k in range(n_r) if k not in (a, c)]
    d, e, f = sorted(rng.choice(others, 3, replace=False))          # samples per pass: 6 or more, then 1 of several, then 6 or more
    for k, (spp, pas) in ((d, (6, 0)), (e, (4, 1)), (f, (8, 6))):
        if classes[k] == "large":                                   # (many samples: not on the largest images)
            renders[k] = _render_plan(rng, "mid", heavy, n_cams)
            classes[k] = "mid"
        force_spp(renders[k], spp)
        renders[k]["spp_pass"] = pas
    g, h_, i = sorted(rng.choice(n_r, 3, replace=False))            # depth 8, then 0 or 1, then 8
    renders[g]["depth"], renders[h_]["depth"], renders[i]["depth"] = 8, int(rng.integers(0, 2)), 8
    wide, narrow = sorted(rng.choice(n_r, 2, replace=False))        # a narrow filter after a wide one
    renders[wide]["radius"], renders[narrow]["radius"] = float(rng.choice([1.2, 1.6])), float(rng.choice([0.3, 0.5]))
    # cameras: 1, then 6 (same eye and fov, turned) at the same size, then 1 again at another size, then 5 (same eye, other fov) at that size
    j = int(rng.integers(0, n_r - 3))
    for k, cam in enumerate((1, 6, 1, 5)):
        renders[j + k]["cam"] = cam
    renders[j + 1]["w"], renders[j + 1]["h"] = renders[j]["w"], renders[j]["h"]
    renders[j + 1]["debug_normal"] = True        # (normals, not radiance: every hit shows, lit or not)
    if (renders[j + 2]["w"], renders[j + 2]["h"]) == (renders[j]["w"], renders[j]["h"]):
        renders[j + 2]["w"] += 1
    renders[j + 3]["w"], renders[j + 3]["h"] = renders[j + 2]["w"], renders[j + 2]["h"]
    for st in renders:
        if st["radius"] > 1.0 and heavy and st["size_class"] == "large":
            st["spp"] = min(st["spp"], 2)       # a wide filter keeps every sample of the band's neighbour rows too
            if st["sampler"] == spt.SAMPLER_JITTERED:
                st["dx"], st["dy"], st["spp"] = 2, 1, 2
            st["spp_pass"] = min(st["spp_pass"], st["spp"] + 1)

    # two of the renders become asynchronous steps (radius 0.5 or 0.3: one band, the copy-out is the frame's last command)
    free = [k for k in range(n_r) if k not in (a, b, c, d, e, f, g, h_, i, wide, narrow, j, j + 1, j + 2, j + 3)]
    for kind in ("async_pair", "async_then_sync"):
        k = free.pop(int(rng.integers(0, len(free)))) if free else None
        if k is None:
            renders.append(_render_plan(rng, "mid", heavy, n_cams))
            k = len(renders) - 1
        st = renders[k]
        st.update(kind=kind, out="reuse", count_visits=False, profile=False)
        if st["radius"] > 1.0:
            st["radius"] = 0.5
        if kind == "async_then_sync":
            other = _render_plan(rng, "mid" if st["size_class"] != "mid" else "tiny", heavy, n_cams)
            other.update(cam=(st["cam"] + 1 + int(rng.integers(0, n_cams - 1))) % n_cams, out="fresh", count_visits=False, profile=False)
            st["then"] = other

    # ray batches: sizes go up and down, 40 000 -> 1 -> 20 000 among them
    sizes = [TRACE_SIZES[int(rng.integers(0, len(TRACE_SIZES)))] for _ in range(int(rng.integers(1, 4)))]
    t0 = int(rng.integers(0, len(sizes) + 1))
    sizes[t0:t0] = [40000, 1, 20000] if rng.random() < 0.5 else [20000, 0, 1, 40000]
    traces = [{"kind": "trace", "n": (min(n, 6000) if heavy else n), "ray_seed": int(rng.integers(0, 1 << 30))} for n in sizes]

    # films: two or three, opened at drawn points, their steps drawn while the list is merged
    n_films = int(rng.integers(2, 4))
    films = []
    for fid in range(n_films):
        kind = ["plain", "moments", "moments", "shard", "first_sample"][int(rng.integers(0, 5))] if fid else "moments"
        w, h = _size(rng, "tiny" if (heavy or rng.random() < 0.3) else "mid", heavy)
        if fid == 0:
            w, h = (int(rng.integers(17, 49)), int(rng.integers(9, 33)))      # smaller than any large render
        sampler = int(rng.integers(0, 3))
        spp = [4, 6, 9, 12][int(rng.integers(0, 4))] if not heavy else [4, 6][int(rng.integers(0, 2))]
        dx, dy = {4: (2, 2), 6: (3, 2), 9: (3, 3), 12: (4, 3)}[spp]
        radius = 0.5 if (kind == "moments" or rng.random() < 0.7) else 0.3
        fs = {"kind": "film_create", "film": fid, "w": w, "h": h, "cam": int(rng.integers(0, n_cams)), "sampler": sampler, "dx": dx, "dy": dy,
              "spp": spp, "depth": int(rng.integers(1, 7)), "radius": radius, "seed": int(rng.integers(0, 1 << 30)),
              "moments": kind == "moments" or (kind != "plain" and bool(rng.random() < 0.5)),
              "spp_pass": [0, 0, 1, 5][int(rng.integers(0, 4))], "first_sample": int(rng.integers(1, spp - 1)) if kind == "first_sample" else 0,
              "shard_index": 0, "shard_count": 1, "strip_rows": 16, "debug_normal": False}
        if kind == "shard":
            fs["strip_rows"] = int(rng.choice([1, 4]))
            fs["shard_count"] = int(rng.integers(2, 4))
            n_strips = (h + fs["strip_rows"] - 1) // fs["strip_rows"]
            fs["shard_index"] = int(rng.integers(0, min(fs["shard_count"], n_strips)))
        films.append(fs)

    # merge: renders and traces keep their order; film steps and refused calls are drawn in between
    body = [("r", k) for k in range(len(renders))]
    for k, _ in enumerate(traces):
        body.insert(int(rng.integers(0, len(body) + 1)), ("t", k))
    t_order = iter(range(len(traces)))
    body = [(kind, next(t_order)) if kind == "t" else (kind, k) for kind, k in body]
    refusals = ["jittered_mismatch", "max_depth_256", "zero_width", "film_wide_box", "increment_past_plan", "adapt_without_moments",
                "pass_too_large"]
    rng.shuffle(refusals)
    refusals = refusals[: int(rng.integers(2, 4))]
    if "pass_too_large" not in refusals and seed % 2 == 0:
        refusals.append("pass_too_large")
    open_at = sorted(int(x) for x in rng.choice(max(len(body) - 4, 1), n_films, replace=True))
    open_at[0] = min(open_at[0], max(0, min(k for k, (kind, idx) in enumerate(body) if kind == "r" and renders[idx]["size_class"] == "large") - 1))
    open_at.sort()
    live = {}          # film id -> its model of the generator: samples left, covered, flags
    steps = []

    def film_step(fid, after_large=False):
        fl = live[fid]
        fs = films[fid]
        left = fs["spp"] - fs["first_sample"] - fl["done"]
        roll = rng.random()
        if after_large and left > 0:
            roll = 0.0
        if roll < 0.45 and left > 0:
            n = int(rng.integers(1, min(left, 4) + 1))
            fl["done"] += n
            steps.append({"kind": "film_render", "film": fid, "n": n, "after_larger_render": bool(after_large)})
        elif roll < 0.6 and fs["moments"] and fs["radius"] == 0.5 and fl["done"] >= 2:
            steps.append({"kind": "film_adapt", "film": fid, "quantile": float(rng.choice([0.2, 0.4, 0.7])), "floor": float(rng.choice([0.0, 1e-3])),
                          "min_samples": int(rng.choice([0, 2, 4]))})
            fl["adapted"] = True
        elif fl["done"] > 0 or roll > 0.8:
            what = ["sum", "counts"]
            if fl["done"] > 0 and (fs["radius"] == 0.5 or (left == 0 and fs["first_sample"] == 0)):
                what.append("mean")       # (radius 0.3: the mean's divisor needs the sample offsets; checked when the film is complete)
            if fs["moments"]:
                what.append("sum_sq")
                if fs["radius"] == 0.5 and fl["done"] > 0:
                    what.append("variance_of_mean")
            steps.append({"kind": "film_read", "film": fid, "what": what})
        elif left > 0:
            fl["done"] += 1
            steps.append({"kind": "film_render", "film": fid, "n": 1, "after_larger_render": False})

    n_opened = 0
    for pos, (kind, idx) in enumerate(body):
        while n_opened < n_films and open_at[n_opened] <= pos:
            steps.append(films[n_opened])
            live[n_opened] = {"done": 0}
            n_opened += 1
        st = renders[idx] if kind == "r" else traces[idx]
        steps.append(st)
        larger = [fid for fid in live if kind == "r" and st["kind"] == "render" and st["w"] * st["h"] > films[fid]["w"] * films[fid]["h"]]
        if larger and rng.random() < 0.8:
            film_step(larger[int(rng.integers(0, len(larger)))], after_large=True)
        for _ in range(int(rng.integers(0, 2))):
            if live:
                film_step(list(live)[int(rng.integers(0, len(live)))])
        if refusals and rng.random() < 0.45:
            steps.append({"kind": "refused", "which": refusals.pop()})
        for fid in list(live):
            fs, fl = films[fid], live[fid]
            if fl["done"] == fs["spp"] - fs["first_sample"] and rng.random() < 0.5:
                film_step(fid)      # usually a read of the complete film
                steps.append({"kind": "film_close", "film": fid})
                del live[fid]
    for w in refusals:
        steps.append({"kind": "refused", "which": w})
    for fid in list(live):
        if live[fid]["done"] > 0:
            steps.append({"kind": "film_read", "film": fid, "what": ["sum", "counts"]})
    keep_open = seed % 3 == 0 and live       # the scene is closed with a film still open
    for fid in list(live)[1 if keep_open else 0:]:
        steps.append({"kind": "film_close", "film": fid})
    steps.append({"kind": "close_scene", "open_films": list(live)[:1] if keep_open else []})
    return steps


def draw_switches(seed, steps):
    """FUZZ_SWITCHES=1: the per-call switches in force at each render / film step (a stream of its own: the step list of a
    seed is the same with and without switches)."""
    rng = np.random.default_rng([seed, 4242])
    out = []
    for st in steps:
        env = {}
        if st["kind"] in ("render", "async_pair", "async_then_sync", "film_create", "film_render", "film_adapt", "film_read"):
            for name, values in CALL_SWITCHES:
                if rng.random() < 0.2:
                    env[name] = values[int(rng.integers(0, len(values)))]
        out.append(env)
    # by construction: the class queues off and on again between two renders in a row (hit_f4 / qa[1] change size), the eye copy
    # used, skipped and used again
    rs = [k for k, st in enumerate(steps) if st["kind"] in ("render", "async_pair", "async_then_sync")]
    i, j = int(rng.integers(0, len(rs) - 1)), int(rng.integers(0, len(rs) - 2))
    out[rs[i]]["SPT_NO_CLASS_QUEUES"] = "1"
    out[rs[i + 1]].pop("SPT_NO_CLASS_QUEUES", None)
    out[rs[j]].pop("SPT_NO_EYE_BLOB", None)
    out[rs[j + 1]]["SPT_NO_EYE_BLOB"] = "1"
    out[rs[j + 2]].pop("SPT_NO_EYE_BLOB", None)
    return out


def check_constraints(steps):
    """-> the list of ordering constraints the step list misses (empty: all hold)."""
    missing = []

    def up_down_up(values, big, small, name):
        first_big = next((k for k, v in enumerate(values) if big(v)), None)
        ok = first_big is not None and any(small(v) and any(big(x) for x in values[k + 1:]) for k, v in enumerate(values) if k > first_big)
        if not ok:
            missing.append(name + ": large, then tiny, then large")

    rs = [st for st in steps if st["kind"] == "render"]
    px = [st["w"] * st["h"] for st in rs]
    tiny_px = [p for st, p in zip(rs, px) if st["size_class"] == "tiny"]
    if tiny_px:
        up_down_up(list(zip(px, (st["size_class"] for st in rs))), lambda v: v[1] == "large" and v[0] >= 7 * max(tiny_px), lambda v: v[1] == "tiny", "pixels")
    else:
        missing.append("pixels: no tiny render")
    up_down_up([(_pass_of(st), st["spp"]) for st in rs], lambda v: v[0] >= 6, lambda v: v[0] == 1 and v[1] > 1, "samples per pass")
    up_down_up([st["depth"] for st in rs], lambda v: v == 8, lambda v: v <= 1, "max_depth")
    up_down_up([st["n"] for st in steps if st["kind"] == "trace"], lambda v: v >= 6000, lambda v: v <= 1, "ray batch")
    if not any(st["radius"] > 1.0 and any(x["radius"] <= 0.5 for x in rs[k + 1:]) for k, st in enumerate(rs)):
        missing.append("a narrow filter after a wide one")
    seq = [(st["cam"], st["w"], st["h"]) for st in steps if st["kind"] in ("render", "async_pair", "async_then_sync")]
    if not any(seq[k][0] == seq[k + 2][0] != seq[k + 1][0] for k in range(len(seq) - 2)):
        missing.append("cameras A -> B -> A")
    if not any({seq[k][0], seq[k + 1][0]} == {1, 5} and seq[k][1:] == seq[k + 1][1:] for k in range(len(seq) - 1)):
        missing.append("two cameras with the same eye in a row at one size")
    if not any({seq[k][0], seq[k + 1][0]} == {1, 6} and seq[k][1:] == seq[k + 1][1:] for k in range(len(seq) - 1)):
        missing.append("two cameras with the same eye and fov in a row at one size")
    if not any(x[0] == y[0] and x[1:] != y[1:] for k, x in enumerate(seq) for y in seq[k + 1:]):
        missing.append("one camera at two image sizes")
    films = {st["film"]: st for st in steps if st["kind"] == "film_create"}
    if not any(st["kind"] == "film_render" and steps[k - 1]["kind"] == "render" and
               steps[k - 1]["w"] * steps[k - 1]["h"] > films[st["film"]]["w"] * films[st["film"]]["h"] for k, st in enumerate(steps) if k):
        missing.append("a film increment right after a larger unrelated render")
    for kind in ("render", "async_pair", "async_then_sync", "trace", "film_create", "film_render", "film_read", "film_close", "refused"):
        if not any(st["kind"] == kind for st in steps):
            missing.append("no %s step" % kind)
    return missing


# ---- running a session --------------------------------------------------------------------------------------------------

class Mismatch(Exception):
    pass


def _renderer(st):
    return spt.PathTracer(max_depth=st["depth"], sampler=st["sampler"], spp=st["spp"], division_x=st["dx"], division_y=st["dy"], seed=st["seed"],
                          filter_radius=st["radius"], debug_normal=st.get("debug_normal", False))


def oracle_film(sc, st, cam, k, flags=None):
    ref, _ = _util.oracle_render(sc, _renderer(st), st["w"], st["h"], camera=cam, flags=_util.device_oracle_flags() if flags is None else flags,
                                 threads=ORACLE_THREADS, shard_index=k, shard_count=st["shard_count"], strip_rows=st["strip_rows"])
    return ref


def _expect(got, ref, what):
    if not _util.same_words(got, ref):
        if got.shape != ref.shape:
            raise Mismatch("%s: shape %s, the oracle's %s" % (what, got.shape, ref.shape))
        if got.dtype == np.float32:
            nan = np.isnan(ref)
            n = int((got.view(np.uint32) != ref.view(np.uint32))[~nan].sum()) + int((nan != np.isnan(got)).sum())
        else:
            n = int((got != ref).sum())
        raise Mismatch("%s: %d of %d words differ from the oracle's" % (what, n, ref.size))


class FilmModel:
    """What a progressive film must hold: the oracle's single samples of its plan, summed in float32 in sample order for the
    pixels that are still active (tests/_util.py: film_add_sample, film_criterion, film_mean_and_variance)."""

    def __init__(self, sc, st, cam):
        self.sc, self.st, self.cam = sc, st, cam
        self.rows = len(spt.shard_rows(st["h"], st["shard_index"], st["shard_count"], st["strip_rows"]))
        shape = (self.rows, st["w"], 3)
        self.s, self.q = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
        self.active = np.ones(shape[:2], bool)
        self.counts = np.zeros(shape[:2], np.uint32)
        self.done = 0

    def add(self, n):
        st = self.st
        xs = _util.oracle_render_samples(self.sc, _renderer(st), st["w"], st["h"], st["first_sample"] + self.done, n, camera=self.cam,
                                         flags=_util.device_oracle_flags(), threads=ORACLE_THREADS, shard_index=st["shard_index"],
                                         shard_count=st["shard_count"], strip_rows=st["strip_rows"])
        for x in xs:
            self.s, self.q = _util.film_add_sample(self.s, self.q, x, self.active)
        self.done += n
        self.counts[self.active] = self.done

    def rel_for(self, quantile):
        """A relative tolerance that retires about `quantile` of the noisy active pixels (as tests/test_gpu_adaptive.py picks it)."""
        n = self.done
        m = self.s.astype(np.float64) / n
        v = np.maximum((self.q.astype(np.float64) / n - m * m) / (n - 1), 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            need = np.max(np.sqrt(v) / np.abs(m), axis=-1)
        need = need[self.active & np.isfinite(need) & (need > 0)]
        return float(np.float32(np.quantile(need, quantile))) if need.size else 0.0

    def adapt(self, rel, floor, min_samples):
        if self.done >= max(min_samples, 2):
            self.active &= ~_util.film_criterion(self.s, self.q, self.done, rel, floor)
        return int(self.active.sum())

    def expected(self, what):
        if what == "sum":
            return self.s
        if what == "sum_sq":
            return self.q
        if what == "counts":
            return self.counts
        st = self.st
        if what == "mean" and st["radius"] != 0.5:     # complete, first_sample 0: the one-call film of the plan
            plan = dict(st)
            return oracle_film(self.sc, plan, self.cam, st["shard_index"])
        m, var = _util.film_mean_and_variance(self.s, self.q, self.counts)
        return m if what == "mean" else var


def _refused(call, status, prefix, what):
    try:
        call()
    except spt.SptError as e:
        if e.status != status or not e.message.startswith(prefix):
            raise Mismatch("%s: refused with status %d %r, expected %d and a message naming %r" % (what, e.status, e.message, status, prefix))
        last = spt.hip_lib().spt_last_error()
        last = last.decode() if isinstance(last, bytes) else str(last)
        if not last.startswith(prefix):
            raise Mismatch("%s: spt_last_error() is %r" % (what, last))
        return
    raise Mismatch("%s: the call was not refused" % what)


def _stats_of(r):
    s = r.last_stats
    return {f: int(getattr(s, f)) for f in STAT_FIELDS + VISIT_FIELDS}


class Session:
    def __init__(self, path, cams):
        self.path = path
        self.sc = spt.load_scene(path)
        self.ds = self.sc.device_scene(0)
        self.cams = [make_camera(c) for c in cams]
        self.films, self.models = {}, {}

    # every render form: all the step's shards, each against the oracle
    def render(self, st, wait=True, sc=None):
        sc = sc or self.sc
        r, cam = _renderer(st), self.cams[st["cam"]]
        cfg = spt.OutputConfig(st["w"], st["h"], None, cam)
        kw = dict(shard_count=st["shard_count"], strip_rows=st["strip_rows"], samples_per_pass=st["spp_pass"])
        stats = []
        full = np.full((st["h"], st["w"], 3), -1.0, dtype=np.float32) if st["out"] == "film" else None
        for k in range(st["shard_count"]):
            got = r.render_shard(sc, cfg, shard_index=k, profile=st["profile"], count_visits=st["count_visits"], reuse_output=st["out"] == "reuse",
                                 film=full, **kw)
            stats.append(_stats_of(r))
            if full is None:
                _expect(got.copy(), oracle_film(self.sc, st, cam, k), "render %dx%d shard %d of %d" % (st["w"], st["h"], k, st["shard_count"]))
        if full is not None:
            ref = np.full_like(full, -1.0)
            for k in range(st["shard_count"]):
                ref[spt.shard_rows(st["h"], k, st["shard_count"], st["strip_rows"])] = oracle_film(self.sc, st, cam, k)
            _expect(full, ref, "render %dx%d in place, %d shards" % (st["w"], st["h"], st["shard_count"]))
        return stats

    def twin(self, st, stats):
        """Render statistics are not the oracle's to give: the same call on a scene opened fresh for it must count the same
        (history independence, not correctness)."""
        fresh = spt.load_scene(self.path)
        try:
            r, cam = _renderer(st), self.cams[st["cam"]]
            for k in range(st["shard_count"]):
                r.render_shard(fresh, spt.OutputConfig(st["w"], st["h"], None, cam), shard_index=k, shard_count=st["shard_count"],
                               strip_rows=st["strip_rows"], samples_per_pass=st["spp_pass"], profile=st["profile"], count_visits=st["count_visits"])
                want = _stats_of(r)
                fields = STAT_FIELDS + (VISIT_FIELDS if st["count_visits"] else ())
                bad = [f for f in fields if want[f] != stats[k][f]]
                if bad:
                    raise Mismatch("render statistics of shard %d differ from a fresh scene's: %s" %
                                   (k, ", ".join("%s %d / %d" % (f, stats[k][f], want[f]) for f in bad)))
        finally:
            fresh.close()

    def async_frames(self, st):
        r, cam = _renderer(st), self.cams[st["cam"]]
        cfg = spt.OutputConfig(st["w"], st["h"], None, cam)
        for k in range(st["shard_count"]):
            kw = dict(shard_index=k, shard_count=st["shard_count"], strip_rows=st["strip_rows"], samples_per_pass=st["spp_pass"], reuse_output=True)
            if st["kind"] == "async_pair":      # the frame queued twice, as tools/fuzz_scenes.py does
                for _ in range(2):
                    got = r.render_shard(self.sc, cfg, wait=False, **kw)
            else:                               # one frame in flight, a synchronous render with another camera and size behind it
                got = r.render_shard(self.sc, cfg, wait=False, **kw)
                if k == 0:
                    self.render(st["then"])
            r.wait(self.sc)
            _expect(got.copy(), oracle_film(self.sc, st, cam, k), "%s %dx%d shard %d" % (st["kind"], st["w"], st["h"], k))

    def trace(self, st):
        rays = _util.random_rays(self.sc, st["n"], seed=st["ray_seed"])
        flags = _util.device_oracle_flags()
        got_h, got_o = self.ds.trace_closest(rays), self.ds.trace_any(rays)
        if os.environ.get("SPT_REFERENCE_BVH"):
            return      # coincident surfaces make a few hits visit-order dependent in that mode (tests/test_gpu_parity.py)
        if _util.oracle_trace_closest(self.sc, rays, flags).tobytes() != got_h.tobytes():
            raise Mismatch("trace_closest of %d rays differs from the oracle's" % st["n"])
        _expect(got_o, _util.oracle_trace_any(self.sc, rays, flags), "trace_any of %d rays" % st["n"])

    def film_create(self, st):
        r, cam = _renderer(st), self.cams[st["cam"]]
        self.films[st["film"]] = r.progressive(self.sc, spt.OutputConfig(st["w"], st["h"], None, cam), first_sample=st["first_sample"],
                                               moments=st["moments"], shard_index=st["shard_index"], shard_count=st["shard_count"],
                                               strip_rows=st["strip_rows"], samples_per_pass=st["spp_pass"])
        self.models[st["film"]] = FilmModel(self.sc, st, cam)

    def film_step(self, st):
        film, model = self.films[st["film"]], self.models[st["film"]]
        if st["kind"] == "film_render":
            film.render(st["n"])
            model.add(st["n"])
            if film.samples != model.done:
                raise Mismatch("film %d covers %d samples, expected %d" % (st["film"], film.samples, model.done))
            _expect(film.sum(), model.s, "film %d: sums after %d samples" % (st["film"], model.done))
        elif st["kind"] == "film_adapt":
            rel = model.rel_for(st["quantile"])
            got = film.adapt(rel, st["floor"], st["min_samples"])
            want = model.adapt(rel, st["floor"], st["min_samples"])
            if got != want:
                raise Mismatch("film %d: adapt left %d pixels active, the criterion %d" % (st["film"], got, want))
            _expect(film.sample_counts(), model.counts, "film %d: counts after adapt" % st["film"])
        elif st["kind"] == "film_read":
            reads = {"sum": film.sum, "sum_sq": film.sum_sq, "mean": film.mean, "variance_of_mean": film.variance_of_mean, "counts": film.sample_counts}
            for what in st["what"]:
                _expect(reads[what](), model.expected(what), "film %d: %s at %d samples" % (st["film"], what, model.done))
        else:
            film.close()
            del self.films[st["film"]], self.models[st["film"]]

    def refused(self, st):
        which = st["which"]
        base = {"kind": "render", "w": 40, "h": 30, "cam": 0, "sampler": 0, "dx": 0, "dy": 0, "spp": 4, "spp_pass": 0, "depth": 4, "radius": 0.5,
                "seed": 1, "shard_count": 1, "strip_rows": 16}

        def render(**kw):
            plan = dict(base, **kw)
            return lambda: _renderer(plan).render_shard(self.sc, spt.OutputConfig(plan["w"], plan["h"], None, self.cams[0]), samples_per_pass=plan["spp_pass"])

        if which == "jittered_mismatch":
            _refused(render(sampler=spt.SAMPLER_JITTERED, dx=2, dy=3, spp=5), 1, "render:", which)
        elif which == "max_depth_256":
            _refused(render(depth=256), 4, "render:", which)
        elif which == "zero_width":
            _refused(render(w=0), 1, "render:", which)
        elif which == "pass_too_large":
            # 100 x 80 pixels: one tile per queue shard, 64 shards x 256 lanes x 2^18 samples = 2^32 queue entries; grow_workspace
            # refuses before it allocates anything
            _refused(render(w=100, h=80, spp=1 << 18, spp_pass=1 << 18), 4, "render: pass too large", which)
        elif which == "film_wide_box":
            plan = dict(base, radius=1.2)
            _refused(lambda: _renderer(plan).progressive(self.sc, spt.OutputConfig(40, 30, None, self.cams[0])), 4, "film_create:", which)
        else:
            plan = dict(base, w=16, h=16, film=-1, first_sample=0, shard_index=0, moments=False)
            with _renderer(plan).progressive(self.sc, spt.OutputConfig(16, 16, None, self.cams[0])) as film:
                model = FilmModel(self.sc, plan, self.cams[0])
                film.render(3)
                model.add(3)
                if which == "increment_past_plan":
                    _refused(lambda: film.render(2), 1, "film_render:", which)
                else:
                    _refused(lambda: film.adapt(0.1), 1, "film_adapt:", which)
                if film.samples != 3:
                    raise Mismatch("%s: the refused call changed the film's sample count" % which)
                _expect(film.sum(), model.s, "%s: the film after the refused call" % which)
                _expect(film.sample_counts(), model.counts, "%s: the film's counts after the refused call" % which)

    def close(self, st=None):
        held = [self.films[fid] for fid in (st["open_films"] if st else [])]
        for fid, film in list(self.films.items()):
            if film not in held:
                film.close()
        self.sc.close()
        for film in held:
            try:
                film.render(1)
            except spt.SptError:
                continue
            raise Mismatch("a film of a closed scene still took samples")
        self.films.clear()


def run_step(session, st):
    """Runs one step on the session and compares it (raises Mismatch); True when the step closed the scene."""
    kind = st["kind"]
    if kind == "render":
        stats = session.render(st)
        if st["count_visits"] or st["profile"]:
            session.twin(st, stats)
    elif kind in ("async_pair", "async_then_sync"):
        session.async_frames(st)
    elif kind == "trace":
        session.trace(st)
    elif kind == "film_create":
        session.film_create(st)
    elif kind.startswith("film_"):
        session.film_step(st)
    elif kind == "refused":
        session.refused(st)
    else:
        session.close(st)
        return True
    return False


def render_step(w, h, cam=0, **kw):
    """A render step written by hand (tests): random sampler, 4 spp, depth 5, radius 0.5, one shard, a fresh output array."""
    st = {"kind": "render", "size_class": "mid", "w": w, "h": h, "cam": cam, "sampler": 0, "dx": 0, "dy": 0, "spp": 4, "spp_pass": 0, "depth": 5,
          "radius": 0.5, "seed": 7, "shard_count": 1, "strip_rows": 16, "debug_normal": False, "count_visits": False, "profile": False, "out": "fresh"}
    st.update(kw)
    return st


def film_step_create(film, w, h, cam=0, **kw):
    st = render_step(w, h, cam, spp=8, **kw)
    st.update(kind="film_create", film=film, moments=st.get("moments", True), first_sample=st.get("first_sample", 0), shard_index=st.get("shard_index", 0))
    return st


def plan_session(seed, work):
    """-> (scene path, scene name, heavy, camera pool, steps), or None with a reason when the loader rejects the scene.
    Needs no GPU: the host loader places the cameras."""
    path, name = draw_scene(seed, work)
    try:
        sc = spt.load_scene(path)
    except spt.SptError as e:
        return None, "scene rejected by the loader: %s" % str(e)[:120]
    heavy = sc.desc.n_mediums > 0 or sc.desc.n_bezier_patches > 40
    cams = camera_pool(sc, np.random.default_rng([seed, 99]))
    sc.close()
    return (path, name, heavy, cams, draw_steps(seed, heavy, len(cams))), None


def run_session(seed, work, switches=None):
    """-> (ok or None when the loader rejected the scene, one-line description).  On a mismatch the scene and the step list go
    to the directory FUZZ_SESSIONS_OUT names (see the module docstring)."""
    if switches is None:
        switches = bool(os.environ.get("FUZZ_SWITCHES"))
    plan, why = plan_session(seed, work)
    if plan is None:
        return None, why
    path, name, heavy, cams, steps = plan
    envs = draw_switches(seed, steps) if switches else [{} for _ in steps]
    names = [n for n, _ in CALL_SWITCHES]
    saved = {n: os.environ.get(n) for n in names}
    for n in names:
        os.environ.pop(n, None)          # the scene is created without them (SPT_NO_EYE_BLOB is also read there)
    t0 = time.time()
    session, k, failure = None, -1, None
    try:
        session = Session(path, cams)
        for k, (st, env) in enumerate(zip(steps, envs)):
            for n in names:
                os.environ.pop(n, None)
            os.environ.update(env)
            if run_step(session, st):
                session = None
    except (Mismatch, spt.SptError, AssertionError) as e:
        failure = "step %d (%s): %s" % (k, json.dumps(steps[k])[:300], str(e)[:300])
    finally:
        try:
            if session is not None:
                session.close()
        finally:
            for n, v in saved.items():
                os.environ.pop(n, None)
                if v is not None:
                    os.environ[n] = v
    kinds = {}
    for st in steps:
        kinds[st["kind"]] = kinds.get(st["kind"], 0) + 1
    info = "%s  %-12s %s%2d steps (%s)  %.1f s" % ("FAIL" if failure else "ok  ", name, "heavy " if heavy else "", len(steps),
                                                  " ".join("%s %d" % (k2[:12], v) for k2, v in sorted(kinds.items())), time.time() - t0)
    if failure:
        info += "  " + failure
        out_dir = os.environ.get("FUZZ_SESSIONS_OUT") or os.path.join(SCENES, "generated", "sessions")
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "session_%d%s.json" % (seed, "_switches" if switches else "")), "w") as fh:
            json.dump({"seed": seed, "scene": name, "switches": envs, "cameras": cams, "steps": steps, "failure": failure}, fh, indent=1)
        if name == "generated":
            shutil.copy(path, os.path.join(out_dir, os.path.basename(path)))
    return failure is None, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", default="0:20")
    args = ap.parse_args()
    lo, hi = (int(x) for x in args.seeds.split(":"))
    work = stage_assets()
    bad, t0 = [], time.time()
    for seed in range(lo, hi):
        ok, info = run_session(seed, work)
        print("seed %4d: %s" % (seed, info), flush=True)
        if ok is False:
            bad.append(seed)
            if "SPT_ERR_HIP" in info:       # the device reported an error: nothing more is started on it
                break
    shutil.rmtree(work, ignore_errors=True)
    print("%d of %d seeds failed %s in %.0f s" % (len(bad), hi - lo, bad, time.time() - t0))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
