"""What albedo films and the denoiser that takes one (spt_film_denoise_job) cost, on one MI355X.

For each workload, in one process: a 16-sample increment of an albedo film (SPT_RENDER_AOV_ALBEDO) next to a 16-sample increment
of a first-hit normal film of the same plan (SPT_RENDER_DEBUG_NORMAL, the guide spt_film_denoise had before), and a 5-iteration
spt_film_denoise_job with the albedo film alone, with both guides and with both guides and demodulation next to spt_film_denoise
with the normal guide.  Host clocks around the synchronous calls (the copy of the image to the host included), median of 5 after
one warm-up call; the increments alternate between the two films.

  python tools/albedo_cost.py [--json profiles/albedo_cost.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
spt = importlib.import_module("simple-path-tracer_amd")

import numpy as np

WORKLOADS = [
    # name, scene, camera, width, height
    ("cfg2_cube", "cfg2_cube.json", None, 1024, 1024),
    ("t_materials", "t_materials.json", "main", 512, 512),
]
INCREMENT, ITERATIONS, REPEATS = 16, 5, 5
SPP = INCREMENT * (REPEATS + 2)     # a warm-up increment, REPEATS timed ones and room for the colour film's first


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def timed(fn):
    fn()
    ms = [clock(fn) for _ in range(REPEATS)]
    return round(float(np.median(ms)), 4), [round(x, 4) for x in ms]


def run(only=None):
    out = []
    for name, scene_name, camera, w, h in WORKLOADS:
        if only and only != name:
            continue
        sc = spt.load_scene(os.path.join(ROOT, "scenes_amd", scene_name))
        r = spt.load_renderer(os.path.join(ROOT, "scenes_amd", "pt.json"), seed=1)
        r.sampler, r.spp = 0, SPP
        cfg = spt.OutputConfig(w, h, None, camera)
        with r.progressive(sc, cfg, moments=True) as film, r.guide_film(sc, cfg) as guide, r.albedo_film(sc, cfg) as albedo:
            film.render(INCREMENT)
            guide.render(INCREMENT)     # (the warm-up increments)
            albedo.render(INCREMENT)
            inc_a, inc_n = [], []
            for _ in range(REPEATS):    # alternating: whatever else the machine does meets both films
                inc_a.append(clock(lambda: albedo.render(INCREMENT)))
                inc_n.append(clock(lambda: guide.render(INCREMENT)))
            calls = {
                "denoise_normal_guide": lambda: film.denoise(guide, iterations=ITERATIONS),
                "job_albedo_only": lambda: film.denoise_job(None, albedo, iterations=ITERATIONS),
                "job_normal_and_albedo": lambda: film.denoise_job(guide, albedo, iterations=ITERATIONS),
                "job_normal_and_albedo_demodulate": lambda: film.denoise_job(guide, albedo, demodulate=True, iterations=ITERATIONS),
            }
            res = {k: timed(fn) for k, fn in calls.items()}
        sc.close()
        med = lambda xs: round(float(np.median(xs)), 4)
        wl = {"workload": "%s %dx%d, random sampler, %d-sample increments, %d iterations" % (name, w, h, INCREMENT, ITERATIONS), "name": name,
              "pixels": w * h, "albedo_increment_ms": med(inc_a), "normal_increment_ms": med(inc_n),
              "albedo_over_normal_increment": round(med(inc_a) / med(inc_n), 4)}
        for k, (m, _) in res.items():
            wl[k + "_ms"] = m
        for k in list(calls)[1:]:
            wl[k + "_over_denoise_normal_guide"] = round(res[k][0] / res["denoise_normal_guide"][0], 4)
        wl["samples_ms"] = dict({k: v[1] for k, v in res.items()}, albedo_increment=[round(x, 4) for x in inc_a],
                                normal_increment=[round(x, 4) for x in inc_n])
        print("%s: increment %.3f ms albedo, %.3f ms normal; denoise %.3f ms (normal guide), job %.3f (albedo) %.3f (both) %.3f (both, demodulated)" % (
            wl["workload"], wl["albedo_increment_ms"], wl["normal_increment_ms"], res["denoise_normal_guide"][0], res["job_albedo_only"][0],
            res["job_normal_and_albedo"][0], res["job_normal_and_albedo_demodulate"][0]))
        out.append(wl)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write this file")
    ap.add_argument("--only", default=None, help="one workload by name")
    args = ap.parse_args()
    doc = {"command": "python tools/albedo_cost.py", "workloads": run(args.only)}
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
