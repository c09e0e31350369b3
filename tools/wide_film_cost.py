"""What a film that keeps its samples costs (SPT_FILM_KEEP_SAMPLES): cfg2_cube at 1024x1024, 64 spp, box radius 1.0 (and 2.2).

The yardstick is one synchronous spt_render of the plan with SPT_RENDER_PROFILE: its total and its kernel_ms[SPT_K_RESOLVE], which
is k_filter_box over the same (2R+1)^2 * spp samples per pixel.  The film takes the plan as 4 x 16 samples.  Recorded per
increment: the host clock around the synchronous spt_film_render (the store's allocation and the redundant halo included); after
each increment, spt_film_read(MEAN) as the device time of its kernels (spt_debug_render_info) and as the host clock around the
whole call.  Host clocks around synchronised calls after a warm-up; the median of
`--reps` repetitions, the spread (min, max) beside it.  Every full film's mean is checked against spt_render's, bit for bit.

  python tools/wide_film_cost.py [--reps 5] [--json profiles/wide_film_cost.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
spt = importlib.import_module("simple-path-tracer_amd")

import numpy as np

K_RESOLVE = 4   # SPT_K_RESOLVE


def stat(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--increments", type=int, default=4)
    ap.add_argument("--json", default=None, help="also write the result here")
    args = ap.parse_args()
    assert spt.device_count() >= 1, "needs an MI355X"
    scene = spt.load_scene(os.path.join(ROOT, "scenes_amd", "cfg2_cube.json"))
    ds = scene.device_scene(0)
    cfg = spt.OutputConfig(args.width, args.height)
    inc = args.spp // args.increments
    result = {"workload": "cfg2_cube %dx%d @ %d spp as %d x %d" % (args.width, args.height, args.spp, args.increments, inc), "reps": args.reps, "radii": {}}
    for radius in (1.0, 2.2):
        r = spt.load_renderer(os.path.join(ROOT, "scenes_amd", "pt.json"), seed=1)
        r.spp = args.spp
        r.filter_radius = radius
        R = int(np.ceil(np.float32(radius) - np.float32(0.5)))
        for _ in range(2):
            ref = r.render_shard(scene, cfg, reuse_output=True)
        ref = ref.copy()
        total, resolve, wall = [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            r.render_shard(scene, cfg, reuse_output=True, profile=True)
            wall.append((time.perf_counter() - t0) * 1e3)
            total.append(r.last_stats.gpu_ms)
            resolve.append(r.last_stats.kernel_ms[K_RESOLVE])
        row = {"R": R, "spt_render": {"gpu_ms": stat(total), "k_filter_box_ms": stat(resolve), "call_ms": stat(wall)},
               "store_bytes": args.width * args.height * args.spp * 12}

        def film_run():
            out = {"render_ms": [], "read_kernel_ms": [], "read_call_ms": []}
            with r.progressive(scene, cfg, keep_samples=True) as film:
                for _ in range(args.increments):
                    t0 = time.perf_counter()
                    film.render(inc)
                    out["render_ms"].append((time.perf_counter() - t0) * 1e3)
                    film.mean()   # warm-up of the read-out at this sample count
                    t0 = time.perf_counter()
                    got = film.mean()
                    out["read_call_ms"].append((time.perf_counter() - t0) * 1e3)
                    out["read_kernel_ms"].append(ds.render_info(2) * 1e-6)
                assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), radius
            return out

        film_run()   # warm-up
        runs = [film_run() for _ in range(args.reps)]
        row["film"] = {key: {"done_%d" % ((k + 1) * inc): stat([run[key][k] for run in runs]) for k in range(args.increments)} for key in runs[0]}
        # the bar: the read-out kernel at the full sample count against k_filter_box, which does the same additions
        k = row["film"]["read_kernel_ms"]["done_%d" % args.spp]
        spread = max(max(resolve) - min(resolve), k["max"] - k["min"])
        row["bar"] = {"read_kernel_ms": k["median"], "k_filter_box_ms": round(statistics.median(resolve), 4), "spread_ms": round(spread, 4),
                      "met": bool(k["median"] <= statistics.median(resolve) + spread)}
        result["radii"]["%g" % radius] = row
        print("radius %g: spt_render %.3f ms (k_filter_box %.3f ms)" % (radius, statistics.median(total), statistics.median(resolve)))
        for k in range(args.increments):
            d = "done_%d" % ((k + 1) * inc)
            print("  %-8s render %8.3f ms  mean() kernel %8.3f ms  call %8.3f ms" % (
                d, row["film"]["render_ms"][d]["median"], row["film"]["read_kernel_ms"][d]["median"], row["film"]["read_call_ms"][d]["median"]))
        print("  bar met: %s" % row["bar"]["met"])
    print(json.dumps(result))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1)
    scene.close()


if __name__ == "__main__":
    main()
