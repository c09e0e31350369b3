#!/usr/bin/env python3
"""What spt_bake costs next to today's route and next to the transport alone, on one GPU -> profiles/bake_cost.json.

Per workload (a 1024^2 lightmap of the generated 1 008 200-triangle grid, 512^2 lightmaps of cfg2's cube and of t_materials' floor;
16 samples per texel, max_depth 8), the covered texels of Scene.lightmap_points as bake points:
  a_bake_device      DeviceScene.bake, the points a torch tensor on the device (SPT_BAKE_DEVICE_POINTERS)
  b_bake_host        DeviceScene.bake, host pointers
  c_host_route       today's route: bake_rays on the host (the gather rays, 48 B each, and the shadow rays), DeviceScene.radiance over the
                     rays with host pointers, the in-order mean per texel in numpy, D from DeviceScene.trace_any
  d_radiance_device  the floor for the transport: DeviceScene.radiance with device pointers over the same rays, already resident
The four are run alternately, a host clock around each synchronous call, the median of --reps with the range, one warm-up per leg
and shape; `d_repeated` repeats leg d back to back (the spread the job itself shows).  ns per path = seconds / (texels * samples).

  python tools/bake_cost.py [--reps 5] [--only grid|cfg2|materials] [--grid 710]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
SAMPLES, DEPTH, SEED = 16, 8, 1


def workloads(only, grid):
    from scene_deform_cost import write_grid_scene
    all_ = (("grid", lambda: write_grid_scene(os.path.join(ROOT, "scenes_amd", "generated"), grid), "grid", 1024),
            ("cfg2", lambda: os.path.join(ROOT, "scenes_amd", "cfg2_cube.json"), "cube", 512),
            ("materials", lambda: os.path.join(ROOT, "scenes_amd", "t_materials.json"), "floor", 512))
    return [w for w in all_ if not only or w[0] == only]


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--grid", type=int, default=710, help="quads per side of the generated grid (710: 1 008 200 triangles)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bake_cost.json"))
    args = ap.parse_args()
    import torch   # before the package, as an embedding application would have it
    import bench
    spt = bench.load_pkg()
    dev = torch.device("cuda", 0)
    f32 = np.float32
    result = {"what": "tools/bake_cost.py on one MI355X: lightmap texels as bake points, %d samples each, max_depth %d; ms per synchronous call "
                      "(host clock), median and range of the alternating repetitions" % (SAMPLES, DEPTH),
              "samples": SAMPLES, "max_depth": DEPTH, "reps": args.reps, "device": torch.cuda.get_device_name(0), "workloads": {}}
    for key, make, instance, size in workloads(args.only, args.grid):
        sc = spt.load_scene(make())
        ds = sc.device_scene(0)
        pts, texels = sc.lightmap_points(instance, size, size)
        n = len(pts)
        t_pts = torch.from_numpy(pts.view(np.float32).reshape(-1, 4).copy()).to(dev)

        def host_route():
            made = spt.bake_rays(sc, pts, samples=SAMPLES, seed=SEED)
            x = ds.radiance(made["rays"].reshape(-1), max_depth=DEPTH, seed=SEED).reshape(n, SAMPLES, 3)
            acc = np.zeros((n, 3), dtype=f32)
            for k in range(SAMPLES):
                acc = acc + x[:, k]
            D = np.zeros((n, 3), dtype=f32)
            for l in range(made["delta_li"].shape[1]):
                li = made["delta_li"][:, l]
                want = np.any(li != 0, axis=-1)
                if want.any():
                    occ = np.ones(n, dtype=bool)
                    occ[want] = ds.trace_any(np.ascontiguousarray(made["delta_rays"][want, l])) != 0
                    D = np.where((want & ~occ)[:, None], D + li, D).astype(f32)
            return D + acc * (f32(1) / f32(SAMPLES))

        rays = spt.bake_rays(sc, pts, samples=SAMPLES, seed=SEED)["rays"].reshape(-1)
        t_rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 12)).to(dev)
        del rays
        legs = {
            "a_bake_device": lambda: ds.bake(t_pts, samples=SAMPLES, max_depth=DEPTH, seed=SEED),
            "b_bake_host": lambda: ds.bake(pts, samples=SAMPLES, max_depth=DEPTH, seed=SEED),
            "c_host_route": host_route,
            "d_radiance_device": lambda: ds.radiance(t_rays, max_depth=DEPTH, seed=SEED),
        }
        same = bool(np.array_equal(legs["b_bake_host"]().view(np.uint32), host_route().view(np.uint32)))   # (warm-up of b and c, and a check)
        legs["a_bake_device"]()
        legs["d_radiance_device"]()
        times = {name: [] for name in legs}
        for _ in range(args.reps):
            for name, fn in legs.items():   # alternating
                times[name].append(timed(fn))
        spread = [timed(legs["d_radiance_device"]) for _ in range(args.reps)]
        paths = n * SAMPLES
        entry = {"lightmap": "%dx%d" % (size, size), "instance": instance, "triangles": int(sc.desc.n_tris), "texels_covered": n, "paths": paths,
                 "bake_equals_host_route": same}
        for name, ts in times.items():
            med = statistics.median(ts)
            entry[name] = {"median_ms": round(med * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3),
                           "ns_per_path": round(med / paths * 1e9, 4)}
        entry["d_repeated"] = {"median_ms": round(statistics.median(spread) * 1e3, 3), "min_ms": round(min(spread) * 1e3, 3), "max_ms": round(max(spread) * 1e3, 3)}
        entry["a_over_d"] = round(statistics.median(times["a_bake_device"]) / statistics.median(times["d_radiance_device"]), 3)
        entry["c_over_a"] = round(statistics.median(times["c_host_route"]) / statistics.median(times["a_bake_device"]), 1)
        result["workloads"][key] = entry
        print(key, json.dumps(entry), flush=True)
        del t_rays, t_pts
        sc.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
