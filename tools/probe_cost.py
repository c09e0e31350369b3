#!/usr/bin/env python3
"""What spt_probe costs next to the existing route and next to spt_bake at the same path count, on one GPU -> profiles/probe_cost.json.

The scene is the generated 1 008 200-triangle grid (the one profiles/scene_vertices_cost.json was measured on); the probes are a
jittered grid over the scene's bounds grown by 10 %.  Three loops alternate in one process, one warm-up each, a host clock around each
synchronous call, the median of --reps with the range:
  a_probes        DeviceScene.probes with the visibility record, host pointers
  a_probes_device the same with the points a torch tensor on the device (SPT_PROBE_DEVICE_POINTERS)
  b_host_route    the existing route: probe_rays on the host (the gather rays, 48 B each, their nine weights and the shadow rays),
                  DeviceScene.radiance over the rays with host pointers, the in-order projection in numpy, D from DeviceScene.trace_any
  c_bake_world    DeviceScene.bake(world=True) over the same positions with the normal (0, 1, 0): the same number of paths through the
                  same bounce loop, one number per point and channel instead of nine
ns per path = seconds / (probes * samples).  --once LEG runs one leg once behind a warm-up (for a kernel trace of that leg alone).

  python tools/probe_cost.py [--reps 5] [--probes 32768] [--samples 64] [--grid 710] [--once a_probes]
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
DEPTH, SEED = 8, 1


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--probes", type=int, default=32768)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--grid", type=int, default=710, help="quads per side of the generated grid (710: 1 008 200 triangles)")
    ap.add_argument("--once", default="", help="run this leg once behind its warm-up and write nothing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_cost.json"))
    args = ap.parse_args()
    import torch   # before the package, as an embedding application would have it
    import bench
    from scene_deform_cost import write_grid_scene
    spt = bench.load_pkg()
    dev = torch.device("cuda", 0)
    f32 = np.float32
    S, n = args.samples, args.probes
    sc = spt.load_scene(write_grid_scene(os.path.join(ROOT, "scenes_amd", "generated"), args.grid))
    ds = sc.device_scene(0)
    inst = sc.array("instances")
    lo, hi = inst["bmin"].min(axis=0).astype(np.float64), inst["bmax"].max(axis=0).astype(np.float64)
    mid, half = (lo + hi) / 2, np.maximum((hi - lo) / 2, 0.5) * 1.1
    p = (mid - half + np.random.default_rng(1).random((n, 3)) * 2 * half).astype(f32)
    t_p = torch.from_numpy(p).to(dev)
    world = np.zeros(n, dtype=spt.BAKE_WORLD_DTYPE)
    world["p"], world["n"] = p, [0, 1, 0]
    w = (f32(4) * f32(np.pi)) * (f32(1) / f32(S))

    def host_route():
        made = spt.probe_rays(sc, p, samples=S, seed=SEED)
        x = ds.radiance(made["rays"].reshape(-1), max_depth=DEPTH, seed=SEED).reshape(n, S, 3)
        acc = np.zeros((n, 9, 3), dtype=f32)
        for k in range(S):
            acc = acc + x[:, k][:, None, :] * made["weights"][:, k][:, :, None]
        D = np.zeros((n, 9, 3), dtype=f32)
        for l in range(made["delta_li"].shape[1]):
            li = made["delta_li"][:, l]
            want = np.any(li != 0, axis=-1)
            if want.any():
                occ = np.ones(n, dtype=bool)
                occ[want] = ds.trace_any(np.ascontiguousarray(made["delta_rays"][want, l])) != 0
                D = np.where((want & ~occ)[:, None, None], D + li[:, None, :] * made["delta_basis"][:, l][:, :, None], D).astype(f32)
        return D + acc * w

    legs = {
        "a_probes": lambda: ds.probes(p, samples=S, max_depth=DEPTH, seed=SEED, aux=True)[0],
        "a_probes_device": lambda: ds.probes(t_p, samples=S, max_depth=DEPTH, seed=SEED, aux=True)[0],
        "b_host_route": host_route,
        "c_bake_world": lambda: ds.bake(world, samples=S, max_depth=DEPTH, seed=SEED, world=True),
    }
    if args.once:
        legs[args.once]()
        print(args.once, "%.3f ms" % (timed(legs[args.once]) * 1e3))
        sc.close()
        return
    same = bool(np.array_equal(legs["a_probes"]().view(np.uint32), host_route().view(np.uint32)))   # (warm-up of a and b, and a check)
    legs["a_probes_device"]()
    legs["c_bake_world"]()
    times = {name: [] for name in legs}
    for _ in range(args.reps):
        for name, fn in legs.items():   # alternating
            times[name].append(timed(fn))
    paths = n * S
    result = {"what": "tools/probe_cost.py on one MI355X: %d probes over the generated grid, %d samples each, max_depth %d; ms per synchronous call "
                      "(host clock), median and range of the alternating repetitions" % (n, S, DEPTH),
              "probes": n, "samples": S, "max_depth": DEPTH, "reps": args.reps, "device": torch.cuda.get_device_name(0), "triangles": int(sc.desc.n_tris),
              "paths": paths, "probes_equal_host_route": same}
    for name, ts in times.items():
        med = statistics.median(ts)
        result[name] = {"median_ms": round(med * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3),
                        "ns_per_path": round(med / paths * 1e9, 4)}
    result["b_over_a"] = round(statistics.median(times["b_host_route"]) / statistics.median(times["a_probes"]), 1)
    result["a_over_c"] = round(statistics.median(times["a_probes"]) / statistics.median(times["c_bake_world"]), 3)
    print(json.dumps(result), flush=True)
    sc.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
