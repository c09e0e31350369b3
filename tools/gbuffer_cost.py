#!/usr/bin/env python3
"""What spt_gbuffer costs next to the routes callers have today, on one GPU -> profiles/gbuffer_cost.json.

Two workloads, one ray per pixel of a 1024 x 1024 pinhole plan (camera_rays with its auxiliary rays): cfg2 (scenes_amd/cfg2_cube.json)
and the million-triangle grid tools/scene_deform_cost.py writes.  Per workload the legs alternate in one process, warmed, a host clock
around each synchronous call; reported are the median and the range of the repetitions and ns per ray.

  a  DeviceScene.gbuffer with device pointers (torch tensors): the intake kernel and k_gbuffer, the records stay on the device
  b  DeviceScene.gbuffer from host arrays: staging up, 64 bytes per ray back
  c  DeviceScene.radiance(max_depth=0, hits=True) with device pointers: stage 1 alone plus its finish kernel, the floor for (a)
  d  what callers do for the same information today: trace_closest, then normals and constant albedos rebuilt in numpy from the
     descriptor's arrays (mesh hits; float32, the library's order of operations)
  e  pinhole only: one 1-spp SPT_RENDER_DEBUG_NORMAL render and one 1-spp SPT_RENDER_AOV_ALBEDO render, the pair that gives a pinhole's
     normal and albedo images

--once LEG [--scene cfg2|grid]: that leg alone, --calls calls behind a warm-up, nothing written - what a kernel trace of its own runs:
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/gbuffer_cost.py --once a_gbuffer_device --scene cfg2 --calls 20
--kernel-stats cfg2=FILE grid=FILE --merge: the kernel_stats CSVs of such traces of leg (a) go into the existing JSON: the split between
the intake kernel and k_gbuffer.

  python tools/gbuffer_cost.py [--reps 7] [--size 1024] [--grid 710]
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def host_reconstruction(spt, sc, ds, seg):
    """Leg (d): closest hits from the device, then world normals and constant albedos of the mesh hits in float32 numpy."""
    tabs = {k: sc.array(k) for k in ("instances", "tri_attr", "surfaces", "materials")}

    def run():
        hits = ds.trace_closest(seg)
        hit = hits["instance"] >= 0
        inst = tabs["instances"][np.maximum(hits["instance"], 0)]
        ta = tabs["tri_attr"][np.maximum(hits["prim"], 0)]
        v, w = hits["v"][:, None], hits["w"][:, None]
        u = (f32(1) - v) - w
        on = (ta["n"][:, 0] * u + ta["n"][:, 1] * v) + ta["n"][:, 2] * w
        on = on / np.sqrt((on[:, 0] * on[:, 0] + on[:, 1] * on[:, 1]) + on[:, 2] * on[:, 2])[:, None]
        nrm = inst["nrm"]
        n = (nrm[:, 0:3] * on[:, 0:1] + nrm[:, 3:6] * on[:, 1:2]) + nrm[:, 6:9] * on[:, 2:3]
        n = n / np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])[:, None]
        albedo = tabs["materials"]["c0"][tabs["surfaces"]["material"][inst["surface"]]]
        p = seg["o"] + seg["d"] * hits["t"][:, None]
        return np.where(hit[:, None], p, f32(0)), np.where(hit[:, None], n, f32(0)), np.where(hit[:, None], albedo, f32(0))
    return run


def kernel_shares(path, calls):
    """rocprofv3's kernel_stats CSV -> {kernel: {"us_per_call", "percent", "launches_per_call"}}, largest first."""
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    out = {}
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        ns = float(r["TotalDurationNs"])
        if ns / total < 0.002:
            continue
        out[r["Name"]] = {"us_per_call": round(ns / 1e3 / calls, 2), "percent": round(100.0 * ns / total, 2), "launches_per_call": round(float(r["Calls"]) / calls, 2)}
    out["(all kernels)"] = {"us_per_call": round(total / 1e3 / calls, 2), "percent": 100.0}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--grid", type=int, default=710, help="quads per side of the generated grid (710: 1 008 200 triangles)")
    ap.add_argument("--once", default="", help="run this leg alone, --calls times behind its warm-up, and write nothing")
    ap.add_argument("--scene", choices=["cfg2", "grid"], default="cfg2", help="the workload of --once")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--kernel-stats", nargs="*", default=[], metavar="SCENE=CSV")
    ap.add_argument("--kernel-stats-calls", type=int, default=21, help="the calls each trace ran, warm-up included (--once: --calls + 1)")
    ap.add_argument("--merge", action="store_true", help="add --kernel-stats to the existing --out file and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gbuffer_cost.json"))
    args = ap.parse_args()
    if args.merge:      # the traces were taken after the clock run: add them to its file, no device needed
        out = json.load(open(args.out))
        out["kernel_trace_of_leg_a"] = {"what": "rocprofv3 --kernel-trace --stats, one run per workload (--once a_gbuffer_device), %d calls each; kernels above "
                                                "0.2 %% of the run" % args.kernel_stats_calls}
        for item in args.kernel_stats:
            key, path = item.split("=", 1)
            out["kernel_trace_of_leg_a"][key] = kernel_shares(path, args.kernel_stats_calls)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        return
    import torch   # before the package, as an embedding application would have it
    import bench
    from scene_deform_cost import write_grid_scene
    spt = bench.load_pkg()
    if spt.device_count() < 1:
        sys.exit("gbuffer_cost: no GPU (a time taken elsewhere says nothing)")
    dev = torch.device("cuda", 0)
    W = H = args.size
    n = W * H

    def workload(name):
        if name == "cfg2":
            sc, cam_name = spt.load_scene(os.path.join(ROOT, "scenes_amd", "cfg2_cube.json")), None
        else:
            sc, cam_name = spt.load_scene(write_grid_scene(os.path.join(ROOT, "scenes_amd", "generated"), args.grid)), "main"
        ds = sc.device_scene(0)
        plan = spt.PathTracer(max_depth=8, sampler=spt.SAMPLER_RECURRENCE, spp=1, seed=1)
        rays, aux = spt.camera_rays(spt.CameraModel.perspective(sc.get_camera(cam_name)), plan, W, H, 0, 1, aux=True)
        rays, aux = rays.reshape(-1), aux.reshape(-1)
        t_rays = torch.from_numpy(rays.view(np.float32).reshape(n, 12).copy()).to(dev)
        t_aux = torch.from_numpy(aux.view(np.float32).reshape(n, 16).copy()).to(dev)
        seg = np.zeros(n, dtype=spt.RAY_DTYPE)
        seg["o"], seg["t_min"], seg["d"], seg["t_max"] = rays["o"], rays["t_min"], rays["d"], np.finfo(np.float32).max
        cfg = spt.OutputConfig(W, H, None, cam_name)
        normal_plan = spt.PathTracer(max_depth=8, sampler=spt.SAMPLER_RECURRENCE, spp=1, seed=1, debug_normal=True)
        albedo_plan = spt.PathTracer(max_depth=8, sampler=spt.SAMPLER_RECURRENCE, spp=1, seed=1, aov_albedo=True)

        def films():
            normal_plan.render_shard(sc, cfg)
            albedo_plan.render_shard(sc, cfg)

        legs = {
            "a_gbuffer_device": lambda: ds.gbuffer(t_rays, t_aux),
            "b_gbuffer_host": lambda: ds.gbuffer(rays, aux),
            "c_radiance_depth0_hits_device": lambda: ds.radiance(t_rays, max_depth=0, hits=True),
            "d_trace_closest_and_numpy": host_reconstruction(spt, sc, ds, seg),
            "e_normal_and_albedo_films_1spp": films,
        }
        return sc, ds, legs, rays, aux

    if args.once:
        sc, ds, legs, _, _ = workload(args.scene)
        legs[args.once]()
        ts = [timed(legs[args.once]) for _ in range(args.calls)]
        print(args.once, args.scene, "%.3f ms median of %d calls" % (statistics.median(ts) * 1e3, args.calls))
        sc.close()
        return
    result = {"what": "tools/gbuffer_cost.py on one MI355X: one ray per pixel of a %d x %d pinhole plan with auxiliary rays, per workload; ms per synchronous "
                      "call (host clock), median and range of %d alternating repetitions, and ns per ray" % (W, H, args.reps),
              "rays": n, "reps": args.reps, "device": torch.cuda.get_device_name(0),
              "bytes_per_ray_stage_2": {"ray": 48, "hit": 20, "record": 64, "aux_when_textures_are_sampled": 64}}
    for name in ("cfg2", "grid"):
        sc, ds, legs, rays, aux = workload(name)
        host = legs["b_gbuffer_host"]()       # (warm-up of b, and a check of a against it)
        same = bool(np.array_equal(legs["a_gbuffer_device"]().view(torch.int32).cpu().numpy().view(np.uint32), host.view(np.uint32).reshape(n, 16)))
        for key in ("c_radiance_depth0_hits_device", "d_trace_closest_and_numpy", "e_normal_and_albedo_films_1spp"):
            legs[key]()
        times = {key: [] for key in legs}
        for _ in range(args.reps):
            for key, fn in legs.items():   # alternating
                times[key].append(timed(fn))      # (every leg is synchronous: the library waits for its stream)
        block = {"triangles": int(sc.desc.n_tris), "hit_share": round(float((host["instance"] >= 0).mean()), 4), "device_records_equal_host_records": same}
        for key, ts in times.items():
            med = statistics.median(ts)
            block[key] = {"median_ms": round(med * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3), "ns_per_ray": round(med / n * 1e9, 3)}
        med = {key: statistics.median(ts) for key, ts in times.items()}
        block["a_over_c"] = round(med["a_gbuffer_device"] / med["c_radiance_depth0_hits_device"], 3)
        block["d_over_a"] = round(med["d_trace_closest_and_numpy"] / med["a_gbuffer_device"], 1)
        block["d_over_b"] = round(med["d_trace_closest_and_numpy"] / med["b_gbuffer_host"], 1)
        block["e_over_a"] = round(med["e_normal_and_albedo_films_1spp"] / med["a_gbuffer_device"], 2)
        result[name] = block
        print(name, json.dumps(block), flush=True)
        sc.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
