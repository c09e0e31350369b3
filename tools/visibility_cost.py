#!/usr/bin/env python3
"""What spt_occluded and spt_ao cost next to the routes that existed before them, on one GPU -> profiles/visibility_cost.json.

Per workload (tools/bake_cost.py's three: a 1024^2 lightmap of the generated 1 008 200-triangle grid, 512^2 lightmaps of cfg2's cube
and of t_materials' floor; 16 samples per texel), the covered texels of Scene.lightmap_points as points and their gather rays
(spt.bake_rays, t_max = f32::MAX) as segments:
  a_occluded_device   DeviceScene.occluded, the segments a torch tensor on the device (SPT_OCCLUDED_DEVICE_POINTERS)
  b_occluded_packed   the same with SPT_OCCLUDED_PACKED
  c_occluded_host     DeviceScene.occluded, host pointers
  d_trace_any         DeviceScene.trace_any, the parity seam
  e_gbuffer_device    DeviceScene.gbuffer over the same rays as device tensors: the closest-hit route that existed
  f_ao_device         DeviceScene.ambient_occlusion, the points a torch tensor on the device (SPT_AO_DEVICE_POINTERS)
  g_ao_host           DeviceScene.ambient_occlusion, host pointers
  h_host_route        bake_rays on the host, DeviceScene.trace_any, the record in numpy (tests/_visibility_ref.py's arithmetic)
The legs are run alternately, each as an untimed call and a timed one (a host clock around the synchronous call), the median of --reps
with the range, one warm-up per leg;
`a_repeated` repeats leg a back to back (the spread the job itself shows).  ns per ray = seconds / (texels * samples).

  python tools/visibility_cost.py [--reps 5] [--only grid|cfg2|materials] [--grid 710] [--out profiles/visibility_cost.json]
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
SAMPLES, SEED = 16, 1


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visibility_cost.json"))
    args = ap.parse_args()
    import torch   # before the package, as an embedding application would have it
    import bench
    spt = bench.load_pkg()
    dev = torch.device("cuda", 0)
    f32 = np.float32
    f32_max = np.finfo(f32).max
    result = {"what": "tools/visibility_cost.py on one MI355X: lightmap texels as points, %d gather rays each as segments (t_max f32::MAX); ms per "
                      "synchronous call (host clock), median and range of the alternating repetitions" % SAMPLES,
              "samples": SAMPLES, "reps": args.reps, "device": torch.cuda.get_device_name(0), "workloads": {}}
    for key, make, instance, size in workloads(args.only, args.grid):
        sc = spt.load_scene(make())
        ds = sc.device_scene(0)
        pts, texels = sc.lightmap_points(instance, size, size)
        n = len(pts)
        t_pts = torch.from_numpy(pts.view(np.float32).reshape(-1, 4).copy()).to(dev)

        def segments(made):
            rays = made["rays"].reshape(-1)
            seg = np.zeros(rays.shape[0], dtype=spt.RAY_DTYPE)
            seg["o"], seg["t_min"], seg["d"], seg["t_max"] = rays["o"], rays["t_min"], rays["d"], f32_max
            return seg

        def host_route():
            made = spt.bake_rays(sc, pts, samples=SAMPLES, seed=SEED)
            occ = ds.trace_any(segments(made)).reshape(n, SAMPLES)
            d = made["rays"]["d"]
            acc, count = np.zeros((n, 3), dtype=f32), np.zeros(n, dtype=np.uint32)
            for k in range(SAMPLES):
                free = occ[:, k] == 0
                acc = np.where(free[:, None], acc + d[:, k], acc)
                count = count + free
            rec = np.zeros(n, dtype=spt.AO_DTYPE)
            rec["sum"], rec["count"], rec["open"] = acc, count, count.astype(f32) * (f32(1) / f32(SAMPLES))
            some = (count > 0) & np.any(acc != 0, axis=-1)
            with np.errstate(invalid="ignore", divide="ignore"):
                length = np.sqrt((acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1]) + acc[:, 2] * acc[:, 2])
                rec["bent"] = np.where(some[:, None], acc / length[:, None], f32(0))
            return rec

        made = spt.bake_rays(sc, pts, samples=SAMPLES, seed=SEED)
        seg = segments(made)
        t_seg = torch.from_numpy(seg.view(np.float32).reshape(-1, 8)).to(dev)
        t_rays = torch.from_numpy(made["rays"].reshape(-1).view(np.float32).reshape(-1, 12)).to(dev)
        del made
        legs = {
            "a_occluded_device": lambda: ds.occluded(t_seg),
            "b_occluded_packed": lambda: ds.occluded(t_seg, packed=True),
            "c_occluded_host": lambda: ds.occluded(seg),
            "d_trace_any": lambda: ds.trace_any(seg),
            "e_gbuffer_device": lambda: ds.gbuffer(t_rays),
            "f_ao_device": lambda: ds.ambient_occlusion(t_pts, samples=SAMPLES, seed=SEED),
            "g_ao_host": lambda: ds.ambient_occlusion(pts, samples=SAMPLES, seed=SEED),
            "h_host_route": host_route,
        }
        # warm-up of every leg, and the checks: occluded is trace_any, ambient_occlusion is the host route
        occ = legs["d_trace_any"]()
        same_occ = bool(np.array_equal(legs["c_occluded_host"](), occ) and np.array_equal(legs["a_occluded_device"]().cpu().numpy(), occ) and
                        np.array_equal(legs["b_occluded_packed"]().cpu().numpy().view(np.uint64), spt.pack_occluded(occ)))
        want = host_route().view(np.uint32)
        same_ao = bool(np.array_equal(legs["g_ao_host"]().view(np.uint32), want) and
                       np.array_equal(legs["f_ao_device"]().cpu().numpy().view(np.uint32).reshape(-1), want))
        gb = legs["e_gbuffer_device"]()
        hit_share = float((gb.view(torch.int32)[:, 7] >= 0).float().mean().item())
        del gb
        times = {name: [] for name in legs}
        for _ in range(args.reps):
            for name, fn in legs.items():   # alternating; an untimed call first, so that no leg is timed on a device its predecessor's host work left idle
                fn()
                times[name].append(timed(fn))
        spread = [timed(legs["a_occluded_device"]) for _ in range(args.reps)]
        rays = n * SAMPLES
        entry = {"lightmap": "%dx%d" % (size, size), "instance": instance, "triangles": int(sc.desc.n_tris), "texels_covered": n, "rays": rays,
                 "occluded_share": round(float(occ.mean()), 4), "gbuffer_hit_share": round(hit_share, 4), "occluded_equals_trace_any": same_occ,
                 "ao_equals_host_route": same_ao}
        for name, ts in times.items():
            med = statistics.median(ts)
            entry[name] = {"median_ms": round(med * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3),
                           "ns_per_ray": round(med / rays * 1e9, 4)}
        entry["a_repeated"] = {"median_ms": round(statistics.median(spread) * 1e3, 3), "min_ms": round(min(spread) * 1e3, 3), "max_ms": round(max(spread) * 1e3, 3)}
        med = {name: statistics.median(ts) for name, ts in times.items()}
        entry["a_over_e"] = round(med["a_occluded_device"] / med["e_gbuffer_device"], 3)
        entry["f_over_a"] = round(med["f_ao_device"] / med["a_occluded_device"], 3)
        entry["d_over_a"] = round(med["d_trace_any"] / med["a_occluded_device"], 1)
        entry["h_over_f"] = round(med["h_host_route"] / med["f_ao_device"], 1)
        result["workloads"][key] = entry
        print(key, json.dumps(entry), flush=True)
        del t_rays, t_seg, t_pts
        sc.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
