#!/usr/bin/env python3
"""What spt_hits costs next to the routes that existed before it, on one GPU -> profiles/hits_cost.json.

Per workload (tools/visibility_cost.py's three: a 1024^2 lightmap of the generated 1 008 200-triangle grid, 512^2 lightmaps of cfg2's
cube and of t_materials' floor; 16 samples per texel), the gather rays of the covered texels (spt.bake_rays, t_max = f32::MAX) as
segments on the device:
  a_hits_k1 / k4 / k8       DeviceScene.all_hits, max_hits 1, 4 and 8 (SPT_HITS_DEVICE_POINTERS): the walk culls behind the K-th key
  b_all_k1 / k4 / k8        the same with count_all (SPT_HITS_COUNT_ALL): every crossing of the segment is visited
  c_gbuffer                 DeviceScene.gbuffer over the same rays as device tensors: the first hit alone
  d_gbuffer_x4              what callers did for layers: 4 calls of gbuffer from torch, t_min advanced to the layer's t in between
The legs are run alternately, each as an untimed call and a timed one (a host clock around the synchronous call), the median of --reps
with the range.  Every leg is checked against the route it replaces: record 0 of a_hits_k1 is c_gbuffer's (t, instance, prim, v, w) on
every ray; the records of b_* are those of a_*; layer j of d_gbuffer_x4 is record j of a_hits_k4 on every ray whose first four
records are triangles, or misses, with different t (a sphere's far root and a tie are what the repeated calls lose: the share of
the rays on which the two routes differ is reported).  ns per ray = seconds / (texels * samples).

  python tools/hits_cost.py [--reps 5] [--only grid|cfg2|materials] [--grid 710] [--out profiles/hits_cost.json]
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
KS = (1, 4, 8)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--grid", type=int, default=710, help="quads per side of the generated grid (710: 1 008 200 triangles)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hits_cost.json"))
    args = ap.parse_args()
    import torch   # before the package, as an embedding application would have it
    import bench
    from visibility_cost import workloads
    spt = bench.load_pkg()
    dev = torch.device("cuda", 0)
    f32_max = float(np.finfo(np.float32).max)
    result = {"what": "tools/hits_cost.py on one MI355X: %d gather rays per lightmap texel as segments (t_max f32::MAX) on the device; ms per "
                      "synchronous call (host clock), median and range of the alternating repetitions" % SAMPLES,
              "samples": SAMPLES, "reps": args.reps, "device": torch.cuda.get_device_name(0), "workloads": {}}
    for key, make, instance, size in workloads(args.only, args.grid):
        sc = spt.load_scene(make())
        ds = sc.device_scene(0)
        pts, texels = sc.lightmap_points(instance, size, size)
        rays = spt.bake_rays(sc, pts, samples=SAMPLES, seed=SEED)["rays"].reshape(-1)
        n = rays.shape[0]
        seg = np.zeros(n, dtype=spt.RAY_DTYPE)
        seg["o"], seg["t_min"], seg["d"], seg["t_max"] = rays["o"], rays["t_min"], rays["d"], f32_max
        t_seg = torch.from_numpy(seg.view(np.float32).reshape(-1, 8)).to(dev)
        t_rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 12)).to(dev)
        del seg, rays

        def layers():
            """4 calls of gbuffer, t_min moved to each layer's t: (n, 4, 5) the (t, instance, prim, v, w) of the layers as float32 words."""
            r = t_rays.clone()
            out = []
            for _ in range(4):
                g = ds.gbuffer(r)
                out.append(torch.stack([g[:, 3], g[:, 7], g[:, 11], g[:, 12], g[:, 13]], dim=1))
                hit = g.view(torch.int32)[:, 7] >= 0
                r[:, 3] = torch.where(hit, g[:, 3], r[:, 3])
            return torch.stack(out, dim=1)

        legs = {}
        for K in KS:
            legs["a_hits_k%d" % K] = lambda K=K: ds.all_hits(t_seg, max_hits=K)
            legs["b_all_k%d" % K] = lambda K=K: ds.all_hits(t_seg, max_hits=K, count_all=True)
        legs["c_gbuffer"] = lambda: ds.gbuffer(t_rays)
        legs["d_gbuffer_x4"] = layers

        # warm-up of every leg, and the checks
        def key5(rec):   # (t, instance, prim, v, w) of spt_hit_rec rows as int32 words
            return rec.view(torch.int32)[..., [0, 1, 2, 4, 5]]
        g = legs["c_gbuffer"]().view(torch.int32)
        rec1, cnt1 = legs["a_hits_k1"]()
        k1_is_gbuffer = bool(torch.equal(key5(rec1)[:, 0], g[:, [3, 7, 11, 12, 13]]))
        hit_share = float((g[:, 7] >= 0).float().mean().item())
        del g, rec1, cnt1
        b_is_a, crossings = True, None
        for K in KS:
            ra, ca = legs["a_hits_k%d" % K]()
            rb, cb = legs["b_all_k%d" % K]()
            b_is_a = b_is_a and bool(torch.equal(ra.view(torch.int32), rb.view(torch.int32))) and bool((ca[:, 0] == torch.clamp(cb[:, 0], max=K)).all())
            if K == 4:
                crossings = cb[:, 0].float()
                lay = layers().view(torch.int32)
                r4 = ra.view(torch.int32)
                t = ra[:, :, 0]
                miss = r4[:, :, 1] < 0
                comparable = (((r4[:, :, 3] >> 8) == 1) | miss).all(dim=1) & ((t[:, 1:] != t[:, :-1]) | miss[:, 1:]).all(dim=1)
                d_is_a = bool(torch.equal(lay[comparable], key5(ra)[comparable]))
                comparable_share = float(comparable.float().mean().item())
                differ_share = float((lay != key5(ra)).any(dim=2).any(dim=1).float().mean().item())
                del lay, r4, t
            del ra, ca, rb, cb
        times = {name: [] for name in legs}
        for _ in range(args.reps):
            for name, fn in legs.items():   # alternating; an untimed call first
                fn()
                times[name].append(timed(fn))
        entry = {"lightmap": "%dx%d" % (size, size), "instance": instance, "triangles": int(sc.desc.n_tris), "texels_covered": len(pts), "rays": n,
                 "gbuffer_hit_share": round(hit_share, 4), "mean_crossings": round(float(crossings.mean().item()), 4),
                 "share_with_2_or_more": round(float((crossings >= 2).float().mean().item()), 4),
                 "k1_record_equals_gbuffer": k1_is_gbuffer, "count_all_records_equal": b_is_a, "gbuffer_x4_equals_k4_where_comparable": d_is_a,
                 "comparable_share": round(comparable_share, 4), "gbuffer_x4_differs_share": round(differ_share, 4)}
        for name, ts in times.items():
            med = statistics.median(ts)
            entry[name] = {"median_ms": round(med * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3),
                           "ns_per_ray": round(med / n * 1e9, 4)}
        med = {name: statistics.median(ts) for name, ts in times.items()}
        entry["a_k1_over_c"] = round(med["a_hits_k1"] / med["c_gbuffer"], 3)
        for K in KS:
            entry["b_over_a_k%d" % K] = round(med["b_all_k%d" % K] / med["a_hits_k%d" % K], 3)
        entry["d_over_a_k4"] = round(med["d_gbuffer_x4"] / med["a_hits_k4"], 3)
        result["workloads"][key] = entry
        print(key, json.dumps(entry), flush=True)
        del t_rays, t_seg
        sc.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
