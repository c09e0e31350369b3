#!/usr/bin/env python3
"""What spt_camera_rays and spt_camera_gbuffer cost next to the routes they replace, on one GPU -> profiles/camera_device_cost.json.

Two workloads: cfg2 (scenes_amd/cfg2_cube.json) and the million-triangle grid tools/scene_deform_cost.py writes.  A thin lens, a
1024 x 1024 plan of 4 samples with the random sampler: 4 194 304 rays.  Per workload the legs alternate in one process, warmed, a host
clock around each leg, which ends in a synchronous library call (or a device synchronise); reported are the median, the range of the
repetitions and ns per ray, and the ratio of each pair.

  a  the rays with their auxiliary rays: camera_rays (spt_host_camera_rays, records in host memory) against
     DeviceScene.camera_rays(on_device=True) (spt_camera_rays, records in device memory)
  b  radiance of the plan's samples: radiance(camera_rays(...)) from host arrays against radiance over the tensors of
     DeviceScene.camera_rays(on_device=True), device pointers; both legs make their rays
  c  first-hit images: camera_gbuffer(host_rays=True), the route before spt_camera_gbuffer, against DeviceScene.camera_gbuffer with
     host and with device outputs
  d  the accumulation stage: DeviceScene.camera_gbuffer(on_device=True) against DeviceScene.camera_rays(on_device=True) +
     DeviceScene.gbuffer + the same sums in torch

  python tools/camera_device_cost.py [--reps 5] [--size 1024] [--grid 710]
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
SAMPLES, DEPTH, SEED = 4, 8, 1


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--grid", type=int, default=710, help="quads per side of the generated grid (710: 1 008 200 triangles)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camera_device_cost.json"))
    args = ap.parse_args()
    import torch   # before the package, as an embedding application would have it
    import bench
    from scene_deform_cost import write_grid_scene
    spt = bench.load_pkg()
    if spt.device_count() < 1:
        sys.exit("camera_device_cost: no GPU (a time taken elsewhere says nothing)")
    W = H = args.size
    n = W * H * SAMPLES

    def workload(name):
        if name == "cfg2":
            sc, cam_name = spt.load_scene(os.path.join(ROOT, "scenes_amd", "cfg2_cube.json")), None
        else:
            sc, cam_name = spt.load_scene(write_grid_scene(os.path.join(ROOT, "scenes_amd", "generated"), args.grid)), "main"
        ds = sc.device_scene(0)
        cam = sc.get_camera(cam_name)
        eye, fwd = np.array(cam.eye[:], dtype=np.float64), np.array(cam.forward[:], dtype=np.float64)
        model = spt.CameraModel.thin_lens(cam, 0.05, max(float(np.dot(-eye, fwd)), 1.0))
        plan = spt.PathTracer(max_depth=DEPTH, sampler=spt.SAMPLER_RANDOM, spp=SAMPLES, seed=SEED)

        def radiance_host():
            rays, aux = spt.camera_rays(model, plan, W, H, 0, SAMPLES, aux=True)
            return ds.radiance(rays.reshape(-1), aux=aux.reshape(-1), max_depth=DEPTH, seed=SEED, rng_skip=2)

        def radiance_device():
            rays, aux = ds.camera_rays(model, plan, W, H, 0, SAMPLES, aux=True, on_device=True)
            return ds.radiance(rays.reshape(-1, 12), aux=aux.reshape(-1, 16), max_depth=DEPTH, seed=SEED, rng_skip=2)

        def images_torch():
            rays, aux = ds.camera_rays(model, plan, W, H, 0, SAMPLES, aux=True, on_device=True)
            rec = ds.gbuffer(rays.reshape(-1, 12), aux.reshape(-1, 16)).reshape(SAMPLES, H, W, 16)
            hit = rec.view(torch.int32)[..., 7] >= 0
            albedo, normal = torch.zeros((H, W, 3), device=rec.device), torch.zeros((H, W, 3), device=rec.device)
            t_sum, hits = torch.zeros((H, W), device=rec.device), torch.zeros((H, W), device=rec.device)
            for s in range(SAMPLES):
                albedo, normal = albedo + rec[s, ..., 8:11], normal + rec[s, ..., 4:7]
                t_sum = t_sum + torch.where(hit[s], rec[s, ..., 3], torch.zeros_like(t_sum))
                hits = hits + hit[s].to(torch.float32)
            inv = 1.0 / SAMPLES
            out = {"albedo": albedo * inv, "normal": normal * inv, "depth": torch.where(hits > 0, t_sum / hits.clamp(min=1.0), torch.zeros_like(hits)),
                   "coverage": hits / SAMPLES}
            torch.cuda.synchronize()
            return out

        legs = {
            "a_rays_host": lambda: spt.camera_rays(model, plan, W, H, 0, SAMPLES, aux=True),
            "a_rays_device": lambda: ds.camera_rays(model, plan, W, H, 0, SAMPLES, aux=True, on_device=True),
            "b_radiance_host_rays": radiance_host,
            "b_radiance_device_rays": radiance_device,
            "c_images_present_route": lambda: spt.camera_gbuffer(ds, model, plan, W, H, samples=SAMPLES, host_rays=True),
            "c_images_device_host_out": lambda: ds.camera_gbuffer(model, plan, W, H, samples=SAMPLES),
            "c_images_device_device_out": lambda: ds.camera_gbuffer(model, plan, W, H, samples=SAMPLES, on_device=True),
            "d_images_gbuffer_and_torch": images_torch,
        }
        return sc, legs

    result = {"what": "tools/camera_device_cost.py on one MI355X: a thin lens, a %d x %d plan of %d samples (random sampler) with auxiliary rays, per "
                      "workload; ms per leg (host clock, each leg ends synchronised), median and range of %d alternating repetitions, and ns per ray"
                      % (W, H, SAMPLES, args.reps),
              "rays": n, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    for name in ("cfg2", "grid"):
        sc, legs = workload(name)
        first = {key: fn() for key, fn in legs.items()}      # warm-up of every leg, and the checks that the routes agree
        host_rays, host_aux = first["a_rays_host"]
        dev_rays, dev_aux = first["a_rays_device"]
        words = lambda t: t.view(torch.int32).cpu().numpy().view(np.uint32)
        same_rays = words(dev_rays).tobytes() == host_rays.tobytes() and words(dev_aux).tobytes() == host_aux.tobytes()
        same_radiance = bool(np.array_equal(words(first["b_radiance_device_rays"]), first["b_radiance_host_rays"].view(np.uint32)))
        present = first["c_images_present_route"]
        same_images = all(np.array_equal(first["c_images_device_host_out"][k].view(np.uint32), v.view(np.uint32)) and
                          np.array_equal(words(first["c_images_device_device_out"][k]), v.view(np.uint32)) for k, v in present.items())
        torch_close = all(bool(np.allclose(first["d_images_gbuffer_and_torch"][k].cpu().numpy(), v, rtol=1e-6, atol=1e-7)) for k, v in present.items())
        del first, host_rays, host_aux, dev_rays, dev_aux
        times = {key: [] for key in legs}
        for _ in range(args.reps):
            for key, fn in legs.items():   # alternating
                times[key].append(timed(fn))
        block = {"triangles": int(sc.desc.n_tris), "hit_share": round(float((present["coverage"] > 0).mean()), 4),
                 "device_rays_equal_host_rays": same_rays, "radiance_over_device_rays_equals_radiance_over_host_rays": same_radiance,
                 "device_images_equal_present_route": same_images, "torch_images_close_to_present_route": torch_close}
        med = {}
        for key, ts in times.items():
            med[key] = statistics.median(ts)
            block[key] = {"median_ms": round(med[key] * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3),
                          "ns_per_ray": round(med[key] / n * 1e9, 3)}
        block["a_host_over_device"] = round(med["a_rays_host"] / med["a_rays_device"], 1)
        block["b_host_over_device"] = round(med["b_radiance_host_rays"] / med["b_radiance_device_rays"], 1)
        block["c_present_over_device_host_out"] = round(med["c_images_present_route"] / med["c_images_device_host_out"], 1)
        block["c_present_over_device_device_out"] = round(med["c_images_present_route"] / med["c_images_device_device_out"], 1)
        block["d_device_over_gbuffer_and_torch"] = round(med["c_images_device_device_out"] / med["d_images_gbuffer_and_torch"], 3)
        result[name] = block
        print(name, json.dumps(block), flush=True)
        sc.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
