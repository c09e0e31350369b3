#!/usr/bin/env python3
"""What spt_radiance costs next to the camera path, on one GPU -> profiles/radiance_cost.json.

Per workload (cfg2 at 1024^2, t_materials at 512^2, BASELINE cfg4 at 1024^2; 16 samples per pixel, max_depth 8, random sampler):
  film    ProgressiveFilm.render(16): k_primary and the camera pipeline, the number to hold the others against.  With --parent-lib DIR
          the same increment is also timed on the libraries in DIR (SPT_LIB_DIR): a child process holds the same scene and film there
          and times ONE increment each time it is told to, so that leg alternates with the others like any of them.
  host    DeviceScene.radiance on numpy rays: 16 camera-equivalent rays per pixel (perspective_rays on random offsets), host pointers.
  device  the same rays as torch tensors on the device (SPT_RADIANCE_DEVICE_POINTERS).
  repeats one ray per pixel with repeats = 16, host pointers: one 48-byte record for 16 paths.
The three (four) are run alternately, a host clock around each synchronous call, the median of 5; `spread` repeats one of them.
The upload ceiling is an ESTIMATE from sizes (48 B in + 12 B out per ray over a nominal PCIe rate), not a measurement.

  python tools/radiance_cost.py [--reps 5] [--parent-lib DIR] [--only cfg2|materials|cfg4]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SAMPLES, DEPTH = 16, 8
PCIE_NOMINAL_GBPS = 64.0   # PCIe 5.0 x16, one direction, before protocol overhead: an upper bound for the estimate


def workloads(only):
    sys.path.insert(0, os.path.join(ROOT, "scenes_amd"))
    import make_scenes
    gen = make_scenes.make_full()
    all_ = (("cfg2", os.path.join(ROOT, "scenes_amd", "cfg2_cube.json"), None, 1024, 1024),
            ("materials", os.path.join(ROOT, "scenes_amd", "t_materials.json"), "main", 512, 512),
            ("cfg4", os.path.join(gen, "cfg4_materials_env.json"), "main", 1024, 1024))
    return [w for w in all_ if not only or w[0] == only]


def film_times(spt, scene, camera, w, h, reps):
    r = spt.PathTracer(max_depth=DEPTH, sampler=spt.SAMPLER_RANDOM, spp=SAMPLES * (reps + 1), seed=1)
    film = r.progressive(scene, spt.OutputConfig(w, h, None, camera))
    film.render(SAMPLES)   # warm-up: workspace
    return film, r


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def film_only(args):
    """The child of --parent-lib, on whatever SPT_LIB_DIR names: per line "load <key>" it opens that workload's scene and a film
    (warm), per line "go" it times one increment and answers with the seconds, "quit" ends it."""
    import bench
    spt = bench.load_pkg()
    table = {w[0]: w for w in workloads(args.only)}
    sc = film = None
    for line in sys.stdin:
        word = line.split()
        if not word or word[0] == "quit":
            break
        if word[0] == "load":
            if film is not None:
                film.close()
                sc.close()
            _, path, camera, w, h = table[word[1]]
            sc = spt.load_scene(path)
            film, _ = film_times(spt, sc, camera, w, h, args.reps)
            print("ready", flush=True)
        elif word[0] == "go":
            print("t %.9f" % timed(lambda: film.render(SAMPLES)), flush=True)
    if film is not None:
        film.close()
        sc.close()


class ParentFilm:
    """The film leg on another build of the libraries, in a child process that answers one increment at a time."""

    def __init__(self, lib_dir, args):
        env = dict(os.environ, SPT_LIB_DIR=os.path.abspath(lib_dir))
        cmd = [sys.executable, os.path.abspath(__file__), "--film-only", "--reps", str(args.reps)] + (["--only", args.only] if args.only else [])
        self.p = subprocess.Popen(cmd, env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def ask(self, line, want):
        self.p.stdin.write(line + "\n")
        self.p.stdin.flush()
        while True:
            ans = self.p.stdout.readline()
            if not ans:
                raise RuntimeError("the parent-library process ended")
            if ans.startswith(want):
                return ans.split()

    def load(self, key):
        self.ask("load " + key, "ready")

    def render(self):
        self.t = float(self.ask("go", "t ")[1])

    def close(self):
        try:
            self.p.stdin.write("quit\n")
            self.p.stdin.flush()
            self.p.wait(timeout=60)
        except Exception:
            self.p.kill()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only", default="")
    ap.add_argument("--film-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radiance_cost.json"))
    args = ap.parse_args()
    if args.film_only:
        return film_only(args)
    import torch   # before the package, as an embedding application would have it
    import bench
    spt = bench.load_pkg()
    dev = torch.device("cuda", 0)
    result = {"samples_per_pixel": SAMPLES, "max_depth": DEPTH, "reps": args.reps, "device": torch.cuda.get_device_name(0), "workloads": {},
              "upload_ceiling": {"estimate_not_measurement": True, "bytes_per_ray": 60, "pcie_nominal_GB_per_s": PCIE_NOMINAL_GBPS,
                                 "rays_per_s": PCIE_NOMINAL_GBPS * 1e9 / 60.0}}
    parent = ParentFilm(args.parent_lib, args) if args.parent_lib else None
    for key, path, camera, w, h in workloads(args.only):
        sc = spt.load_scene(path)
        ds = sc.device_scene(0)
        cam = sc.get_camera(camera)
        rng = np.random.default_rng(1)
        off = rng.random((SAMPLES, h, w, 2), dtype=np.float32)
        rays = spt.perspective_rays(cam, w, h, off).reshape(-1)
        one = np.ascontiguousarray(rays[: w * h])
        t_rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 12)).to(dev)
        film, _ = film_times(spt, sc, camera, w, h, args.reps)
        legs = {
            "film": lambda: film.render(SAMPLES),
            "host": lambda: ds.radiance(rays, max_depth=DEPTH, seed=1, rng_skip=2),
            "device": lambda: ds.radiance(t_rays, max_depth=DEPTH, seed=1, rng_skip=2),
            "repeats16_host": lambda: ds.radiance(one, max_depth=DEPTH, seed=1, rng_skip=2, repeats=SAMPLES),
        }
        if parent is not None:
            parent.load(key)
            legs["film_parent_lib"] = parent.render   # (its own clock, around the increment inside the child)
        for name in ("host", "device", "repeats16_host"):
            legs[name]()   # warm-up: workspace, staging
        times = {name: [] for name in legs}
        for _ in range(args.reps):
            for name, fn in legs.items():   # alternating
                t = timed(fn)
                times[name].append(parent.t if name == "film_parent_lib" else t)
        spread = [timed(legs["device"]) for _ in range(args.reps)]
        n_paths = w * h * SAMPLES
        entry = {"width": w, "height": h, "paths": n_paths}
        for name, ts in times.items():
            med = statistics.median(ts)
            if name == "film_parent_lib":
                entry[name] = {"median_ms": round(med * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3)}
                continue
            entry[name] = {"median_ms": round(med * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3),
                           "Mpaths_per_s": round(n_paths / med / 1e6, 1)}
        entry["device_repeated"] = {"min_ms": round(min(spread) * 1e3, 3), "max_ms": round(max(spread) * 1e3, 3),
                                    "median_ms": round(statistics.median(spread) * 1e3, 3)}
        entry["host_vs_upload_ceiling"] = round((n_paths / statistics.median(times["host"])) / result["upload_ceiling"]["rays_per_s"], 3)
        result["workloads"][key] = entry
        print(key, json.dumps(entry))
        film.close()
        del t_rays
        sc.close()
    if parent is not None:
        parent.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
