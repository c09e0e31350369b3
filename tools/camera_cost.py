#!/usr/bin/env python3
"""What a camera model costs, on one GPU -> profiles/camera_models_cost.json.

cfg2 (scenes_amd/cfg2_cube.json + pt.json) at the bench's headline size, 1024 x 1024 @ 256 spp, four loops in one process, warmed,
alternating block by block so that they share whatever else the machine does.  A block is --block frames queued with
SPT_RENDER_ASYNC into a page-locked film and one spt_render_wait, a host clock around it; reported are the median over the blocks and
their spread (max - min), in ms per frame and ns per sample.

  a  spt_render, the pinhole fast path (candidate masks, origin candidates, pass pipeline)
  b  the same under SPT_CAMERA_GENERAL=1: the pinhole through k_primary_cam - the price of full path records and no culling
  c  a thin lens of radius 0.05 focused on the cube (spt_render_camera)
  d  what callers did before: DeviceScene.radiance(thin_lens_rays(...)) with the rays made in float64 numpy on the host and uploaded,
     --d-spp samples per pixel per call (48 bytes per sample go up; the whole plan does not fit a sensible host array), host
     generation and upload included; reported per sample

(c) must take less time per sample than (d): that is the feature's reason.  (b) / (a) decides nothing.

--parent-lib DIR: the parent commit's build (its simple-path-tracer_amd/lib).  Loop (a) is then also run in fresh processes that
alternate between that build and this one (--rounds each), and the margin for "the headline did not move" is the spread of the
parent against itself in that call.

--only a|b|c: that loop alone, --frames frames behind a warm-up, nothing written - what a kernel trace of its own runs:
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/camera_cost.py --only b --frames 20
--kernel-stats a=FILE b=FILE c=FILE: the kernel_stats CSVs of such traces; their kernels' shares go into the JSON beside the host clock's
ratios (the trace of b against the trace of a says where b / a comes from); with --merge they are added to the file of an earlier run.

  python tools/camera_cost.py [--frames 60] [--block 10] [--d-spp 4] [--parent-lib DIR] [--rounds 3] [--kernel-stats a=.. b=.. c=..]
"""
import csv
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SWITCH = "SPT_CAMERA_GENERAL"


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "spread": round(max(xs) - min(xs), 4), "n": len(xs)}


def setup(spt, args):
    scene = spt.load_scene(os.path.join(ROOT, "scenes_amd", "cfg2_cube.json"))
    r = spt.load_renderer(os.path.join(ROOT, "scenes_amd", "pt.json"), seed=1)
    r.spp = args.spp
    ptr = C.c_void_p()
    assert spt.hip_lib().spt_alloc_pinned(args.width * args.height * 12, C.byref(ptr)) == 0
    film = np.ctypeslib.as_array((C.c_float * (args.width * args.height * 3)).from_address(ptr.value)).reshape(args.height, args.width, 3)
    return scene, r, film, ptr


def timed_blocks(r, scene, loops, blocks, block, tag):
    per_frame = {k: [] for k in loops}
    for fn in loops.values():       # warm-up: workspace, code objects, both buffer sets
        for _ in range(4):
            fn()
        r.wait(scene)
    for _ in range(blocks):
        for key, fn in loops.items():
            r.wait(scene)
            t0 = time.perf_counter()
            for _ in range(block):
                fn()
            r.wait(scene)
            per_frame[key].append((time.perf_counter() - t0) * 1e3 / block)
            print("[%s] %s: %.3f ms per frame" % (tag, key, per_frame[key][-1]), file=sys.stderr, flush=True)
    return per_frame


def child_a(args):
    """Loop (a) alone, in this process's build (SPT_LIB_DIR): one JSON line with the per-block times."""
    import bench
    spt = bench.load_pkg()
    scene, r, film, ptr = setup(spt, args)
    cfg = spt.OutputConfig(args.width, args.height)
    per = timed_blocks(r, scene, {"a": lambda: r.render_shard(scene, cfg, film=film, wait=False)}, -(-args.frames // args.block), args.block,
                       os.environ.get("SPT_LIB_DIR", "this build"))
    scene.close()
    spt.hip_lib().spt_free_pinned(ptr)
    print(json.dumps(per["a"]))


def kernel_shares(path, frames):
    """rocprofv3's kernel_stats CSV -> {kernel: {"ms_per_frame", "percent", "calls_per_frame"}}, template arguments kept, largest first."""
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    out = {}
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        ns = float(r["TotalDurationNs"])
        if ns / total < 0.002:
            continue
        out[r["Name"]] = {"ms_per_frame": round(ns / 1e6 / frames, 4), "percent": round(100.0 * ns / total, 2), "calls_per_frame": round(float(r["Calls"]) / frames, 2)}
    out["(all kernels)"] = {"ms_per_frame": round(total / 1e6 / frames, 4), "percent": 100.0}
    return out


def add_kernel_trace(out, args):
    out["kernel_trace"] = {"what": "rocprofv3 --kernel-trace --stats, one run per loop (--only), %d frames each; kernels above 0.2 %% of the run" % args.kernel_stats_frames}
    for item in args.kernel_stats:
        key, path = item.split("=", 1)
        out["kernel_trace"][key] = kernel_shares(path, args.kernel_stats_frames)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--d-spp", type=int, default=4)
    ap.add_argument("--d-calls", type=int, default=3)
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child-a", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--only", choices=["a", "b", "c"])
    ap.add_argument("--kernel-stats", nargs="*", default=[], metavar="LOOP=CSV")
    ap.add_argument("--merge", action="store_true", help="add --kernel-stats to the existing --out file and stop")
    ap.add_argument("--kernel-stats-frames", type=int, default=24, help="the frames each trace ran, warm-up included (--only: --frames + 4)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camera_models_cost.json"))
    args = ap.parse_args()
    if args.child_a:
        return child_a(args)
    if args.merge:      # the traces were taken after the clock run: add them to its file, no device needed
        out = json.load(open(args.out))
        add_kernel_trace(out, args)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        return
    import bench
    spt = bench.load_pkg()
    if spt.device_count() < 1:
        sys.exit("camera_cost: no GPU (a time taken elsewhere says nothing)")
    scene, r, film, ptr = setup(spt, args)
    w, h = args.width, args.height
    cfg = spt.OutputConfig(w, h)
    cam = scene.get_camera(None)
    focus = float(np.linalg.norm(np.array(cam.eye[:], dtype=np.float64)))   # the cube stands at the origin
    lens = spt.CameraModel.thin_lens(cam, 0.05, focus)
    ds = scene.device_scene(0)

    def frame_a():
        r.render_shard(scene, cfg, film=film, wait=False)

    def frame_b():
        os.environ[SWITCH] = "1"
        try:
            r.render_shard(scene, cfg, film=film, wait=False)
        finally:
            del os.environ[SWITCH]

    def frame_c():
        r.render_shard(scene, cfg, film=film, wait=False, camera_model=lens)

    if args.only:
        fn = {"a": frame_a, "b": frame_b, "c": frame_c}[args.only]
        for _ in range(4 + args.frames):
            fn()
        r.wait(scene)
        scene.close()
        spt.hip_lib().spt_free_pinned(ptr)
        return
    before = ds.render_info(8)
    per = timed_blocks(r, scene, {"a_pinhole": frame_a, "b_pinhole_general": frame_b, "c_thin_lens": frame_c}, -(-args.frames // args.block), args.block, "loops")
    cam_passes = ds.render_info(8) - before
    # (d): host generation in float64 numpy, upload, spt_radiance; synchronous calls of --d-spp samples per pixel
    rng = np.random.default_rng(1)
    d_ms, d_gen_ms = [], []
    for k in range(args.d_calls + 1):
        t0 = time.perf_counter()
        off = rng.random((args.d_spp, h, w, 2), dtype=np.float32)
        uv = rng.random((args.d_spp, h, w, 2), dtype=np.float32) * 2 - 1
        rays = spt.thin_lens_rays(cam, w, h, off, uv, 0.05, focus)
        t1 = time.perf_counter()
        ds.radiance(rays.reshape(-1), max_depth=r.max_depth, seed=1, rng_skip=2)
        t2 = time.perf_counter()
        if k:     # (the first call grows the workspace)
            d_ms.append((t2 - t0) * 1e3)
            d_gen_ms.append((t1 - t0) * 1e3)
        print("[d] %d spp: %.1f ms (%.1f ms of it host generation)" % (args.d_spp, (t2 - t0) * 1e3, (t1 - t0) * 1e3), file=sys.stderr, flush=True)
    n_frame, n_d = float(w) * h * args.spp, float(w) * h * args.d_spp
    out = {"what": "tools/camera_cost.py on one MI355X: scenes_amd/cfg2_cube.json + pt.json at %d x %d @ %d spp; loops a - c: ms per frame (host clock around "
                   "blocks of %d asynchronous frames ending in spt_render_wait; median and spread over the blocks, alternating block by block); d: ms per "
                   "synchronous call of %d spp, rays from thin_lens_rays (float64 numpy) included" % (w, h, args.spp, args.block, args.d_spp),
           "ms_per_frame": {k: stats(v) for k, v in per.items()},
           "d_radiance_of_host_rays_ms_per_call": stats(d_ms), "d_host_generation_ms_per_call": stats(d_gen_ms), "d_spp": args.d_spp,
           "passes_through_k_primary_cam": cam_passes}
    med = {k: v["median"] for k, v in out["ms_per_frame"].items()}
    out["ns_per_sample"] = {k: round(v * 1e6 / n_frame, 5) for k, v in med.items()}
    out["ns_per_sample"]["d_radiance_of_host_rays"] = round(out["d_radiance_of_host_rays_ms_per_call"]["median"] * 1e6 / n_d, 5)
    out["b_over_a"] = round(med["b_pinhole_general"] / med["a_pinhole"], 3)
    out["c_over_a"] = round(med["c_thin_lens"] / med["a_pinhole"], 3)
    out["d_over_c_per_sample"] = round(out["ns_per_sample"]["d_radiance_of_host_rays"] / out["ns_per_sample"]["c_thin_lens"], 1)
    scene.close()
    spt.hip_lib().spt_free_pinned(ptr)
    if args.parent_lib:
        runs = {"parent": [], "this": []}
        for _ in range(args.rounds):
            for key, lib in (("parent", os.path.abspath(args.parent_lib)), ("this", spt.LIB_DIR)):
                env = dict(os.environ, SPT_LIB_DIR=lib)
                res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-a", "--frames", str(args.frames), "--block", str(args.block),
                                      "--width", str(w), "--height", str(h), "--spp", str(args.spp)], env=env, capture_output=True, text=True, timeout=600)
                if res.returncode != 0:
                    sys.exit("camera_cost: loop (a) failed in the %s build:\n%s" % (key, res.stderr[-2000:]))
                runs[key].append(round(statistics.median(json.loads(res.stdout.strip().splitlines()[-1])), 4))
        out["a_against_parent"] = {"ms_per_frame_medians_of_fresh_processes": runs,
                                   "parent_spread": round(max(runs["parent"]) - min(runs["parent"]), 4),
                                   "this_median_minus_parent_median": round(statistics.median(runs["this"]) - statistics.median(runs["parent"]), 4)}
    if args.kernel_stats:
        add_kernel_trace(out, args)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
