#!/usr/bin/env python3
"""What animating a scene costs per frame, on one GPU -> profiles/scene_update_cost.json.

cfg2 (scenes_amd/cfg2_cube.json + pt.json) at the bench's headline size, 1024 x 1024 @ 256 spp, once as it is (LDS-resident
geometry) and once under SPT_NO_LDS_GEO=1 (the large-scene form, whose update rewrites the dynamic tail of the blob only).
Three loops, each --frames frames (>= 200) after a warm-up, timed in blocks of --block frames: a host clock around a block that
ends in spt_render_wait, so a block's time over its frames is the steady-state time per frame; the median over the blocks and
their spread (max - min) are reported.  The loops alternate block by block, so they share whatever else the machine does.

  a  spt_render with SPT_RENDER_ASYNC into a page-locked film, only the camera moving (what the library could do before
     spt_scene_update)
  b  the same with the cube rotated before every frame: Scene.set_transforms + DeviceScene.update (spt_scene_update)
  c  the same animation without spt_scene_update: destroy the device scene, create it from the edited descriptor, render

Also: the host time of the update call alone and of set_transforms alone (a host clock around each call, the median over all
frames of loop b) and the bytes the last update copied (spt_debug_render_info, counter 5).

Loop c creates the device scene - streams, events, some forty device buffers and the render workspace of the image size - once per
frame, so it is slower than the others by orders of magnitude: --only splits the two runs into two calls.

  python tools/scene_update_cost.py [--frames 200] [--block 20] [--width 1024] [--height 1024] [--spp 256] [--only default|SPT_NO_LDS_GEO=1]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "spread": round(max(xs) - min(xs), 4), "n": len(xs)}


def cube_fwd(angle_deg):
    """The cube of cfg2 rotated about y (Affine from_rotation_y of the loader), as spt_instance::fwd: three columns, then t."""
    a = math.radians(angle_deg)
    s, c = math.sin(a), math.cos(a)
    return np.array([c, 0, -s, 0, 1, 0, s, 0, c, 0, 0, 0], dtype=np.float32)


def run(spt, args, env):
    for k, v in env.items():
        os.environ[k] = v
    try:
        scene = spt.load_scene(os.path.join(ROOT, "scenes_amd", "cfg2_cube.json"))
        r = spt.load_renderer(os.path.join(ROOT, "scenes_amd", "pt.json"), seed=1)
        r.spp = args.spp
        w, h = args.width, args.height
        lib = spt.hip_lib()
        ptr = C.c_void_p()
        assert lib.spt_alloc_pinned(w * h * 12, C.byref(ptr)) == 0
        film = np.ctypeslib.as_array((C.c_float * (w * h * 3)).from_address(ptr.value)).reshape(h, w, 3)
        frame = [0]

        def camera():       # a small orbit: every frame has another eye, as a moving camera has
            t = 0.002 * frame[0]
            eye = (7.0 * math.sin(t), 0.0, 7.0 * math.cos(t))
            return spt.make_camera(eye, (-eye[0], 0.0, -eye[2]), (0.0, 1.0, 0.0), 45.0)

        update_ms, transform_ms, seam = [], [], {"update_bytes": 0}

        def frame_a():
            r.render_shard(scene, spt.OutputConfig(w, h, None, camera()), film=film, wait=False)

        def frame_b():
            t0 = time.perf_counter()
            scene.set_transforms({"cube": cube_fwd(60.0 + 0.5 * frame[0])})
            t1 = time.perf_counter()
            scene.device_scene(0).update()
            t2 = time.perf_counter()
            transform_ms.append((t1 - t0) * 1e3)
            update_ms.append((t2 - t1) * 1e3)
            r.render_shard(scene, spt.OutputConfig(w, h, None, camera()), film=film, wait=False)

        def frame_c():
            scene.set_transforms({"cube": cube_fwd(60.0 + 0.5 * frame[0])})
            scene.close_device_scene(0)                     # spt_render_wait + spt_scene_destroy
            r.render_shard(scene, spt.OutputConfig(w, h, None, camera()), film=film, wait=False)      # spt_scene_create inside

        loops = {"a_camera_only": frame_a, "b_scene_update": frame_b, "c_destroy_create": frame_c}
        per_frame = {k: [] for k in loops}
        for fn in loops.values():       # warm-up: workspace, code objects, both buffer sets
            for _ in range(4):
                fn()
                frame[0] += 1
            r.wait(scene)
        update_ms.clear()
        transform_ms.clear()
        blocks = -(-args.frames // args.block)
        for _ in range(blocks):
            for key, fn in loops.items():
                r.wait(scene)
                t0 = time.perf_counter()
                for _ in range(args.block):
                    fn()
                    frame[0] += 1
                r.wait(scene)
                per_frame[key].append((time.perf_counter() - t0) * 1e3 / args.block)
                if key == "b_scene_update":     # outside the timed block, before loop c replaces the device scene and its counters
                    seam["update_bytes"] = scene.device_scene(0).render_info(5)
                print("[%s] %s: %.3f ms per frame" % (",".join(env) or "default", key, per_frame[key][-1]), file=sys.stderr, flush=True)
        info = {"lds_resident": not env, "frames_per_loop": blocks * args.block, "block": args.block,
                "ms_per_frame": {k: stats(v) for k, v in per_frame.items()},
                "update_call_host_ms": stats(update_ms), "set_transforms_host_ms": stats(transform_ms),
                "update_bytes": seam["update_bytes"]}
        a, b = info["ms_per_frame"]["a_camera_only"]["median"], info["ms_per_frame"]["b_scene_update"]["median"]
        own = info["update_call_host_ms"]["median"] + info["set_transforms_host_ms"]["median"]
        info["b_minus_a_ms"] = round(b - a, 4)
        info["host_ms_in_set_transforms_and_update"] = round(own, 4)
        info["note"] = ("b - a = %.3f ms per frame against %.3f ms of host time in set_transforms + update (medians); the spread of loop a over its "
                        "blocks is %.3f ms.  The gap is reported, not attributed: no experiment here takes it apart"
                        % (b - a, own, info["ms_per_frame"]["a_camera_only"]["spread"]))
        scene.close()
        lib.spt_free_pinned(ptr)
        return info
    finally:
        for k in env:
            os.environ.pop(k, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--only", choices=["default", "SPT_NO_LDS_GEO=1"], help="one of the two runs (the other is kept from the file that is there)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_update_cost.json"))
    args = ap.parse_args()
    import bench
    spt = bench.load_pkg()
    if spt.device_count() < 1:
        sys.exit("scene_update_cost: no GPU (a time taken elsewhere says nothing)")
    out = {"what": "tools/scene_update_cost.py on one MI355X: scenes_amd/cfg2_cube.json + pt.json at %d x %d @ %d spp, ms per frame (host clock around blocks "
                   "of %d frames ending in spt_render_wait; median and spread over the blocks), loops alternating block by block"
                   % (args.width, args.height, args.spp, args.block),
           "runs": {}}
    if args.only and os.path.exists(args.out):
        with open(args.out) as f:
            out["runs"] = json.load(f).get("runs", {})
    for name, env in (("default", {}), ("SPT_NO_LDS_GEO=1", {"SPT_NO_LDS_GEO": "1"})):
        if not args.only or args.only == name:
            out["runs"][name] = run(spt, args, env)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
