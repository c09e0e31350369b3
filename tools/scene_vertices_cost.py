#!/usr/bin/env python3
"""What deforming a mesh from its vertex arrays costs per frame, on one GPU -> profiles/scene_vertices_cost.json.

Written after tools/scene_deform_cost.py: the same two scenes ("cfg2": scenes_amd/cfg2_cube.json at the bench's headline size,
LDS-resident; "grid": the generated displaced grid of 1 008 200 triangles, large-scene form), the same block method (a host clock
around a block of frames that ends in spt_render_wait; median and spread over the blocks), the loops alternating block by block in
one process:

  a  spt_render with SPT_RENDER_ASYNC into a page-locked film, only the camera moving
  b  the same with spt_scene_deform before every frame, records made beforehand (two states, alternating): the baseline, measured
     in the same run
  v  the same with spt_scene_deform_vertices before every frame: the positions of the same two states

Per call (loops b and v): the host time of the call, the time its copies and kernels took on the device (HIP events around them:
spt_debug_render_info, counter 6, read in a pass of its own outside the timed blocks) and the bytes it copied (counter 5).  On the
host alone: Scene.set_mesh_positions, Scene.set_mesh_vertices and the materialisation the next read of the descriptor runs; one
spt_scene_mesh_topology registration.

  python tools/scene_vertices_cost.py [--only cfg2|grid] [--grid 710] [--frames 100] [--block 10]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from scene_deform_cost import State, stats, write_grid_scene   # noqa: E402  (the scenes and the records of loop b are that tool's)

f32 = np.float32


def run(spt, args, which):
    if which == "cfg2":
        path, name, spp = os.path.join(ROOT, "scenes_amd", "cfg2_cube.json"), "cube", args.spp
        deform = lambda p, t: (p * np.array([1.0 + 0.2 * math.sin(t), 1.0, 1.0 + 0.2 * math.cos(t)], dtype=f32)).astype(f32)
        frames, block = args.frames, args.block
    else:
        path, name, spp = write_grid_scene(os.path.join(ROOT, "scenes_amd", "generated"), args.grid), "grid", args.grid_spp
        deform = lambda p, t: (p + np.stack([0 * p[:, 0], 0.01 * np.sin(6 * p[:, 0] + t) * np.cos(5 * p[:, 2]), 0 * p[:, 0]], axis=1)).astype(f32)
        frames, block = args.grid_frames, args.grid_block
    scene = spt.load_scene(path)
    r = spt.load_renderer(os.path.join(ROOT, "scenes_amd", "pt.json"), seed=1)
    r.spp = spp
    w, h = args.width, args.height
    lib = spt.hip_lib()
    ptr = C.c_void_p()
    assert lib.spt_alloc_pinned(w * h * 12, C.byref(ptr)) == 0
    film = np.ctypeslib.as_array((C.c_float * (w * h * 3)).from_address(ptr.value)).reshape(h, w, 3)
    mesh = scene.mesh_index(name)
    rest = scene.mesh_positions(name)
    n_tris = int(scene.array("meshes")[mesh]["tri_count"])
    frame = [0]

    def camera():
        t = 0.002 * frame[0]
        if which == "cfg2":
            eye = (7.0 * math.sin(t), 0.0, 7.0 * math.cos(t))
            return spt.make_camera(eye, (-eye[0], 0.0, -eye[2]), (0.0, 1.0, 0.0), 45.0)
        eye = (4.5 * math.sin(t), 2.2, 4.5 * math.cos(t))
        return spt.make_camera(eye, (-eye[0], -2.0, -eye[2]), (0.0, 1.0, 0.0), 45.0)

    # on the host alone: the two loader entries and the materialisation, on the two states of the loops
    set_positions_ms, set_vertices_ms, materialise_ms = [], [], []
    positions = [deform(rest, t) for t in (0.7, 2.1)]
    states = []
    for rep in range(3):
        for p in positions:
            t0 = time.perf_counter()
            scene.set_mesh_vertices(name, p)
            t1 = time.perf_counter()
            scene.desc                                  # makes the pending mesh
            t2 = time.perf_counter()
            scene.set_mesh_positions(name, p)
            t3 = time.perf_counter()
            set_vertices_ms.append((t1 - t0) * 1e3)
            materialise_ms.append((t2 - t1) * 1e3)
            set_positions_ms.append((t3 - t2) * 1e3)
            if rep == 0:
                states.append(State(scene, mesh))       # the records of loop b, and the dynamic arrays of both loops
    ds = scene.device_scene(0)                          # created on state 1's geometry
    topo = scene.mesh_topology(name)
    register_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        ds.set_topology(topo["mesh"], topo["indices"], topo["face_of_tri"], topo["uv"], topo["normals"])
        register_ms.append((time.perf_counter() - t0) * 1e3)
    call_ms = {"b": [], "v": []}

    def apply(kind, k, timed=True):
        s = states[k % 2]
        t0 = time.perf_counter()
        if kind == "b":
            ds.update_arrays(s.instances, s.lights, tlas_nodes=s.tlas, meshes={mesh: (s.tri_pos, s.tri_attr)})
        else:
            ds.update_arrays(s.instances, s.lights, tlas_nodes=s.tlas, vertices={mesh: (positions[k % 2], None)})
        if timed:
            call_ms[kind].append((time.perf_counter() - t0) * 1e3)

    def frame_a():
        r.render_shard(scene, spt.OutputConfig(w, h, None, camera()), film=film, wait=False)

    def frame_b():
        apply("b", frame[0])
        frame_a()

    def frame_v():
        apply("v", frame[0])
        frame_a()

    loops = {"a_camera_only": frame_a, "b_scene_deform": frame_b, "v_scene_deform_vertices": frame_v}
    per_frame = {k: [] for k in loops}
    for fn in loops.values():                # warm-up: workspace, code objects, the refit's scratch and heights
        for _ in range(3):
            fn()
            frame[0] += 1
        r.wait(scene)
    for v in call_ms.values():
        v.clear()
    for _ in range(-(-frames // block)):
        for key, fn in loops.items():
            r.wait(scene)
            t0 = time.perf_counter()
            for _ in range(block):
                fn()
                frame[0] += 1
            r.wait(scene)
            per_frame[key].append((time.perf_counter() - t0) * 1e3 / block)
            print("[%s] %s: %.3f ms per frame" % (which, key, per_frame[key][-1]), file=sys.stderr, flush=True)
    # per call, in a pass of its own: the queue is empty before each call, counter 6 waits for the call's events
    device_ms, nbytes = {"b": [], "v": []}, {}
    for kind in ("b", "v"):
        for k in range(10):
            r.wait(scene)
            apply(kind, k, timed=False)
            device_ms[kind].append(ds.render_info(6) / 1e6)
        nbytes[kind] = ds.render_info(5)
    # the same film either way
    apply("b", 0, timed=False)
    cfg = spt.OutputConfig(w, h)
    film_b = r.render_shard(scene, cfg).copy()
    apply("v", 0, timed=False)
    same = bool(np.array_equal(r.render_shard(scene, cfg).view(np.uint32), film_b.view(np.uint32)))
    info = {"triangles_of_the_mesh": n_tris, "vertices_of_the_mesh": int(len(rest)), "lds_resident": which == "cfg2", "width": w, "height": h, "spp": spp,
            "ms_per_frame": {k: stats(v) for k, v in per_frame.items()},
            "deform_call_host_ms": stats(call_ms["b"]), "deform_call_device_ms": stats(device_ms["b"]), "deform_bytes": nbytes["b"],
            "deform_vertices_call_host_ms": stats(call_ms["v"]), "deform_vertices_call_device_ms": stats(device_ms["v"]), "deform_vertices_bytes": nbytes["v"],
            "same_film_by_records_and_by_vertices": same,
            "set_mesh_positions_host_ms": stats(set_positions_ms), "set_mesh_vertices_host_ms": stats(set_vertices_ms),
            "materialise_host_ms": stats(materialise_ms), "mesh_topology_registration_ms": stats(register_ms)}
    scene.close()
    lib.spt_free_pinned(ptr)
    return info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--grid", type=int, default=710, help="quads per side of the generated grid (710: 1 008 200 triangles)")
    ap.add_argument("--grid-spp", type=int, default=16)
    ap.add_argument("--grid-frames", type=int, default=40)
    ap.add_argument("--grid-block", type=int, default=10)
    ap.add_argument("--only", choices=["cfg2", "grid"], help="one of the runs (the other is kept from the file that is there)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_vertices_cost.json"))
    args = ap.parse_args()
    import bench
    spt = bench.load_pkg()
    if spt.device_count() < 1:
        sys.exit("scene_vertices_cost: no GPU (a time taken elsewhere says nothing)")
    out = {"what": "tools/scene_vertices_cost.py on one MI355X: ms per frame (host clock around blocks of frames ending in spt_render_wait; median and "
                   "spread over the blocks), loops alternating block by block; see the tool's docstring",
           "runs": {}}
    if args.only and os.path.exists(args.out):
        with open(args.out) as f:
            out["runs"] = json.load(f).get("runs", {})
    for which in ("cfg2", "grid"):
        if not args.only or args.only == which:
            os.environ.pop("SPT_NO_LDS_GEO", None)
            out["runs"][which] = run(spt, args, which)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
