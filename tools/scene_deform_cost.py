#!/usr/bin/env python3
"""What deforming a mesh costs per frame, on one GPU -> profiles/scene_deform_cost.json.

Two runs.  "cfg2": scenes_amd/cfg2_cube.json + pt.json at the bench's headline size (LDS-resident geometry: a deformation builds
the cube's tree again on the host and writes the blob whole).  "grid": a generated displaced grid of >= 1 M triangles under a point
light (the large-scene form: the triangles are rewritten and the BLAS is refitted on the device).  Per run three loops after a
warm-up, timed in blocks: a host clock around a block that ends in spt_render_wait, so a block's time over its frames is the
steady-state time per frame; the median over the blocks and their spread are reported.  The loops alternate block by block.

  a  spt_render with SPT_RENDER_ASYNC into a page-locked film, only the camera moving
  b  the same with the mesh deformed before every frame: spt_scene_deform with records made beforehand (two states, alternating),
     so the loop holds the library's call and nothing of the loader
  c  the same animation without spt_scene_deform: destroy the device scene, create it from the edited descriptor, render

Per call (loop b): the host time of the call, the time its copies and kernels took on the device (HIP events around them:
spt_debug_render_info, counter 6, read in a pass of its own outside the timed blocks) and the bytes it copied (counter 5).  Also the
host time of Scene.set_mesh_positions, the loader's part of an animation that goes through it.

Refit-tree cost ("grid"): spt_render on the scene after a small deformation (1 % of the extent) and after a large one (the vertices
shuffled across the extent), against a scene freshly created from the same geometry.  The ratio says when to recreate.

Also spt_scene_create: the creation records three numbers per mesh for the refit.  Of the grid, the median of the creations the run
makes; "cfg5_scene_create": of cfg5 (998 k triangles), in a process of its own, and with --parent-lib DIR on the libraries of the
commit before as well, alternating.

  python tools/scene_deform_cost.py [--only cfg2|grid|cfg5_scene_create] [--parent-lib DIR] [--grid 710] [--frames 100] [--block 10]
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
f32 = np.float32


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "spread": round(max(xs) - min(xs), 4), "n": len(xs)}


def write_grid_scene(directory, n):
    """An n x n-quad displaced grid (2 n^2 triangles) under a point light, written once."""
    os.makedirs(os.path.join(directory, "models"), exist_ok=True)
    obj = os.path.join(directory, "models", "grid_%d.obj" % n)
    if not os.path.exists(obj):
        k = np.arange(n + 1)
        x, z = np.meshgrid(k / n * 2.0 - 1.0, k / n * 2.0 - 1.0)
        y = 0.08 * np.sin(9 * x) * np.cos(7 * z)
        v = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
        j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        a = (j * (n + 1) + i + 1).ravel()
        b, c, d = a + 1, a + n + 2, a + n + 1
        faces = np.concatenate([np.stack([a, d, c], axis=1), np.stack([a, c, b], axis=1)])
        with open(obj, "w") as f:
            np.savetxt(f, v, fmt="v %.7g %.7g %.7g")
            np.savetxt(f, np.stack([(x.ravel() + 1) / 2, (z.ravel() + 1) / 2], axis=1), fmt="vt %.7g %.7g")
            f.write("vn 0 1 0\n")
            np.savetxt(f, np.stack([faces[:, 0], faces[:, 0], faces[:, 1], faces[:, 1], faces[:, 2], faces[:, 2]], axis=1), fmt="f %d/%d/1 %d/%d/1 %d/%d/1")
    scene = {
        "cameras": [{"type": "perspective", "name": "main", "eye": [0.0, 2.2, 4.5], "forward": [0.0, -0.45, -1.0], "up": [0.0, 1.0, 0.0], "fov": 45.0}],
        "textures": [{"type": "scalar", "name": "white", "value": [0.8, 0.8, 0.8]}],
        "materials": [{"type": "lambert", "name": "m_white", "albedo": "white"}],
        "mediums": [], "surfaces": [],
        "primitives": [{"type": "trimesh", "name": "grid", "obj_file": "models/grid_%d.obj" % n}],
        "instances": [{"name": "grid", "primitive": "grid", "material": "m_white", "scale": [2.0, 1.0, 2.0]}],
        "lights": [{"type": "point", "name": "p0", "position": [1.5, 3.0, 2.0], "strength": [9.0, 9.0, 9.0]}],
    }
    path = os.path.join(directory, "grid_%d.json" % n)
    with open(path, "w") as f:
        json.dump(scene, f)
    return path


class State:
    """What one spt_scene_deform call takes, copied out of a host scene as it stands."""

    def __init__(self, scene, mesh):
        m = scene.array("meshes")[mesh]
        a, b = int(m["tri_first"]), int(m["tri_first"]) + int(m["tri_count"])
        self.tri_pos, self.tri_attr = scene.array("tri_pos")[a:b].copy(), scene.array("tri_attr")[a:b].copy()
        self.instances, self.lights, self.tlas = scene.array("instances"), scene.array("lights"), scene.array("tlas_nodes")


def run(spt, args, which):
    if which == "cfg2":
        path, name, spp = os.path.join(ROOT, "scenes_amd", "cfg2_cube.json"), "cube", args.spp
        deform = lambda p, t: (p * np.array([1.0 + 0.2 * math.sin(t), 1.0, 1.0 + 0.2 * math.cos(t)], dtype=f32)).astype(f32)
        frames, block, c_block = args.frames, args.block, 2                # (a creation takes about a second: profiles/scene_update_cost.json)
    else:
        path, name, spp = write_grid_scene(os.path.join(ROOT, "scenes_amd", "generated"), args.grid), "grid", args.grid_spp
        deform = lambda p, t: (p + np.stack([0 * p[:, 0], 0.01 * np.sin(6 * p[:, 0] + t) * np.cos(5 * p[:, 2]), 0 * p[:, 0]], axis=1)).astype(f32)
        frames, block, c_block = args.grid_frames, args.grid_block, 1      # (a creation builds a binned-SAH tree over the mesh on the host)
    t0 = time.perf_counter()
    scene = spt.load_scene(path)
    load_s = time.perf_counter() - t0
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
    create_ms, set_ms = [], []

    def camera():
        if which == "cfg2":
            t = 0.002 * frame[0]
            eye = (7.0 * math.sin(t), 0.0, 7.0 * math.cos(t))
            return spt.make_camera(eye, (-eye[0], 0.0, -eye[2]), (0.0, 1.0, 0.0), 45.0)
        t = 0.002 * frame[0]
        eye = (4.5 * math.sin(t), 2.2, 4.5 * math.cos(t))
        return spt.make_camera(eye, (-eye[0], -2.0, -eye[2]), (0.0, 1.0, 0.0), 45.0)

    def set_positions(p):
        t0 = time.perf_counter()
        scene.set_mesh_positions(name, p)
        set_ms.append((time.perf_counter() - t0) * 1e3)

    def device_scene():      # (timed when it creates)
        if 0 not in scene._device_scenes:
            t0 = time.perf_counter()
            scene.device_scene(0)
            create_ms.append((time.perf_counter() - t0) * 1e3)
        return scene.device_scene(0)

    # the two states loops b and c alternate between, records made beforehand
    states = []
    for t in (0.7, 2.1):
        set_positions(deform(rest, t))
        states.append(State(scene, mesh))
    ds = device_scene()      # created on state 1's geometry
    call_ms = []

    def apply(k, timed=True):
        s = states[k % 2]
        t0 = time.perf_counter()
        scene.device_scene(0).update_arrays(s.instances, s.lights, tlas_nodes=s.tlas, meshes={mesh: (s.tri_pos, s.tri_attr)})
        if timed:
            call_ms.append((time.perf_counter() - t0) * 1e3)

    def frame_a():
        r.render_shard(scene, spt.OutputConfig(w, h, None, camera()), film=film, wait=False)

    def frame_b():
        apply(frame[0])
        r.render_shard(scene, spt.OutputConfig(w, h, None, camera()), film=film, wait=False)

    def frame_c():
        scene.close_device_scene(0)                     # spt_render_wait + spt_scene_destroy
        device_scene()                                  # spt_scene_create from the descriptor as it stands
        r.render_shard(scene, spt.OutputConfig(w, h, None, camera()), film=film, wait=False)

    loops = {"a_camera_only": (frame_a, block), "b_scene_deform": (frame_b, block), "c_destroy_create": (frame_c, c_block)}
    per_frame = {k: [] for k in loops}
    for key, (fn, _) in loops.items():       # warm-up: workspace, code objects, the refit's scratch and heights
        for _ in range(1 if key == "c_destroy_create" else 3):
            fn()
            frame[0] += 1
        r.wait(scene)
    call_ms.clear()
    for _ in range(-(-frames // block)):
        for key, (fn, n) in loops.items():
            r.wait(scene)
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
                frame[0] += 1
            r.wait(scene)
            per_frame[key].append((time.perf_counter() - t0) * 1e3 / n)
            print("[%s] %s: %.3f ms per frame" % (which, key, per_frame[key][-1]), file=sys.stderr, flush=True)
    # per call, in a pass of its own: the queue is empty before each call, counter 6 waits for the call's events
    ds = device_scene()
    device_ms = []
    for k in range(10):
        r.wait(scene)
        apply(k, timed=False)
        device_ms.append(ds.render_info(6) / 1e6)
    info = {"triangles_of_the_mesh": n_tris, "lds_resident": which == "cfg2", "width": w, "height": h, "spp": spp, "load_scene_s": round(load_s, 3),
            "ms_per_frame": {k: stats(v) for k, v in per_frame.items()},
            "deform_call_host_ms": stats(call_ms), "deform_call_device_ms": stats(device_ms), "deform_bytes": ds.render_info(5),
            "set_mesh_positions_host_ms": stats(set_ms), "scene_create_ms": stats(create_ms)}
    if which == "grid":
        info["refit_tree"] = refit_tree_cost(spt, scene, r, path, name, rest, w, h, set_positions)
    scene.close()
    lib.spt_free_pinned(ptr)
    return info


def refit_tree_cost(spt, scene, r, path, name, rest, w, h, set_positions):
    """spt_render (synchronous, median of 7) on the live scene deformed from the file's positions, against a fresh scene of the same geometry."""
    cfg = spt.OutputConfig(w, h)

    def render_ms(sc):
        out = []
        r.render_shard(sc, cfg)
        for _ in range(7):
            t0 = time.perf_counter()
            r.render_shard(sc, cfg)
            out.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(out)

    rng = np.random.default_rng(5)
    extent = float((rest.max(axis=0) - rest.min(axis=0)).max())
    cases = {"small_1_percent_of_the_extent": (rest + rng.uniform(-0.01 * extent, 0.01 * extent, size=rest.shape)).astype(f32),
             "medium_25_percent_of_the_extent": (rest + 0.25 * extent * np.sin(3.0 * rest[:, [2, 0, 1]] + 1.0)).astype(f32),
             "large_vertices_shuffled": rest[rng.permutation(len(rest))].copy()}
    out = {}
    for key, pos in cases.items():
        scene.close_device_scene(0)
        set_positions(rest)
        ds = scene.device_scene(0)          # the tree of the file's positions
        set_positions(pos)
        ds.update()                         # refitted
        refit = render_ms(scene)
        film_refit = r.render_shard(scene, cfg).copy()
        scene.close_device_scene(0)
        out[key] = {"render_ms_refitted": round(refit, 3)}
        try:
            fresh = render_ms(scene)        # device_scene(0) inside: built over the deformed positions
        except spt.SptError as e:           # (a tree over triangles that span the whole extent can outgrow the traversal stack)
            out[key]["fresh_scene_refused"] = str(e)
            continue
        same = bool(np.array_equal(r.render_shard(scene, cfg).view(np.uint32), film_refit.view(np.uint32)))
        out[key].update({"render_ms_fresh": round(fresh, 3), "ratio": round(refit / fresh, 3), "same_film": same})
    return out


def cfg5_create_child():
    """spt_scene_create of cfg5 (scenes_amd/make_scenes.py: a 998 k-triangle mesh) on the libraries of this process, 7 times: one JSON line."""
    import bench
    sys.path.insert(0, os.path.join(ROOT, "scenes_amd"))
    import make_scenes
    spt = bench.load_pkg()
    sc = spt.load_scene(os.path.join(make_scenes.make_full(), "cfg5_blob_medium.json"))
    ms = []
    for _ in range(7):
        t0 = time.perf_counter()
        sc.device_scene(0)
        ms.append((time.perf_counter() - t0) * 1e3)
        sc.close_device_scene(0)
    print(json.dumps({"triangles": int(sc.desc.n_tris), "first_creation_ms": round(ms[0], 1), "later_creations_ms": stats(ms[1:])}))


def cfg5_create(parent_lib):
    """The creation records three numbers per mesh for the refit: spt_scene_create of cfg5 on this tree's libraries and, with
    --parent-lib DIR, on the libraries in DIR (a build of the commit before), each in a process of its own, alternating twice."""
    import subprocess
    out = {"this_tree": [], "parent_lib": []}
    for _ in range(2):
        for key, lib_dir in (("this_tree", None), ("parent_lib", parent_lib)):
            if key == "parent_lib" and not parent_lib:
                continue
            env = dict(os.environ)
            env.pop("SPT_LIB_DIR", None)
            if lib_dir:
                env["SPT_LIB_DIR"] = os.path.abspath(lib_dir)
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--cfg5-child"], env=env, capture_output=True, text=True, timeout=600)
            if res.returncode != 0:
                sys.exit("scene_deform_cost: the cfg5 child failed: " + res.stderr[-2000:])
            out[key].append(json.loads(res.stdout.strip().splitlines()[-1]))
            print("[cfg5_scene_create] %s: %s" % (key, out[key][-1]), file=sys.stderr, flush=True)
    if not parent_lib:
        del out["parent_lib"]
    return out


def main():
    if "--cfg5-child" in sys.argv:
        cfg5_create_child()
        return
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
    ap.add_argument("--only", choices=["cfg2", "grid", "cfg5_scene_create"], help="one of the runs (the others are kept from the file that is there)")
    ap.add_argument("--parent-lib", metavar="DIR", help="cfg5_scene_create: also on the libraries in DIR (SPT_LIB_DIR), for a before / after")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_deform_cost.json"))
    args = ap.parse_args()
    import bench
    spt = bench.load_pkg()
    if spt.device_count() < 1:
        sys.exit("scene_deform_cost: no GPU (a time taken elsewhere says nothing)")
    out = {"what": "tools/scene_deform_cost.py on one MI355X: ms per frame (host clock around blocks of frames ending in spt_render_wait; median and "
                   "spread over the blocks), loops alternating block by block; see the tool's docstring",
           "runs": {}}
    if args.only and os.path.exists(args.out):
        with open(args.out) as f:
            out["runs"] = json.load(f).get("runs", {})
    for which in ("cfg2", "grid"):
        if not args.only or args.only == which:
            os.environ.pop("SPT_NO_LDS_GEO", None)
            out["runs"][which] = run(spt, args, which)
    if not args.only or args.only == "cfg5_scene_create":
        out["runs"]["cfg5_scene_create"] = cfg5_create(args.parent_lib)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
