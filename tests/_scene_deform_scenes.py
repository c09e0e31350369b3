"""The scene files of the mesh-deformation tests (tests/test_scene_deform_host.py, tests/test_gpu_scene_deform.py), written into a
directory of the test's: a 12 x 12-quad cloth (288 triangles), a cube instanced twice (one instance scaled non-uniformly and
rotated), a one-triangle mesh, a five-triangle fan, an emissive two-triangle quad (a shape light), a sphere and a point light.
The deformations are functions of the vertex positions a loaded scene reports (Scene.mesh_positions), so they do not depend on the
loader's vertex order."""
import json
import os

import numpy as np

f32 = np.float32

CUBE_OBJ = """v 1 -1 -1
v 1 1 -1
v 1 1 1
v 1 -1 1
v -1 -1 -1
v -1 -1 1
v -1 1 1
v -1 1 -1
vn 1 0 0
vn -1 0 0
vn 0 1 0
vn 0 -1 0
vn 0 0 1
vn 0 0 -1
vt 0 0
vt 1 0
vt 1 1
vt 0 1
f 1/1/1 2/2/1 3/3/1
f 1/1/1 3/3/1 4/4/1
f 5/1/2 6/2/2 7/3/2
f 5/1/2 7/3/2 8/4/2
f 8/1/3 7/2/3 3/3/3
f 8/1/3 3/3/3 2/4/3
f 5/1/4 1/2/4 4/3/4
f 5/1/4 4/3/4 6/4/4
f 6/1/5 4/2/5 3/3/5
f 6/1/5 3/3/5 7/4/5
f 5/1/6 8/2/6 2/3/6
f 5/1/6 2/3/6 1/4/6
"""

QUAD_OBJ = """v -1 0 -1
v -1 0 1
v 1 0 1
v 1 0 -1
vt 0 0
vt 0 1
vt 1 1
vt 1 0
vn 0 -1 0
f 1/1/1 3/3/1 2/2/1
f 1/1/1 4/4/1 3/3/1
"""

TRI1_OBJ = """v -1 0 0
v 1 0 0
v 0 1.5 0.2
vt 0 0
vt 1 0
vt 0.5 1
vn 0 0 1
f 1/1/1 2/2/1 3/3/1
"""

# a fan of five triangles around one vertex: its tree has a node with fewer than four children
TRI5_OBJ = """v 0 0 0
v 1 0 0
v 0.8 0.7 0.1
v 0.2 1.0 0.3
v -0.6 0.8 0.1
v -1 0.1 0
v -0.7 -0.7 0.2
vt 0.5 0.5
vt 1 0.5
vt 0.9 0.9
vt 0.6 1
vt 0.2 0.9
vt 0 0.5
vt 0.2 0.1
vn 0 0 1
f 1/1/1 2/2/1 3/3/1
f 1/1/1 3/3/1 4/4/1
f 1/1/1 4/4/1 5/5/1
f 1/1/1 5/5/1 6/6/1
f 1/1/1 6/6/1 7/7/1
"""


def grid_obj(n, height=lambda x, z: 0.0 * x):
    """An n x n-quad grid over [-1, 1]^2 in the xz plane (2 n^2 triangles), with uvs and up normals."""
    k = np.arange(n + 1)
    x, z = np.meshgrid(k / n * 2.0 - 1.0, k / n * 2.0 - 1.0)      # row j: z, column i: x
    y = height(x, z)
    lines = ["v %r %r %r" % (float(a), float(b), float(c)) for a, b, c in zip(x.ravel(), y.ravel(), z.ravel())]
    lines += ["vt %r %r" % (float(a), float(b)) for a, b in zip((x.ravel() + 1) / 2, (z.ravel() + 1) / 2)]
    lines.append("vn 0 1 0")
    for j in range(n):
        for i in range(n):
            a, b, c, d = j * (n + 1) + i + 1, j * (n + 1) + i + 2, (j + 1) * (n + 1) + i + 2, (j + 1) * (n + 1) + i + 1
            lines += ["f %d/%d/1 %d/%d/1 %d/%d/1" % (a, a, d, d, c, c), "f %d/%d/1 %d/%d/1 %d/%d/1" % (a, a, c, c, b, b)]
    return "\n".join(lines) + "\n"


MESHES = ("cloth", "cube", "tri1", "tri5", "quad")          # the trimesh primitives, by name
BIG_TRIANGLES = 2 * 174 * 174                                # the mesh no test names (scene_dict(big=True)): 60 552 triangles


def scene_dict(aggregate="bvh", light_sampler="uniform", big=False):
    d = {
        "cameras": [{"type": "perspective", "name": "main", "eye": [0.0, 1.6, 6.5], "forward": [0.0, -0.25, -1.0], "up": [0.0, 1.0, 0.0], "fov": 45.0}],
        "textures": [{"type": "scalar", "name": "white", "value": [0.8, 0.8, 0.8]}, {"type": "scalar", "name": "red", "value": [0.75, 0.2, 0.15]},
                     {"type": "scalar", "name": "blue", "value": [0.2, 0.3, 0.8]}, {"type": "scalar", "name": "green", "value": [0.2, 0.7, 0.25]}],
        "materials": [{"type": "lambert", "name": "m_white", "albedo": "white"}, {"type": "lambert", "name": "m_red", "albedo": "red"},
                      {"type": "lambert", "name": "m_blue", "albedo": "blue"}, {"type": "lambert", "name": "m_green", "albedo": "green"}],
        "mediums": [],
        "primitives": [{"type": "sphere", "name": "unit_sphere", "radius": 1.0}] +
                      [{"type": "trimesh", "name": n, "obj_file": "models/%s.obj" % n} for n in MESHES],
        "surfaces": [{"name": "s_lamp", "material": "m_white", "emissive": [9.0, 8.0, 6.0], "double_sided": True},
                     {"name": "s_tri1", "material": "m_green", "double_sided": True}, {"name": "s_tri5", "material": "m_red", "double_sided": True},
                     {"name": "s_cloth", "material": "m_white", "double_sided": True}],
        "instances": [
            {"name": "cloth", "primitive": "cloth", "surface": "s_cloth", "scale": [3.0, 1.0, 3.0], "translate": [0.0, -1.0, 0.0]},
            {"name": "cube_a", "primitive": "cube", "material": "m_red", "scale": [0.5, 0.5, 0.5], "translate": [-1.6, -0.3, 0.2]},
            {"name": "cube_b", "primitive": "cube", "material": "m_blue", "scale": [0.3, 0.7, 0.45], "rotate": [20.0, 35.0, 10.0], "translate": [1.5, -0.1, 0.6]},
            {"name": "one", "primitive": "tri1", "surface": "s_tri1", "scale": [0.6, 0.6, 0.6], "translate": [-0.3, -0.6, 1.4]},
            {"name": "fan", "primitive": "tri5", "surface": "s_tri5", "scale": [0.7, 0.7, 0.7], "rotate": [0.0, -20.0, 0.0], "translate": [0.9, 0.4, -0.9]},
            {"name": "lamp", "primitive": "quad", "surface": "s_lamp", "scale": [0.6, 1.0, 0.6], "translate": [-0.2, 2.2, 0.4]},
            {"name": "ball", "primitive": "unit_sphere", "material": "m_white", "scale": [0.5, 0.5, 0.5], "translate": [0.0, -0.4, -0.6]},
        ],
        "lights": [{"type": "point", "name": "bulb", "position": [2.0, 2.5, 2.5], "strength": [5.0, 5.0, 6.0]}],
        "light_sampler": light_sampler,
        "aggregate": aggregate,
    }
    if big:
        d["primitives"].append({"type": "trimesh", "name": "terrain", "obj_file": "models/terrain.obj"})
        d["instances"].append({"name": "terrain", "primitive": "terrain", "material": "m_green", "scale": [6.0, 1.0, 6.0], "translate": [0.0, -1.6, 0.0]})
    return d


def write_models(directory, big=False):
    os.makedirs(os.path.join(str(directory), "models"), exist_ok=True)
    models = [("cube.obj", CUBE_OBJ), ("quad.obj", QUAD_OBJ), ("tri1.obj", TRI1_OBJ), ("tri5.obj", TRI5_OBJ), ("cloth.obj", grid_obj(12))]
    if big:
        models.append(("terrain.obj", grid_obj(174, lambda x, z: 0.1 * np.sin(5 * x) * np.cos(4 * z))))
    for name, text in models:
        path = os.path.join(str(directory), "models", name)
        if not os.path.exists(path):
            with open(path, "w") as f:
                f.write(text)


def write_scene(directory, file_name, **kw):
    write_models(directory, big=kw.get("big", False))
    path = os.path.join(str(directory), file_name)
    with open(path, "w") as f:
        json.dump(scene_dict(**kw), f)
    return path


# ---- deformations: new positions from the loaded ones ----------------------------------------------------------------------------

def wave(p, phase=0.0, amp=0.25):
    """A sinusoidal wave on the cloth."""
    q = p.copy()
    q[:, 1] += (amp * np.sin(3.0 * p[:, 0] + phase) * np.cos(2.0 * p[:, 2])).astype(f32)
    return q


def shear(p, k=0.4):
    q = p.copy()
    q[:, 0] += f32(k) * p[:, 1]
    return q


def bend(p, k=0.3):
    """Bent along its diagonal and tapered (a four-vertex quad changes its shape and its area)."""
    q = p.copy()
    q[:, 1] -= f32(k) * p[:, 0] * p[:, 2]
    q[:, 0] += f32(0.25) * p[:, 0] * p[:, 2]
    return q


def smooth(p, rng, amp=0.2):
    """A random smooth displacement: one low-frequency sine per axis."""
    q = p.copy()
    for k in range(3):
        w = rng.uniform(0.5, 3.0, size=3)
        q[:, k] += (amp * rng.uniform(0.2, 1.0) * np.sin(p @ w + rng.uniform(0, 6.28))).astype(f32)
    return q


DEFORMED = {"cloth": wave, "cube": shear, "quad": bend}      # the deformation of the parity tests


def tri_pos_from_vertices(positions, faces):
    """The (n, 3, 3) corner positions of faces (n, 3) over vertex positions (v, 3)."""
    return np.asarray(positions, dtype=f32)[np.asarray(faces)]


def mesh_tri_pos(scene, mesh):
    """The (tri_count, 3, 3) corner positions of mesh index `mesh` in a loaded scene's descriptor."""
    m = scene.array("meshes")[mesh]
    tp = scene.array("tri_pos")[int(m["tri_first"]):int(m["tri_first"]) + int(m["tri_count"])]
    return np.stack([tp["p0"], tp["p1"], tp["p2"]], axis=1)
