"""The scene files of the scene-update tests (tests/test_scene_update_host.py, tests/test_gpu_scene_update.py), written into a
directory of the test's: an OBJ cube instanced twice, two spheres (one emissive), a floor, a point light, the power_is sampler.
A and B differ in instance transforms only; in B the left cube stands in the right half of the image and the lamp is scaled
differently (so the shape light's power, and with it the alias table, differs too)."""
import copy
import json
import os

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
f 1/1/1 2/1/1 3/1/1
f 1/1/1 3/1/1 4/1/1
f 5/1/2 6/1/2 7/1/2
f 5/1/2 7/1/2 8/1/2
f 8/1/3 7/1/3 3/1/3
f 8/1/3 3/1/3 2/1/3
f 5/1/4 1/1/4 4/1/4
f 5/1/4 4/1/4 6/1/4
f 6/1/5 4/1/5 3/1/5
f 6/1/5 3/1/5 7/1/5
f 5/1/6 8/1/6 2/1/6
f 5/1/6 2/1/6 1/1/6
"""

PLANE_OBJ = """v -1 0 -1
v -1 0 1
v 1 0 1
v 1 0 -1
vt 0 0
vn 0 1 0
f 1/1/1 2/1/1 3/1/1
f 1/1/1 3/1/1 4/1/1
"""

TRANSFORM_KEYS = ("matrix", "scale", "rotate", "translate")

TRANSFORMS_A = {
    "floor": {"scale": [4.0, 1.0, 4.0], "translate": [0.0, -1.0, 0.0]},
    "cube_l": {"scale": [0.5, 0.8, 0.5], "rotate": [0.0, 25.0, 0.0], "translate": [-1.7, -0.2, 0.0]},
    "cube_r": {"scale": [0.4, 0.4, 0.4], "rotate": [15.0, 40.0, 0.0], "translate": [1.6, -0.6, 0.8]},
    "ball": {"scale": [0.6, 0.6, 0.6], "translate": [0.2, -0.4, -0.8]},
    "lamp": {"scale": [0.3, 0.3, 0.3], "translate": [-0.4, 1.9, 1.0]},
}
TRANSFORMS_B = {
    "floor": {"scale": [4.0, 1.0, 4.0], "translate": [0.0, -1.0, 0.0]},
    "cube_l": {"scale": [0.5, 0.8, 0.5], "rotate": [0.0, -35.0, 10.0], "translate": [1.9, -0.2, -0.4]},   # left half -> right half
    "cube_r": {"scale": [0.4, 0.4, 0.4], "rotate": [15.0, 40.0, 0.0], "translate": [-1.2, -0.6, 1.2]},
    "ball": {"scale": [0.6, 0.6, 0.6], "translate": [-0.3, -0.4, -1.0]},
    "lamp": {"scale": [0.45, 0.3, 0.4], "translate": [0.6, 2.1, 0.6]},
}


def scene_dict(transforms, aggregate="bvh", bulb=(2.0, 2.5, 2.5)):
    d = {
        "cameras": [{"type": "perspective", "name": "main", "eye": [0.0, 1.2, 6.0], "forward": [0.0, -0.2, -1.0], "up": [0.0, 1.0, 0.0], "fov": 45.0}],
        "textures": [{"type": "scalar", "name": "white", "value": [0.8, 0.8, 0.8]}, {"type": "scalar", "name": "red", "value": [0.75, 0.2, 0.15]},
                     {"type": "scalar", "name": "blue", "value": [0.2, 0.3, 0.8]}],
        "materials": [{"type": "lambert", "name": "m_white", "albedo": "white"}, {"type": "lambert", "name": "m_red", "albedo": "red"},
                      {"type": "lambert", "name": "m_blue", "albedo": "blue"}],
        "mediums": [],
        "primitives": [{"type": "sphere", "name": "unit_sphere", "radius": 1.0}, {"type": "trimesh", "name": "cube", "obj_file": "models/cube.obj"},
                       {"type": "trimesh", "name": "plane", "obj_file": "models/plane.obj"}],
        "surfaces": [{"name": "s_lamp", "material": "m_white", "emissive": [9.0, 8.0, 6.0]}],
        "instances": [
            {"name": "floor", "primitive": "plane", "material": "m_white"},
            {"name": "cube_l", "primitive": "cube", "material": "m_red"},
            {"name": "cube_r", "primitive": "cube", "material": "m_blue"},
            {"name": "ball", "primitive": "unit_sphere", "material": "m_white"},
            {"name": "lamp", "primitive": "unit_sphere", "surface": "s_lamp"},
        ],
        "lights": [{"type": "point", "name": "bulb", "position": list(bulb), "strength": [7.0, 7.0, 8.0]}],
        "light_sampler": "power_is",
        "aggregate": aggregate,
    }
    for inst in d["instances"]:
        inst.update(copy.deepcopy(transforms[inst["name"]]))
    return d


def write_models(directory):
    os.makedirs(os.path.join(directory, "models"), exist_ok=True)
    for name, text in (("cube.obj", CUBE_OBJ), ("plane.obj", PLANE_OBJ)):
        with open(os.path.join(directory, "models", name), "w") as f:
            f.write(text)


def write_scene(directory, file_name, transforms, **kw):
    write_models(directory)
    path = os.path.join(str(directory), file_name)
    with open(path, "w") as f:
        json.dump(scene_dict(transforms, **kw), f)
    return path


def write_renderer(directory, spp=4, max_depth=4, file_name="pt.json"):
    path = os.path.join(str(directory), file_name)
    with open(path, "w") as f:
        json.dump({"type": "pt", "max_depth": max_depth, "sampler": {"type": "recurrence", "spp": spp}, "filter": {"type": "box", "radius": 0.5}}, f)
    return path


def fwd_by_name(scene, names):
    """{name: the 12 floats of spt_instance::fwd} of a loaded scene."""
    inst = scene.array("instances")
    return {n: inst[scene.instance_index(n)]["fwd"].copy() for n in names}


DYNAMIC_FIELDS = ("instances", "tlas_nodes", "lights")


def dynamic_bytes(spt, scene):
    """The four arrays an update replaces, as bytes: instances, tlas_nodes, lights and the alias table's props / u / k."""
    import ctypes as C
    out = {f: scene.array(f).tobytes() for f in DYNAMIC_FIELDS}
    d = scene.desc
    n = d.light_alias.n
    out["alias_n"] = n
    for f, ty in (("props", C.c_float), ("u", C.c_float), ("k", C.c_uint32)):
        out["alias_" + f] = C.string_at(getattr(d.light_alias, f), n * C.sizeof(ty)) if n else b""
    return out
