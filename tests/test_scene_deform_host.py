"""Moving the vertices of a loaded mesh on the host (spt_host_scene_mesh_positions / _set_mesh_positions) and the layout of
spt_mesh_deform: nothing here needs a device.

The contract of set_mesh_positions: the mesh's tri_pos / tri_attr range is rewritten in place from the new vertices (triangle k
stays the same face), the boxes of its caller-side BLAS are refitted over the unchanged topology, its instances' boxes, the TLAS,
the shape lights' power and the alias table follow; the file's own positions give the loaded descriptor back byte for byte."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _scene_deform_scenes as S
import _util

spt = _util.load_pkg()
f32 = np.float32
FIELDS = ("tlas_nodes", "blas_nodes", "instances", "meshes", "tri_pos", "tri_attr", "spheres", "surfaces", "materials", "lights")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("scene_deform_host")
    return {"dir": d, "uniform": S.write_scene(d, "uniform.json"), "power_is": S.write_scene(d, "power_is.json", light_sampler="power_is")}


def _bytes(sc):
    out = {f: sc.array(f).tobytes() for f in FIELDS}
    d = sc.desc
    n = d.light_alias.n
    for f, ty in (("props", C.c_float), ("u", C.c_float), ("k", C.c_uint32)):
        out["alias_" + f] = C.string_at(getattr(d.light_alias, f), n * C.sizeof(ty)) if n else b""
    return out


def _faces(sc, name):
    """(tri_count, 3) vertex indices of the mesh's triangles in descriptor order: every corner matched to the first vertex at its
    position (vertices that share a position move together under a deformation that is a function of the position)."""
    pos = sc.mesh_positions(name)
    corners = S.mesh_tri_pos(sc, sc.mesh_index(name))
    faces = np.zeros(corners.shape[:2], dtype=np.int64)
    for t in range(corners.shape[0]):
        for c in range(3):
            faces[t, c] = int(np.flatnonzero((pos == corners[t, c]).all(axis=1))[0])
    return faces


def test_positions_are_the_obj_loaders_vertices(files):
    sc = spt.load_scene(files["uniform"])
    counts = {"cloth": 169, "cube": 24, "tri1": 3, "tri5": 7, "quad": 4}      # distinct v/vt/vn tuples
    for i, name in enumerate(S.MESHES):
        assert sc.mesh_index(name) == i
        pos = sc.mesh_positions(name)
        assert pos.shape == (counts[name], 3) and pos.dtype == f32
        corners = S.mesh_tri_pos(sc, i).reshape(-1, 3)
        assert {tuple(p) for p in pos} == {tuple(p) for p in corners}
    assert np.array_equal(sc.mesh_positions("tri1"), np.array([[-1, 0, 0], [1, 0, 0], [0, 1.5, 0.2]], dtype=f32))      # first-seen order


@pytest.mark.parametrize("which", ["uniform", "power_is"])
def test_round_trip_gives_the_loaded_descriptor(files, which):
    sc = spt.load_scene(files[which])
    before = _bytes(sc)
    rest = {name: sc.mesh_positions(name) for name in S.MESHES}
    for name, fn in S.DEFORMED.items():
        sc.set_mesh_positions(name, fn(rest[name]))
    moved = _bytes(sc)
    for f in ("tri_pos", "tri_attr", "blas_nodes", "instances", "tlas_nodes", "lights"):
        assert moved[f] != before[f], f
    if which == "power_is":
        assert moved["alias_props"] != before["alias_props"]      # the quad's area, and so its power, differs
    assert moved["meshes"] == before["meshes"] and moved["surfaces"] == before["surfaces"]
    for name in S.DEFORMED:
        assert np.array_equal(sc.mesh_positions(name), S.DEFORMED[name](rest[name]))
        sc.set_mesh_positions(name, rest[name])
    assert _bytes(sc) == before


def test_records_follow_the_vertices(files):
    sc = spt.load_scene(files["uniform"])
    for name, fn in (("cloth", S.wave), ("cube", S.shear), ("quad", S.bend), ("tri5", lambda p: S.shear(p, 1.5)), ("tri1", lambda p: (p * f32(2.0)).astype(f32))):
        m = sc.mesh_index(name)
        faces = _faces(sc, name)
        others = {n: S.mesh_tri_pos(sc, sc.mesh_index(n)) for n in S.MESHES if n != name}
        attr_before = sc.array("tri_attr")
        new = fn(sc.mesh_positions(name))
        sc.set_mesh_positions(name, new)
        got = S.mesh_tri_pos(sc, m)
        assert np.array_equal(got, S.tri_pos_from_vertices(new, faces)), name      # triangle k is still face k
        for n, want in others.items():
            assert np.array_equal(S.mesh_tri_pos(sc, sc.mesh_index(n)), want), (name, n)
        mesh = sc.array("meshes")[m]
        a, b = int(mesh["tri_first"]), int(mesh["tri_first"]) + int(mesh["tri_count"])
        attr = sc.array("tri_attr")
        assert np.array_equal(attr["n"][a:b], attr_before["n"][a:b]) and np.array_equal(attr["uv"][a:b], attr_before["uv"][a:b])      # normals = None keeps them
        assert attr[:a].tobytes() == attr_before[:a].tobytes() and attr[b:].tobytes() == attr_before[b:].tobytes()
        # the caller-side BLAS: the same topology, every box exactly the bounds of what is below it
        nodes = sc.array("blas_nodes")
        first, count = int(mesh["root"]), int(mesh["node_count"])
        tri = S.mesh_tri_pos(sc, m)

        def bounds(i):
            nd = nodes[i]
            if nd["b"] & 0x80000000:
                k0, cnt = int(nd["a"]) - a, int(nd["b"] & 0x7fffffff)
                pts = tri[k0:k0 + cnt].reshape(-1, 3)
                lo, hi = pts.min(axis=0), pts.max(axis=0)
            else:
                (l0, h0), (l1, h1) = bounds(int(nd["a"])), bounds(int(nd["b"]))
                lo, hi = np.minimum(l0, l1), np.maximum(h0, h1)
            assert np.array_equal(nd["bmin"], lo) and np.array_equal(nd["bmax"], hi), (name, i)
            return lo, hi

        lo, hi = bounds(first)
        assert first <= first + count <= len(nodes)
        # every instance of the mesh: the world box of the 8 corners of the new object-space box, in the loader's arithmetic
        inst = sc.array("instances")
        users = [i for i in range(len(inst)) if inst["prim_type"][i] == 1 and inst["prim_id"][i] == m]
        assert users
        for i in users:
            fwd = inst["fwd"][i]
            c0, c1, c2, t = fwd[0:3], fwd[3:6], fwd[6:9], fwd[9:12]
            pts = []
            for c in range(8):
                p = np.array([hi[0] if c & 4 else lo[0], hi[1] if c & 2 else lo[1], hi[2] if c & 1 else lo[2]], dtype=f32)
                pts.append(((c0 * p[0] + c1 * p[1]) + c2 * p[2]) + t)
            pts = np.array(pts, dtype=f32)
            assert np.array_equal(inst["bmin"][i], pts.min(axis=0)) and np.array_equal(inst["bmax"][i], pts.max(axis=0)), (name, i)


def test_normals_and_tangents(files):
    sc = spt.load_scene(files["uniform"])
    m = sc.mesh_index("quad")
    mesh = sc.array("meshes")[m]
    a, b = int(mesh["tri_first"]), int(mesh["tri_first"]) + int(mesh["tri_count"])
    before = sc.array("tri_attr")[a:b]
    pos = sc.mesh_positions("quad")
    up = np.tile(np.array([[0.0, 1.0, 0.0]], dtype=f32), (len(pos), 1))
    sc.set_mesh_positions("quad", pos[:, [2, 1, 0]].copy(), normals=up)        # x and z swapped: the tangents follow the positions
    after = sc.array("tri_attr")[a:b]
    assert np.array_equal(after["n"], np.broadcast_to(up[0], after["n"].shape))
    assert not np.array_equal(after["t"], before["t"])
    assert np.array_equal(after["uv"], before["uv"])


def test_refusals_leave_every_array_untouched(files):
    sc = spt.load_scene(files["power_is"])
    before = _bytes(sc)
    pos = sc.mesh_positions("cloth")
    lib = spt.host_lib()

    def refused(status, name, p, normals=None):
        with pytest.raises(spt.SptError) as e:
            sc.set_mesh_positions(name, p, normals)
        assert e.value.status == status, str(e.value)
        assert _bytes(sc) == before
        assert np.array_equal(sc.mesh_positions("cloth"), pos)

    refused(102, "nobody", pos)                                  # SPT_HOST_ERR_SCHEMA
    refused(102, "unit_sphere", pos)                             # (a primitive, but no trimesh)
    refused(1, "cloth", pos[:-1])                                # a wrong count
    refused(1, "cloth", np.concatenate([pos, pos[:1]]))
    for value in (np.nan, np.inf, -np.inf):
        bad = pos.copy()
        bad[17, 1] = value
        refused(1, "cloth", bad)
        refused(1, "cloth", pos, normals=bad)
    huge = pos.copy()
    huge[3] = f32(3.0e38)                                        # finite, but the instance's box (scaled by 3) is not
    refused(1, "cloth", huge)
    n = C.c_uint32(0)
    assert lib.spt_host_scene_mesh_positions(sc._h, b"nobody", C.byref(n), None) == 102
    assert lib.spt_host_scene_mesh_positions(sc._h, None, C.byref(n), None) == 1
    assert lib.spt_host_scene_set_mesh_positions(sc._h, b"cloth", len(pos), None, None) == 1
    assert _bytes(sc) == before


def test_gltf_and_catmull_clark_meshes_are_refused():
    import json
    sc = spt.load_scene(os.path.join(_util.SCENES, "t_gltf.gltf"))
    lib = spt.host_lib()
    n = C.c_uint32(0)
    with open(os.path.join(_util.SCENES, "t_gltf.gltf")) as f:
        doc = json.load(f)
    names = [(m.get("name", "mesh_%d" % i) + "_prim_0").encode() for i, m in enumerate(doc["meshes"])]
    assert names
    for name in names:
        assert lib.spt_host_scene_mesh_positions(sc._h, name, C.byref(n), None) == 103, name      # SPT_HOST_ERR_UNSUPPORTED
    sc.close()
    sc = spt.load_scene(os.path.join(_util.SCENES, "t_catmull.json"))
    with open(os.path.join(_util.SCENES, "t_catmull.json")) as f:
        doc = json.load(f)
    cc = [p["name"] for p in doc["primitives"] if p["type"] == "catmull_clark"]
    assert cc
    for name in cc:
        with pytest.raises(spt.SptError) as e:
            sc.mesh_positions(name)
        assert e.value.status == 103
        with pytest.raises(spt.SptError) as e:
            sc.set_mesh_positions(name, np.zeros((3, 3), dtype=f32))
        assert e.value.status == 103
    sc.close()


def test_mesh_deform_layout(tmp_path):
    cc = shutil.which(os.environ.get("CC", "cc")) or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no C compiler"
    exe = str(tmp_path / "scene_deform_layout_check")
    src = os.path.join(_util.ROOT, "tests", "scene_deform_layout_check.c")
    res = subprocess.run([cc, "-Wall", "-Wextra", "-I", os.path.join(_util.ROOT, "include"), "-o", exe, src], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    c = {k: int(v) for k, v in (line.split() for line in out.stdout.splitlines())}
    assert c["SPT_ABI_VERSION"] == 14 == spt.SPT_ABI_VERSION       # additive: detected by symbol
    assert C.sizeof(spt.MeshDeform) == c["sizeof.spt_mesh_deform"]
    names = [f[0] for f in spt.MeshDeform._fields_]
    assert names == ["mesh", "tri_count", "tri_pos", "tri_attr"]
    for name in names:
        assert getattr(spt.MeshDeform, name).offset == c["spt_mesh_deform." + name], name
    assert C.sizeof(spt.TriPos) == c["sizeof.spt_tri_pos"] == 48
    assert C.sizeof(spt.TriAttr) == c["sizeof.spt_tri_attr"] == 144
    assert C.sizeof(spt.SceneUpdateDesc) == c["sizeof.spt_scene_update_desc"]      # spt_scene_update's struct is as it was
    with open(os.path.join(_util.ROOT, "include", "spt_abi.h")) as f:
        header = f.read()
    assert "spt_status spt_scene_update(spt_scene* scene, const spt_scene_update_desc* u);" in header
    assert "spt_status spt_scene_deform(spt_scene* scene, const spt_scene_update_desc* u, uint32_t n_meshes, const spt_mesh_deform* meshes);" in header
