"""Deforming a loaded mesh from vertex arrays on the host (spt_host_scene_mesh_topology / _set_mesh_vertices / _dynamic) and the
layout of spt_mesh_topology / spt_mesh_vertices: nothing here needs a device.

The contract of set_mesh_vertices: the instances, the TLAS, the lights and the alias table follow at once and are the bytes
set_mesh_positions leaves; the mesh's tri_pos / tri_attr / blas_nodes ranges are made when the descriptor is read, and are then the
bytes set_mesh_positions leaves too."""
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
    d = tmp_path_factory.mktemp("scene_vertices_host")
    return {"dir": d, "uniform": S.write_scene(d, "uniform.json"), "power_is": S.write_scene(d, "power_is.json", light_sampler="power_is")}


def _alias(a):
    n = a.n
    return {"alias_" + f: (C.string_at(getattr(a, f), n * C.sizeof(ty)) if n else b"") for f, ty in (("props", C.c_float), ("u", C.c_float), ("k", C.c_uint32))}


def _bytes(sc):
    """Every array of the descriptor (reading it makes the pending meshes)."""
    out = {f: sc.array(f).tobytes() for f in FIELDS}
    out.update(_alias(sc.desc.light_alias))
    return out


def _dynamic(sc):
    """The four arrays of spt_host_scene_dynamic, which makes nothing."""
    u = spt.SceneUpdateDesc()
    assert spt.host_lib().spt_host_scene_dynamic(sc._h, C.byref(u)) == 0
    assert u.size == C.sizeof(spt.SceneUpdateDesc) and u.flags == 0
    out = {"tlas_nodes": C.string_at(u.tlas_nodes, u.n_tlas_nodes * C.sizeof(spt.BvhNode)),
           "instances": C.string_at(u.instances, u.n_instances * C.sizeof(spt.Instance)),
           "lights": C.string_at(u.lights, u.n_lights * C.sizeof(spt.Light))}
    out.update(_alias(u.light_alias))
    return out


def _dynamic_of_desc(sc):
    b = _bytes(sc)
    return {k: b[k] for k in ("tlas_nodes", "instances", "lights", "alias_props", "alias_u", "alias_k")}


def _tilted(n):
    nrm = np.tile(np.array([[0.6, 0.8, 0.0]], dtype=f32), (n, 1))
    nrm[::2] = np.array([0.0, 0.6, 0.8], dtype=f32)
    return nrm


@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("which", ["uniform", "power_is"])
def test_vertices_give_the_bytes_of_positions(files, which, normals):
    by_pos, by_vtx = spt.load_scene(files[which]), spt.load_scene(files[which])
    loaded = _bytes(by_vtx)
    rest = {name: by_pos.mesh_positions(name) for name in S.MESHES}
    for name, fn in S.DEFORMED.items():
        nrm = _tilted(len(rest[name])) if normals and name == "cloth" else None
        by_pos.set_mesh_positions(name, fn(rest[name]), nrm)
        by_vtx.set_mesh_vertices(name, fn(rest[name]), nrm)
        assert np.array_equal(by_vtx.mesh_positions(name), fn(rest[name]))
    want = _bytes(by_pos)
    # before anything is made: the dynamic arrays are already the other scene's, the records of the pending meshes still the file's
    assert _dynamic(by_vtx) == _dynamic_of_desc(by_pos)
    assert _dynamic(by_vtx) != {k: loaded[k] for k in _dynamic(by_vtx)}
    # afterwards: every array
    got = _bytes(by_vtx)
    for f in got:
        assert got[f] == want[f], f
    assert got["tri_pos"] != loaded["tri_pos"] and got["tri_attr"] != loaded["tri_attr"] and got["blas_nodes"] != loaded["blas_nodes"]
    assert _dynamic(by_vtx) == _dynamic_of_desc(by_pos)
    # and back to the file's vertices (the normals too): the loaded descriptor
    for name in S.DEFORMED:
        by_vtx.set_mesh_vertices(name, rest[name], _file_normals(loaded, by_vtx, name) if normals and name == "cloth" else None)
    assert _bytes(by_vtx) == loaded
    by_pos.close()
    by_vtx.close()


def _file_normals(loaded, sc, name):
    """The vertex normals of the loaded file, from its tri_attr records and the topology."""
    topo = sc.mesh_topology(name)
    mesh = np.frombuffer(loaded["meshes"], dtype=np.dtype(spt.Mesh))[topo["mesh"]]
    attr = np.frombuffer(loaded["tri_attr"], dtype=np.dtype(spt.TriAttr))[int(mesh["tri_first"]):int(mesh["tri_first"]) + int(mesh["tri_count"])]
    out = np.zeros_like(topo["normals"])
    for k, face in enumerate(topo["face_of_tri"]):
        out[topo["indices"][face]] = attr["n"][k]
    return out


def test_a_pending_mesh_is_made_by_the_first_reader(files):
    """The records stay the file's until the descriptor is read: seen through the address the descriptor hands out."""
    sc = spt.load_scene(files["uniform"])
    d = sc.desc
    m = sc.mesh_index("cloth")
    first = int(d.meshes[m].tri_first)
    addr = C.addressof(d.tri_pos[first])
    before = C.string_at(addr, 48 * 4)
    sc.set_mesh_vertices("cloth", S.wave(sc.mesh_positions("cloth")))
    assert C.string_at(addr, 48 * 4) == before                # pending: nothing made
    assert C.addressof(sc.desc.tri_pos[first]) == addr        # the arrays keep their addresses
    assert C.string_at(addr, 48 * 4) != before                # ... and reading the descriptor made the records
    sc.close()


def test_an_emissive_mesh_is_made_at_once(files):
    a, b = spt.load_scene(files["power_is"]), spt.load_scene(files["power_is"])
    d = b.desc
    m = b.mesh_index("quad")
    addr = C.addressof(d.tri_pos[int(d.meshes[m].tri_first)])
    before = C.string_at(addr, 48 * 2)
    loaded_alias = _dynamic(b)["alias_props"]
    new = S.bend(a.mesh_positions("quad"))
    a.set_mesh_positions("quad", new)
    b.set_mesh_vertices("quad", new)
    assert C.string_at(addr, 48 * 2) != before                # not pending: the shape light's area needs the triangles
    assert _dynamic(b) == _dynamic_of_desc(a)
    assert _dynamic(b)["alias_props"] != loaded_alias         # the quad's area, and so its power, differs
    assert _bytes(b) == _bytes(a)
    a.close()
    b.close()


def test_refusals_leave_every_array_untouched(files):
    sc = spt.load_scene(files["power_is"])
    before = _bytes(sc)
    pos = sc.mesh_positions("cloth")
    lib = spt.host_lib()

    def refused(status, name, p, normals=None):
        with pytest.raises(spt.SptError) as e:
            sc.set_mesh_vertices(name, p, normals)
        assert e.value.status == status, str(e.value)
        assert _dynamic(sc) == {k: before[k] for k in _dynamic(sc)}
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
    quad = sc.mesh_positions("quad")                             # the emissive mesh refuses as set_mesh_positions does
    refused(1, "quad", quad[:-1])
    t = spt.MeshTopology()
    assert lib.spt_host_scene_mesh_topology(sc._h, b"nobody", C.byref(t)) == 102
    assert lib.spt_host_scene_mesh_topology(sc._h, None, C.byref(t)) == 1
    assert lib.spt_host_scene_set_mesh_vertices(sc._h, b"cloth", len(pos), None, None) == 1
    assert lib.spt_host_scene_dynamic(sc._h, None) == 1
    assert _bytes(sc) == before
    sc.close()


def test_positions_and_vertices_supersede_each_other(files):
    a, b, c = (spt.load_scene(files["uniform"]) for _ in range(3))
    rest = a.mesh_positions("cloth")
    one, two = S.wave(rest), S.wave(rest, phase=1.0, amp=0.4)
    a.set_mesh_positions("cloth", two)
    b.set_mesh_vertices("cloth", one)          # pending ...
    b.set_mesh_positions("cloth", two)         # ... and superseded
    c.set_mesh_positions("cloth", one)
    c.set_mesh_vertices("cloth", two)
    want = _bytes(a)
    assert _dynamic(b) == _dynamic_of_desc(a) and _dynamic(c) == _dynamic_of_desc(a)
    assert _bytes(b) == want and _bytes(c) == want
    for sc in (a, b, c):
        sc.close()


def test_mesh_topology_agrees_with_the_obj_file(files):
    sc = spt.load_scene(files["uniform"])
    for i, name in enumerate(S.MESHES):
        topo = sc.mesh_topology(name)
        pos = sc.mesh_positions(name)
        mesh = sc.array("meshes")[i]
        assert topo["mesh"] == i == sc.mesh_index(name)
        nt, nv = int(mesh["tri_count"]), len(pos)
        assert topo["indices"].shape == (nt, 3) and topo["indices"].dtype == np.uint32 and int(topo["indices"].max()) == nv - 1
        assert topo["uv"].shape == (nv, 2) and topo["normals"].shape == (nv, 3)
        assert sorted(topo["face_of_tri"].tolist()) == list(range(nt))      # a permutation
        # the records of the descriptor are the gather of the vertex arrays through face_of_tri and indices
        a, b = int(mesh["tri_first"]), int(mesh["tri_first"]) + nt
        tri = S.mesh_tri_pos(sc, i)
        attr = sc.array("tri_attr")[a:b]
        corners = topo["indices"][topo["face_of_tri"]]
        assert np.array_equal(tri, pos[corners]), name
        assert np.array_equal(attr["n"], topo["normals"][corners]) and np.array_equal(attr["uv"], topo["uv"][corners]), name
    # the faces in the file's order: tri1 and the first faces of the cube as written
    assert np.array_equal(sc.mesh_topology("tri1")["indices"], np.array([[0, 1, 2]], dtype=np.uint32))
    assert np.array_equal(sc.mesh_topology("tri5")["indices"], np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 5], [0, 5, 6]], dtype=np.uint32))
    assert np.array_equal(sc.mesh_topology("cube")["indices"][:2], np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32))
    assert np.array_equal(sc.mesh_topology("quad")["uv"], np.array([[0, 0], [1, 1], [0, 1], [1, 0]], dtype=f32))
    assert np.array_equal(sc.mesh_topology("quad")["normals"], np.tile(np.array([[0, -1, 0]], dtype=f32), (4, 1)))
    sc.close()


def test_scene_vertices_layout(tmp_path):
    cc = shutil.which(os.environ.get("CC", "cc")) or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no C compiler"
    exe = str(tmp_path / "scene_vertices_layout_check")
    src = os.path.join(_util.ROOT, "tests", "scene_vertices_layout_check.c")
    res = subprocess.run([cc, "-Wall", "-Wextra", "-I", os.path.join(_util.ROOT, "include"), "-o", exe, src], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    c = {k: int(v) for k, v in (line.split() for line in out.stdout.splitlines())}
    assert c["SPT_ABI_VERSION"] == 14 == spt.SPT_ABI_VERSION       # additive: detected by symbol
    for ty, struct, names in ((spt.MeshTopology, "spt_mesh_topology", ["size", "mesh", "n_vertices", "tri_count", "indices", "face_of_tri", "uv", "normals"]),
                              (spt.MeshVertices, "spt_mesh_vertices", ["mesh", "n_vertices", "positions", "normals"])):
        assert C.sizeof(ty) == c["sizeof." + struct]
        assert [f[0] for f in ty._fields_] == names
        for name in names:
            assert getattr(ty, name).offset == c[struct + "." + name], (struct, name)
    assert C.sizeof(spt.SceneUpdateDesc) == c["sizeof.spt_scene_update_desc"]      # the structs before are as they were
    assert C.sizeof(spt.MeshDeform) == c["sizeof.spt_mesh_deform"]
    with open(os.path.join(_util.ROOT, "include", "spt_abi.h")) as f:
        header = f.read()
    assert "spt_status spt_scene_deform(spt_scene* scene, const spt_scene_update_desc* u, uint32_t n_meshes, const spt_mesh_deform* meshes);" in header
    assert "spt_status spt_scene_deform_vertices(spt_scene* scene, const spt_scene_update_desc* u, uint32_t n_meshes, const spt_mesh_vertices* meshes);" in header
