"""The per-origin-triangle candidate table of include/spt_origin_cand.h, through spt_host_origin_candidates, against brute force.

A shadow or extension ray of the fused simple shade kernel starts at it.position on a triangle T and is tested only against the
triangles of one of T's four words (loose / tight, up / down).  A word may lack a triangle U only when no such ray can pass the
kernel's test of U.  Here the origin is formed in float32 one operation at a time as the kernel forms it - a ray from an eye point
that tri_test_edges accepts on T in T's object space, po = o + d t -, the shading frame, t_min and the word choice are restated the
same way (numpy does not contract), and every (origin triangle, ray, triangle) the restated test accepts with t > t_min must have
its bit set in the word the kernel would pick.  Directions cover the hemispheres with heavy weight on |wi.z| in {0, 1e-6, 1e-5,
z0 on both sides, 1e-2}, origins lie within 1e-3 of edges and vertices half of the time.  Condition: zero misses.  No GPU.
"""
import numpy as np
import pytest

import _util

f32 = np.float32
T_MIN_EPS = f32(0.0001)
Z0 = f32(1e-3)

CUBE_V = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64)
# outward winding; the two triangles of a face are neighbours in the list
CUBE_F = [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7), (1, 7, 3)]
PLANE_V = np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], dtype=np.float64)
PLANE_F = [(0, 2, 1), (0, 3, 2)]   # normal +y


@pytest.fixture(scope="module")
def spt():
    _util.ensure_cpu_build()
    return _util.load_pkg()


def flat_mesh(verts, faces):
    """(n, 9) positions and (n, 9) vertex normals: the face's own normal at its three vertices."""
    pos = np.array([[verts[a], verts[b], verts[c]] for a, b, c in faces], dtype=np.float64)
    n = np.cross(pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return pos.reshape(-1, 9).astype(f32), np.repeat(n[:, None, :], 3, axis=1).reshape(-1, 9).astype(f32)


def icosahedron():
    """Smooth normals: the vertex normal is the vertex's direction from the centre."""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, p, 0], [1, p, 0], [-1, -p, 0], [1, -p, 0], [0, -1, p], [0, 1, p], [0, -1, -p], [0, 1, -p], [p, 0, -1], [p, 0, 1], [-p, 0, -1], [-p, 0, 1]], dtype=np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    pos = np.array([[v[a], v[b], v[c]] for a, b, c in f]).reshape(-1, 9).astype(f32)
    return pos, pos.copy()


def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def instance(m, translate):
    """spt_instance of the linear map m and a translation: fwd, inv (3 columns + translation) and the normal matrix's columns, float32."""
    m = np.asarray(m, dtype=np.float64)
    t = np.asarray(translate, dtype=np.float64)
    mi = np.linalg.inv(m)
    fwd = np.concatenate([m.T.reshape(9), t]).astype(f32)
    inv = np.concatenate([mi.T.reshape(9), -mi @ t]).astype(f32)
    nrm = mi.reshape(9).astype(f32)       # the columns of the inverse transpose are the rows of the inverse
    return fwd, inv, nrm


class Scene:
    def __init__(self, parts):
        """parts: (mesh positions, mesh normals, linear map, translation)"""
        self.fwd, self.inv, self.nrm, self.pos, self.vn, self.owner = [], [], [], [], [], []
        for k, (pos, vn, m, t) in enumerate(parts):
            fwd, inv, nrm = instance(m, t)
            self.fwd.append(fwd); self.inv.append(inv); self.nrm.append(nrm)
            self.pos.append(pos); self.vn.append(vn); self.owner += [k] * len(pos)
        self.fwd, self.inv, self.nrm = (np.array(a, dtype=f32) for a in (self.fwd, self.inv, self.nrm))
        self.pos, self.vn = np.concatenate(self.pos), np.concatenate(self.vn)
        self.owner = np.array(self.owner, dtype=np.uint32)

    def table(self, spt):
        return spt.origin_candidates(self.inv, self.fwd, self.nrm, self.owner, self.pos, self.vn)

    def world(self):
        """(n, 3, 3) float64 world vertices"""
        out = np.zeros((len(self.pos), 3, 3))
        for k, p in enumerate(self.pos.astype(np.float64).reshape(-1, 3, 3)):
            f = self.fwd[self.owner[k]].astype(np.float64)
            out[k] = p @ f[:9].reshape(3, 3) + f[9:12]
        return out


# ---- the kernel's f32 operations, one at a time ---------------------------------------------------------------------------
def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def normalize(a):
    return a / np.sqrt(dot3(a, a))[..., None]


def xf_vector(m, v):
    return (m[0:3] * v[..., 0:1] + m[3:6] * v[..., 1:2]) + m[6:9] * v[..., 2:3]


def xf_point(m, p):
    return xf_vector(m, p) + m[9:12]


def tri_test_edges(p0, e1, e2, o, d):
    """trace.h: (accepted, t, v, w)"""
    q = cross3(d, e2)
    det = dot3(e1, q)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = f32(1.0) / det
        s = o - p0
        v = dot3(s, q) * inv
        rr = cross3(s, e1)
        w = dot3(d, rr) * inv
        u = f32(1.0) - v - w
        t = dot3(e2, rr) * inv
        ok = (det != 0) & (v >= 0) & (w >= 0) & (u >= 0)
    return ok, t, v, w


def local_directions(rng, n):
    """(n, 3) float32 unit vectors of the shading frame: a third uniform over the sphere, the rest at chosen |z|."""
    z = rng.uniform(-1.0, 1.0, size=n)
    special = np.array([0.0, 1e-6, 1e-5, 1e-3 * (1 - 3e-7), 1e-3, 1e-3 * (1 + 3e-7), 0.9e-3, 1.1e-3, 1e-2, 2e-3, 0.3])
    k = rng.integers(0, len(special), size=n)
    pick = rng.uniform(size=n) < 0.67
    z = np.where(pick, special[k] * rng.choice([-1.0, 1.0], size=n), z)
    phi = rng.uniform(0.0, 2.0 * np.pi, size=n)
    s = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    return np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=-1).astype(f32)


def points_on(rng, n):
    """barycentric (v, w) of n points: half of them within 1e-3 of an edge or a vertex"""
    a, b = rng.uniform(size=n), rng.uniform(size=n)
    flip = a + b > 1.0
    a, b = np.where(flip, 1.0 - a, a), np.where(flip, 1.0 - b, b)
    kind = rng.integers(0, 8, size=n)
    tiny = rng.uniform(0.0, 1e-3, size=n)
    tiny2 = rng.uniform(0.0, 1e-3, size=n)
    a = np.where(kind == 0, tiny, a); b = np.where(kind == 1, tiny, b)                         # edges v = 0, w = 0
    b = np.where(kind == 2, 1.0 - a - tiny * (1.0 - a), b)                                    # edge u = 0
    a = np.where(kind == 3, tiny, a); b = np.where(kind == 3, tiny2, b)                        # vertex p0
    return a, b


def misses(sc, words, rng, n_rays, eye_dist, double_sided):
    """Number of (origin triangle, ray, triangle) the restated kernel accepts outside the word it would pick, and how many it accepted."""
    n_tri = len(sc.pos)
    tri = sc.pos.reshape(-1, 3, 3)
    p0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]   # the blob's f32 differences
    world = sc.world()
    lo, hi = (words & np.uint64(0xffffffff)).astype(np.uint64), (words >> np.uint64(32)).astype(np.uint64)
    bad = accepted = 0
    for T in range(n_tri):
        inv_t, fwd_t, nrm_t = sc.inv[sc.owner[T]], sc.fwd[sc.owner[T]], sc.nrm[sc.owner[T]]
        # an eye on either side of T and a target on T: the camera ray (or an earlier bounce's ray) whose hit is the vertex
        bv, bw = points_on(rng, n_rays)
        target = world[T, 0] + bv[:, None] * (world[T, 1] - world[T, 0]) + bw[:, None] * (world[T, 2] - world[T, 0])
        away = rng.normal(size=(n_rays, 3))
        away /= np.linalg.norm(away, axis=1, keepdims=True)
        o = (target + away * rng.uniform(0.05, eye_dist, size=(n_rays, 1))).astype(f32)
        d = normalize((target.astype(f32) - o).astype(f32))
        ok, t, v, w = tri_test_edges(p0[T], e1[T], e2[T], xf_point(inv_t, o), xf_vector(inv_t, d))
        ok &= t > T_MIN_EPS
        po = o + d * t[:, None]                                               # point_at
        u = f32(1.0) - v - w
        vn = sc.vn[T].reshape(3, 3)
        with np.errstate(invalid="ignore", over="ignore"):
            n_obj = normalize((vn[0] * u[:, None] + vn[1] * v[:, None]) + vn[2] * w[:, None])
            normal = normalize((nrm_t[0:3] * n_obj[:, 0:1] + nrm_t[3:6] * n_obj[:, 1:2]) + nrm_t[6:9] * n_obj[:, 2:3])
            tangent = xf_vector(fwd_t, normalize(e1[T])[None, :] + np.zeros_like(n_obj))
            hit_back = dot3(d, normal) > 0
            flip = hit_back & double_sided
            zw = np.where(flip[:, None], -normal, normal)
            yw = normalize(cross3(zw, tangent))
            xw = cross3(yw, zw)
            wi = local_directions(rng, n_rays)
            dw = (xw * wi[:, 0:1] + yw * wi[:, 1:2]) + zw * wi[:, 2:3]      # Coordinate::to_world
            for kind in ("extension", "shadow"):
                wz = wi[:, 2] if kind == "extension" else dot3(zw, dw)        # samp.wi.z / to_local(ls.dir).z
                t_min = T_MIN_EPS / np.maximum(np.abs(wz), f32(0.00001))
                down = (wz < 0) != flip
                tight = np.abs(wz) >= Z0
                col = np.where(down, 3, 2)
                w_lo = np.where(tight, lo[T][col], lo[T][0] | lo[T][1])
                w_hi = np.where(tight, hi[T][col], hi[T][0] | hi[T][1])
                for U in range(n_tri):
                    inv_u = sc.inv[sc.owner[U]]
                    ok_u, t_u, _, _ = tri_test_edges(p0[U], e1[U], e2[U], xf_point(inv_u, po), xf_vector(inv_u, dw))
                    hit = ok & ok_u & (t_u > t_min)
                    bit = ((w_lo if U < 32 else w_hi) >> np.uint64(U % 32)) & np.uint64(1)
                    accepted += int(hit.sum())
                    bad += int((hit & (bit == 0)).sum())
    return bad, accepted


def popcounts(words):
    return np.array([[bin(int(x)).count("1") for x in row] for row in words])


CUBE = flat_mesh(CUBE_V, CUBE_F)
PLANE = flat_mesh(PLANE_V, PLANE_F)
ROT60 = np.array([[0.5, 0.0, 0.8660254037844386], [0.0, 1.0, 0.0], [-0.8660254037844386, 0.0, 0.5]])


def _scenes():
    rng = np.random.default_rng(7)
    out = {"unit_cube": Scene([CUBE + (ROT60, (0, 0, 0))]),
           "coincident": Scene([CUBE + (np.eye(3), (-1, 0, 0)), CUBE + (np.eye(3), (1, 0, 0))]),
           "plane_under_cubes": Scene([PLANE + (np.diag([3.0, 1.0, 3.0]), (0, -0.5, 0)), CUBE + (0.5 * rotation(rng), (-0.9, 0.4, 0.1)),
                                       CUBE + (np.diag([0.5, 0.5, 0.5]), (0.8, 0.0, 0.3))]),
           "smooth": Scene([icosahedron() + (np.eye(3), (0, 0, 0))]),
           "near_100": Scene([CUBE + (ROT60, (100.0, 99.0, -101.0))])}
    for k, s in enumerate([(0.2, 0.2, 0.2), (4.0, 4.0, 4.0), (0.2, 1.0, 4.0), (1.6, 0.5, 0.9)]):
        out["scaled_%d" % k] = Scene([CUBE + (rotation(rng) @ np.diag(s), (0.3, -0.2, 0.5))])
    for gap in (5e-5, 1e-4, 2e-4):
        out["gap_%g" % gap] = Scene([CUBE + (np.eye(3), (-1, 0, 0)), CUBE + (np.eye(3), (1.0 + gap, 0, 0))])
    return out


SCENES = _scenes()


@pytest.mark.parametrize("double_sided", [False, True], ids=["one_sided", "double_sided"])
@pytest.mark.parametrize("name", list(SCENES))
def test_no_accepted_ray_outside_its_word(spt, name, double_sided):
    sc = SCENES[name]
    words, info = sc.table(spt)
    rng = np.random.default_rng(11)
    n_rays = 3000 if len(sc.pos) <= 12 else 1200
    eye_dist = min(info["reach"] - info["radius"], 8.0 * info["radius"])   # eyes within the table's reach of the centre
    assert eye_dist > 0.05
    bad, accepted = misses(sc, words, rng, n_rays, eye_dist, double_sided)
    pc = popcounts(words)
    print("%s: reach %.3g delta %.3g (scene %.3g) tight %d; mean bits loose %.2f tight %.2f; %d accepted, %d misses"
          % (name, info["reach"], info["delta"], info["delta_scene"], info["tight"], pc[:, :2].mean(), pc[:, 2:].mean(), accepted, bad))
    assert accepted > 0
    assert bad == 0


def test_cube_tightness(spt):
    """On the cube every tight word is empty, every loose word keeps exactly self, sibling and the 8 triangles of the four adjacent faces."""
    words, info = SCENES["unit_cube"].table(spt)
    pc = popcounts(words)
    print("cube: loose bits", pc[:, :2].tolist(), "tight bits", pc[:, 2:].tolist(), "reach %.3g" % info["reach"])
    assert info["tight"]
    assert info["reach"] > 7.0 + 1e-3, "the table serves the benchmark's camera (7 from the centre)"
    # up - every ray of a camera outside the body: nothing tight; loose keeps self, sibling and the adjacent faces, not the opposite face
    assert (pc[:, 2] == 0).all()
    assert (pc[:, 0] == 10).all()
    # down - a ray that enters the body (a camera inside it, test_gpu_origin_candidates.py: eye_inside) does hit its other faces:
    # tight keeps all but self and sibling, loose everything
    assert (pc[:, 3] == 10).all()
    assert (pc[:, 1] == 12).all()
    for t in range(12):
        assert (int(words[t, 0]) >> t) & 1 and (int(words[t, 0]) >> (t ^ 1)) & 1


def test_smooth_mesh_keeps_everything(spt):
    words, _ = SCENES["smooth"].table(spt)
    assert (words == np.uint64((1 << 20) - 1)).all()


def test_far_from_the_origin_tight_falls_back(spt):
    words, info = SCENES["near_100"].table(spt)
    assert not info["tight"] and info["delta_scene"] >= 0.25 * float(T_MIN_EPS)
    assert (words[:, 2] == words[:, 0]).all() and (words[:, 3] == words[:, 1]).all()


def test_gaps_on_either_side_of_the_tight_threshold(spt):
    """Two cubes whose facing sides are a gap apart: a face's tight word keeps the other cube's facing triangles at every gap the
    table cannot rule out (an accepted hit is at least kTMinEps (1 - eps_z) - delta above the plane)."""
    for gap in (5e-5, 1e-4, 2e-4):
        sc = SCENES["gap_%g" % gap]
        words, info = sc.table(spt)
        h = float(T_MIN_EPS) * (1.0 - 1.0 / 64.0) - info["delta"]
        world = sc.world()
        facing = [k for k in range(12) if np.allclose(world[k][:, 0], 0.0)]           # the first cube's side x = 0
        others = [k for k in range(12, 24) if (np.abs(world[k][:, 0] - gap) < 1e-6).all()]   # the second cube's side x = gap (as f32 places it)
        assert len(facing) == 2 and len(others) == 2
        for t in facing:
            for u in others:
                kept = (int(words[t, 2]) >> u) & 1
                print("gap %g: tight word of %d keeps %d: %d (h = %.3g)" % (gap, t, u, kept, h))
                assert kept == (0 if world[u][:, 0].max() < h else 1)
