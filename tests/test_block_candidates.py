"""The conservative block-versus-triangle test of include/spt_block_cand.h, through spt_host_block_candidates, against brute force.

A block is the 16 x 4 pixels one wave of the primary kernel owns.  Its candidate mask may drop a triangle only when no sample ray
of the block's pixels can pass the kernel's triangle test.  Here the rays are formed in float32 one operation at a time exactly as
k_primary forms them (numpy does not contract), the test of tri_test_eye / tri_test_edges is restated the same way, and every
(block, pixel, sample, triangle) that the restated test accepts with t > t_min must have its bit set.  No GPU.
"""
import os

import numpy as np
import pytest

import _util

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_MIN = f32(0.0001)

CUBE_V = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64)
CUBE_F = [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7), (1, 7, 3)]


@pytest.fixture(scope="module")
def spt():
    _util.ensure_cpu_build()
    return _util.load_pkg()


def cube_tris():
    return np.array([[CUBE_V[a], CUBE_V[b], CUBE_V[c]] for a, b, c in CUBE_F], dtype=np.float32).reshape(-1, 9)


def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def transform(rng, scale, translate):
    """fwd = T R S as 3 columns + translation (spt_instance), inv = its inverse, both float32."""
    m = rotation(rng) @ np.diag(scale)
    fwd = np.concatenate([m.T.reshape(9), np.asarray(translate, dtype=np.float64)]).astype(f32)
    mi = np.linalg.inv(m)
    inv = np.concatenate([mi.T.reshape(9), -mi @ np.asarray(translate, dtype=np.float64)]).astype(f32)
    return fwd, inv


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def r2_offsets(pixel, spp, n):
    """spt_r2_offset for samples 0 .. n - 1 of `pixel` (an array): (..., n) float32 each."""
    k = (pixel[..., None].astype(np.uint64) * spp + np.arange(n, dtype=np.uint64) + 1) & 0xFFFFFFFF
    xi = (0x800000 + k * 0xC13FAA) & 0xFFFFFF
    yi = (0x800000 + k * 0x91E10E) & 0xFFFFFF
    return xi.astype(f32) * f32(5.9604644775390625e-8), yi.astype(f32) * f32(5.9604644775390625e-8)


def brute_force_hits(cam, width, height, image_rows, inv, tris):
    """(rows, width, n_tris) bool: some sample ray of the pixel passes the kernel's triangle test with t > t_min."""
    eye, fwd, up, right = (np.array(list(v), dtype=f32) for v in (cam.eye, cam.forward, cam.up, cam.right))
    hc = f32(cam.half_cot_half_fov)
    aspect, width_inv, height_inv = f32(width) / f32(height), f32(1.0) / f32(width), f32(1.0) / f32(height)
    j = np.asarray(image_rows, dtype=np.int64)[:, None] + np.zeros((1, width), dtype=np.int64)
    i = np.arange(width, dtype=np.int64)[None, :] + np.zeros_like(j)
    ox, oy = r2_offsets(j * width + i, 64, 64)
    corners = np.array([[0, 0], [1, 0], [0, 1], [1, 1]], dtype=f32)
    ox = np.concatenate([ox, np.broadcast_to(corners[:, 0], ox.shape[:2] + (4,))], axis=-1).astype(f32)
    oy = np.concatenate([oy, np.broadcast_to(corners[:, 1], oy.shape[:2] + (4,))], axis=-1).astype(f32)
    x = (((i.astype(f32)[..., None] + ox) * width_inv) - f32(0.5)) * aspect
    y = ((height - j - 1).astype(f32)[..., None] + oy) * height_inv - f32(0.5)
    cam_fwd = fwd * hc
    du = (cam_fwd + right * x[..., None]) + up * y[..., None]
    d = du / np.sqrt(dot3(du, du))[..., None]
    m = inv.astype(f32)
    od = (m[0:3] * d[..., 0:1] + m[3:6] * d[..., 1:2]) + m[6:9] * d[..., 2:3]
    oo = ((m[0:3] * eye[0] + m[3:6] * eye[1]) + m[6:9] * eye[2]) + m[9:12]
    hits = np.zeros(j.shape + (len(tris),), dtype=bool)
    with np.errstate(all="ignore"):
        for t, tri in enumerate(tris.astype(f32)):
            p0, p1, p2 = tri[0:3], tri[3:6], tri[6:9]
            s, e1, e2 = oo - p0, p1 - p0, p2 - p0
            rr = cross3(s, e1)
            c = dot3(e2, rr)
            q = cross3(od, e2)
            det = dot3(e1 + np.zeros_like(q), q)
            inv_det = f32(1.0) / det
            v = dot3(s + np.zeros_like(q), q) * inv_det
            w = dot3(od, rr + np.zeros_like(od)) * inv_det
            u = f32(1.0) - v - w
            tt = c * inv_det
            ok = (det != 0) & (v >= 0) & (w >= 0) & (u >= 0) & (tt > T_MIN)
            hits[..., t] = ok.any(axis=-1)
    return hits


def check_case(spt, cam, width, height, fwd, inv, tris, shard_index=0, shard_count=1, strip_rows=16):
    rows = spt.shard_rows(height, shard_index, shard_count, strip_rows)
    if len(rows) == 0:
        return 0, 0
    hits = brute_force_hits(cam, width, height, rows, inv, tris)
    tiles_x = (width + 15) // 16
    misses, kept, total = [], 0, 0
    for ty in range((len(rows) + 15) // 16):
        for tx in range(tiles_x):
            for wave in range(4):
                r0 = ty * 16 + wave * 4
                block = 4 * (tx + tiles_x * ty) + wave
                mask = spt.block_candidates(cam, width, height, block, inv, fwd, tris, shard_index, shard_count, strip_rows)
                need = hits[r0:r0 + 4, tx * 16:tx * 16 + 16].any(axis=(0, 1)) if r0 < len(rows) else np.zeros(len(tris), dtype=bool)
                for t in range(len(tris)):
                    if need[t] and not (mask >> t) & 1:
                        misses.append((block, t))
                kept += bin(mask).count("1")
                total += len(tris)
    assert not misses, "triangles hit by a sample ray but dropped from the block's mask (block, triangle): %s" % misses[:8]
    return kept, total


IMAGES = [(16, 4), (24, 10), (37, 21), (48, 36), (33, 7)]


def look_at(spt, eye, target, fov):
    fw = np.asarray(target, dtype=np.float64) - np.asarray(eye, dtype=np.float64)
    up = np.array([0.0, 1.0, 0.0]) if abs(fw[1]) < 0.9 * np.linalg.norm(fw) else np.array([1.0, 0.0, 0.0])
    return spt.make_camera(eye, fw, up, fov)


def cases(spt):
    """(name, camera, fwd, inv): seeded random cameras around a rotated, non-uniformly scaled cube, including the eye inside the mesh's
    box, the eye on a face plane and the mesh partly behind the eye."""
    rng = np.random.default_rng(20240611)
    out = []
    for n in range(20):
        scale = rng.uniform(0.4, 2.5, size=3) if n % 2 else np.array([1.0, 1.0, 1.0]) * rng.uniform(0.5, 2.0)
        centre = rng.uniform(-1.0, 1.0, size=3)
        fwd, inv = transform(rng, scale, centre)
        m = fwd[:9].reshape(3, 3).T.astype(np.float64)
        kind = ("outside", "inside", "face_plane", "behind")[n % 4]
        if kind == "outside":
            eye = centre + rotation(rng) @ np.array([0.0, 0.0, rng.uniform(4.0, 9.0)])
            target = centre + rng.uniform(-0.5, 0.5, size=3)
        elif kind == "inside":
            eye = centre + m @ rng.uniform(-0.8, 0.8, size=3)
            target = eye + rng.normal(size=3)
        elif kind == "face_plane":   # on the plane of the face x = +1 of the cube, inside or beside the face
            local = np.array([1.0, rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5)])
            eye = centre + m @ local
            target = centre + m @ (local * np.array([1.0, 0.2, 0.2]) + np.array([rng.uniform(-0.3, 0.3), 0.0, 0.0])) + rng.normal(size=3) * 0.05
        else:   # just outside a face, looking along it: part of the mesh is behind the eye plane
            eye = centre + m @ np.array([rng.uniform(1.05, 1.4), rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5)])
            target = eye + m @ np.array([rng.uniform(-0.4, 0.1), 1.0, rng.uniform(-0.3, 0.3)])
        out.append(("%s_%d" % (kind, n), look_at(spt, eye.astype(f32), target.astype(f32), float(rng.uniform(35.0, 80.0))), fwd, inv))
    return out


def test_masks_keep_every_triangle_a_sample_ray_hits(spt):
    tris = cube_tris()
    kept = total = 0
    for n, (name, cam, fwd, inv) in enumerate(cases(spt)):
        width, height = IMAGES[n % len(IMAGES)]
        k, t = check_case(spt, cam, width, height, fwd, inv, tris)
        kept, total = kept + k, total + t
    print("candidate bits kept: %d of %d" % (kept, total))
    assert kept < total, "the test never drops a triangle: it proves nothing"


@pytest.mark.parametrize("strip_rows", [2, 4])
def test_masks_of_interleaved_shards(spt, strip_rows):
    """shard_count 3: with strip_rows 2 the 4 local rows of a block are two runs of image rows, 4 rows apart."""
    tris = cube_tris()
    for n, (name, cam, fwd, inv) in enumerate(cases(spt)[:8]):
        width, height = [(48, 36), (37, 21), (24, 10), (33, 7)][n % 4]
        for shard in range(3):
            check_case(spt, cam, width, height, fwd, inv, tris, shard, 3, strip_rows)


def test_far_mesh_and_argument_checks(spt):
    """A mesh so far away that whole triangles are smaller than a pixel; a refused call."""
    tris = cube_tris()
    rng = np.random.default_rng(7)
    fwd, inv = transform(rng, np.array([1.0, 0.5, 2.0]), np.array([0.3, -0.2, 0.1]))
    cam = look_at(spt, np.array([0.0, 0.0, 400.0], dtype=f32), np.array([0.3, -0.2, 0.1], dtype=f32), 50.0)
    kept, total = check_case(spt, cam, 48, 36, fwd, inv, tris)
    assert 0 < kept < total // 4
    with pytest.raises(spt.SptError):
        spt.block_candidates(cam, 48, 36, 0, inv, fwd, np.zeros((65, 9), dtype=f32))


def test_cfg2_cube_tightness(spt):
    """scenes_amd/cfg2_cube.json at 1024 x 1024: candidates per non-empty block (printed; profiles/r06_experiments.md has the
    histogram), and blocks that no projected triangle's padded bounding box touches have empty masks."""
    scene = spt.load_scene(os.path.join(ROOT, "scenes_amd", "cfg2_cube.json"))
    try:
        cam = scene.get_camera(None)
        inst = scene.array("instances")
        assert len(inst) == 1
        fwd, inv = np.array(inst[0]["fwd"], dtype=f32), np.array(inst[0]["inv"], dtype=f32)
        tp = scene.array("tri_pos")
        tris = np.concatenate([tp["p0"], tp["p1"], tp["p2"]], axis=1).astype(f32)
        width = height = 1024
        # projected vertices in float64: pixel i covers u in [i, i + 1), image row j covers v in [H - 1 - j, H - j)
        m = fwd[:9].reshape(3, 3).T.astype(np.float64)
        world = tris.reshape(-1, 3).astype(np.float64) @ m.T + fwd[9:].astype(np.float64) - np.array(list(cam.eye), dtype=np.float64)
        z = world @ np.array(list(cam.forward), dtype=np.float64)
        assert (z > 0).all()
        hc = float(cam.half_cot_half_fov)
        u = (hc * (world @ np.array(list(cam.right), dtype=np.float64)) / z / (width / height) + 0.5) * width
        v = height - (hc * (world @ np.array(list(cam.up), dtype=np.float64)) / z + 0.5) * height   # in image rows, downwards
        u, v = u.reshape(-1, 3), v.reshape(-1, 3)
        pad = 8.0   # pixels, half a block: the quarter pixel of the test's own padding plus its tolerance, which reaches ~4 pixels for the faces seen at a shallow angle
        counts = []
        for block in range(4 * (width // 16) * (height // 16)):
            tile, wave = divmod(block, 4)
            tx, ty = tile % (width // 16), tile // (width // 16)
            i0, i1, j0, j1 = tx * 16, tx * 16 + 16, ty * 16 + wave * 4, ty * 16 + wave * 4 + 4
            touched = ((u.min(axis=1) - pad <= i1) & (u.max(axis=1) + pad >= i0) & (v.min(axis=1) - pad <= j1) & (v.max(axis=1) + pad >= j0)).any()
            mask = spt.block_candidates(cam, width, height, block, inv, fwd, tris)
            if not touched:
                assert mask == 0, "block %d lies outside every triangle's padded bounding box and keeps %x" % (block, mask)
            counts.append(bin(mask).count("1"))
        hist = np.bincount(np.array(counts), minlength=13)
        print("blocks: %d, empty: %d, candidates per non-empty block: %s" % (len(counts), hist[0], {k: int(n) for k, n in enumerate(hist) if k and n}))
        assert hist[0] > 0 and hist[1:].sum() > 0
    finally:
        scene.close()
