"""spt_radiance (DeviceScene.radiance) on rays no pinhole camera makes, against the oracle, word for word.

tests/test_gpu_radiance.py holds spt_radiance to the oracle on camera rays only: one origin per camera, unit directions, the camera's
t_min, auxiliary rays that share the ray's origin.  Bake, probe and the camera models start their paths elsewhere - on a surface, at a
free point, on a lens, on an orthographic plane, at a panorama's eye - and their tests compare them with spt_radiance.  Here those
rays (tests/_anywhere_ref.py makes the batches) go through spt_radiance and through oracle_radiance, the same contract on the
oracle's trace_ray (pinned on the CPU by tests/test_oracle_radiance.py), and every word of every ray must agree: the colours by
_util.same_words, hits_out with oracle_trace_closest byte for byte.  max_depth 5, seed 11, the oracle under device_oracle_flags().

Every batch also asserts on the ORACLE's values that it is not vacuous: on t_materials and t_textured at least 25 % of the rays have a
finite non-zero colour, of at least 100 distinct colours; on t_medium (one small emitter, no environment) at least 5 %; on the other
lit scenes 25 % and 50 distinct colours.  cfg2_cube is a convex body in the void under one directional light: it serves hits, misses,
ties and back faces, not colours.

A failure names the first differing ray: its record, both values, and the first max_depth at which the two sides part."""
import os

import numpy as np
import pytest

import _anywhere_ref as ref
import _util

pytestmark = pytest.mark.gpu

spt = _util.load_pkg()
f32 = np.float32
DEPTH, SEED = ref.DEPTH, ref.SEED


def _ds(name):
    return ref.scene(name).device_scene(0)


def _not_vacuous(name, rgb, hits, what):
    frac, distinct = ref.census(rgb)
    hit = hits["instance"] >= 0
    print("%s, %s: %d rays, %.1f %% finite non-zero, %d distinct colours, %.1f %% hit" % (name, what, rgb.shape[0], 100 * frac, distinct, 100 * hit.mean()))
    assert hit.any() and (~hit).any(), "%s, %s: the batch needs hits and misses" % (name, what)
    if name in ("t_materials", "t_textured"):
        assert frac >= 0.25 and distinct >= 100, (name, what, frac, distinct)
    elif name == "t_medium":
        assert frac >= 0.05, (name, what, frac)
    elif name != "cfg2_cube":
        assert frac >= 0.25 and distinct >= 50, (name, what, frac, distinct)


def _first_difference(name, ds, rays, aux, skip, repeats, got, want):
    bad = ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))
    i = int(np.flatnonzero(bad.any(axis=-1))[0])
    one, one_aux = rays[i:i + 1], (aux[i:i + 1] if aux is not None else None)
    parted = None
    for depth in range(1, DEPTH + 1):
        a = ds.radiance(one, aux=one_aux, repeats=repeats, max_depth=depth, seed=SEED, rng_skip=skip)
        b = _util.oracle_radiance(ref.scene(name), one, one_aux, repeats=repeats, max_depth=depth, seed=SEED, rng_skip=skip, flags=_util.device_oracle_flags())
        if not _util.same_words(a, b):
            parted = (depth, a[0].tolist(), b[0].tolist())
            break
    return ("%d of %d rays differ from the oracle; the first is ray %d: o %r t_min %r d %r stream (%d, %d)%s; device %r, oracle %r; alone they part at "
            "max_depth %r" % (int(bad.any(axis=-1).sum()), got.shape[0], i, rays["o"][i].tolist(), float(rays["t_min"][i]), rays["d"][i].tolist(),
                              int(rays["stream_a"][i]), int(rays["stream_b"][i]), "" if aux is None else " aux %r" % (aux[i].tolist(),),
                              got[i].tolist(), want[i].tolist(), parted))


def _compare(name, kind, repeats=1, ds=None, vacuity=True, colours=True):
    rays, aux, skip, want, want_hits = ref.batch(name, kind, repeats)
    if vacuity:
        _not_vacuous(name, want, want_hits, kind)
    ds = _ds(name) if ds is None else ds
    got, hits = ds.radiance(rays, aux=aux, repeats=repeats, max_depth=DEPTH, seed=SEED, rng_skip=skip, hits=True)
    if hits.tobytes() != want_hits.tobytes():
        i = int(np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(hits, want_hits)])[0])
        raise AssertionError("%s, %s: hits_out differs from oracle_trace_closest, first at ray %d: o %r t_min %r d %r; device %r, oracle %r"
                             % (name, kind, i, rays["o"][i].tolist(), float(rays["t_min"][i]), rays["d"][i].tolist(), hits[i], want_hits[i]))
    assert got.shape == want.shape
    if colours and not _util.same_words(got, want):
        raise AssertionError("%s, %s: %s" % (name, kind, _first_difference(name, ds, rays, aux, skip, repeats, got, want)))
    return got, hits


# ---- 1. surface origins -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["", ":t0"], ids=["as_made", "t_min_0"])
@pytest.mark.parametrize("name", ["t_materials", "t_textured", "t_medium"])
def test_surface_origins(name, variant):
    """Gather rays of a bake: origins on the meshes (inside triangles, on edges, at vertices), t_min = 0.0001 / cos as made; and the
    same rays with t_min = 0, where the origin's own triangle and its neighbours are hit at t = 0 and the tie rule decides."""
    _compare(name, "surface" + variant)
    if variant and name == "t_materials":
        # ... which is another question than the one above: some of the oracle's answers change
        a, b = ref.batch(name, "surface"), ref.batch(name, "surface:t0")
        changed = (a[3].view(np.uint32) != b[3].view(np.uint32)).any(axis=-1).mean()
        assert changed >= 0.03 and a[4].tobytes() != b[4].tobytes(), changed


def test_surface_origins_of_a_scene_with_patches():
    """t_bezier is forwarded to the library with the patch primitive: WORLD points on the patches and the sphere, and the floor's
    mesh points."""
    _compare("t_bezier", "world")
    _compare("t_bezier", "surface")


# the walkers of scenes that do not fit LDS: the streaming intake kernel, and the walker over the geometry in memory
@pytest.mark.parametrize("switches", [{"SPT_NO_LDS_GEO": "1"}, {"SPT_NO_LDS_GEO": "1", "SPT_NO_STREAM": "1"}], ids=["stream", "memory"])
@pytest.mark.parametrize("name", ["t_materials", "t_textured"])
def test_surface_origins_under_the_large_scene_walkers(monkeypatch, switches, name):
    for k, v in switches.items():
        monkeypatch.setenv(k, v)      # (read when the device scene is made)
    sc = spt.load_scene(os.path.join(_util.SCENES, name + ".json"))
    try:
        for kind in ("surface", "surface:t0"):
            _compare(name, kind, ds=sc.device_scene(0), vacuity=False)
    finally:
        sc.close()


# ---- 2. free points ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cfg2_cube", "t_materials", "t_medium"])
def test_free_points(name):
    """Gather rays of 24 probes, 32 each.  The first probes stand inside closed bodies (every ray hits, from behind or from inside a
    glass or medium-bounded object); the next is about 10^3 scene radii away in the void (every ray misses: the environment at depth
    0, and coordinates of that size)."""
    rays, aux, skip, want, want_hits = ref.batch(name, "free")
    hit = (want_hits["instance"] >= 0).reshape(24, 32)
    inside = len(ref.INSIDE[name])
    assert hit[:inside].all() and not hit[inside].any()
    assert np.abs(rays["o"].reshape(24, 32, 3)[inside]).max() > 1000
    if name == "cfg2_cube":
        t = want_hits["t"].reshape(24, 32)[0]
        assert (t > 0.9).all() and (t < 1.8).all()      # the cube's faces (half edge 1) from its centre
    if name == "t_materials":
        far = want.reshape(24, 32, 3)[inside]
        assert np.isfinite(far).all() and (far > 0).all() and len(np.unique(far, axis=0)) > 8     # the environment map, seen from afar
    _compare(name, "free")


# ---- 3. camera models -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("aux", [":noaux", ""], ids=["without_aux", "with_aux"])
@pytest.mark.parametrize("kind", ["thin_lens", "orthographic", "panorama"])
@pytest.mark.parametrize("name", ["t_textured", "t_pndf"])
def test_camera_model_rays(name, kind, aux):
    """tests/_camera_ref.py's rays of a thin lens, an orthographic view and a panorama (random sampler: rng_skip 2).  Every ray of a
    lens has an origin of its own (which its auxiliary rays share); on the orthographic plane the auxiliary rays start beside the ray,
    parallel to it.  Without aux the first hit is textured as every later hit is, which the oracle answers too."""
    rays, ax, skip, want, _ = ref.batch(name, kind + aux)
    assert skip == 2
    if not aux:
        if kind == "orthographic":
            assert (ax["rx_o"] != rays["o"]).any(axis=-1).mean() > 0.9 and (ax["ry_o"] != rays["o"]).any(axis=-1).mean() > 0.9
            # ... and those origins matter: from the ray's own origin the oracle's differentials give other colours
            moved = ax.copy()
            moved["rx_o"], moved["ry_o"] = rays["o"], rays["o"]
            other = _util.oracle_radiance(ref.scene(name), rays, moved, max_depth=DEPTH, seed=SEED, rng_skip=skip, flags=_util.device_oracle_flags())
            assert (other.view(np.uint32) != want.view(np.uint32)).any(axis=-1).mean() > 0.1
        # the differentials matter: without them the oracle gives other colours
        assert not _util.same_words(want, ref.batch(name, kind + ":noaux")[3])
    if kind != "panorama":
        assert len(np.unique(rays["o"], axis=0)) > 1000
    _compare(name, kind + aux)


# ---- 4. zero components, edges and vertices ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cfg2_cube", "t_materials"])
def test_zero_components_edges_and_vertices(name):
    """Axis-parallel rays through every mesh vertex with +0.0 and -0.0 in the other two components (on the cube, rotated about y, the
    vertical ones run along its edges), rays along the edges, rays aimed at the vertices: where two triangles answer with the same t
    the (t, instance, prim) rule decides, and a reciprocal of a signed zero decides the slab test."""
    rays = ref.batch(name, "axes")[0]
    zero = rays["d"] == 0
    assert zero.any() and np.signbit(rays["d"][zero]).any() and not np.signbit(rays["d"][zero]).all()
    _compare(name, "axes")


# ---- 5. many rays, repeats --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cfg2_cube", "t_materials"])
def test_16641_rays_with_two_repeats(name):
    """129 probes of 129 rays, repeats = 2: 33 282 paths, so two intake workgroups share a queue shard and a path's record index is
    (ray) * repeats + k with both factors in play."""
    rays, _, _, want, _ = ref.batch(name, "big", 2)
    assert rays.shape[0] == 16641
    got, _ = _compare(name, "big", repeats=2)
    if name == "t_materials":     # the two paths of a ray differ, so the mean is not a single path's colour
        single = _util.oracle_radiance(ref.scene(name), rays[:512], max_depth=DEPTH, seed=SEED, flags=_util.device_oracle_flags())
        assert not _util.same_words(single, want[:512])


# ---- 6. directions that are not unit vectors ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["x3", "x025"])
def test_directions_of_other_lengths(variant):
    """d is taken as it is (include/spt_abi.h): the surface batch of t_materials with every direction scaled by 3 and by 0.25.  Many
    of the oracle's colours are not finite for the longer directions; at least a quarter of them must still be finite and not black,
    so that the comparison is one of colours."""
    name = "t_materials"
    want = ref.batch(name, "surface:" + variant)[3]
    assert ref.live(want).mean() >= 0.25
    assert not _util.same_words(want, ref.batch(name, "surface")[3])      # the length matters to the oracle
    _compare(name, "surface:" + variant)
