"""The expected value of an albedo film (SPT_RENDER_AOV_ALBEDO) from the CPU oracle as it stands: the EMISSIVE STAND-IN.

The oracle knows no albedo flag.  It is handed a descriptor derived from the scene's, in which every surface EMITS its albedo and
nothing else can add light: no lights, no environment, every material a constant specular conductor (a delta lobe: no light
sample), max_depth 1.  trace_ray then returns 0 + (1 * le) * 1 = le for a hit and +0 for a miss, and le is
    emissive                       for a constant material (the albedo rule of spt_abi.h applied to the record), or
    emissive * tex_color(map)      for a recipe whose c0 is a texture: (1, 1, 1) * tex[0], or ((1 - metallic) * tex[0]) for
                                   PBR_METALLIC with a scalar metallic - the device computes base * (1 - metallic), the same
                                   product the other way round,
evaluated with the same tex_input as material_at.  The equality holds under three preconditions, asserted of every scene:
    every constant albedo is +0 in all channels or has luminance > 0 (the oracle adds le only when luminance(le) > 0);
    every albedo texture is, per texel, +0 in all channels or of luminance > 0 too.  ADD, MUL, SRGB and MODIFIER nodes over images
        and non-negative scalars cannot leave that set; a SUB or DIV node can (a negative channel, 0 / 0), so a graph is admitted
        only when interval bounds over it (images lie in [0, 1]) keep every divisor > 0 and either every channel >= 0 or the
        luminance > 0.  t_textured.json has both kinds: checker_half = checker / 0.5 in [0, 2], and one_minus_noise =
        sRGB(0.8 - noise * (0.9, 0.7, 0.5)), whose red channel can be negative while its luminance stays above 0.01;
    every PBR_METALLIC recipe has a scalar metallic (one emissive triple per surface has to hold 1 - metallic).
"""
import ctypes as C

import numpy as np

import _util

f32 = np.float32
spt = _util.load_pkg()

BXDF_LAMBERT, BXDF_SPECULAR_CONDUCTOR = 0, 2
PLASTIC_LOBES = (6, 7, 9)          # MICROFACET_PLASTIC, SPECULAR_PLASTIC, PNDF_PLASTIC
CONDUCTORS = (1, 2, 8)             # MICROFACET_CONDUCTOR, SPECULAR_CONDUCTOR, PNDF_CONDUCTOR
FRESNEL_SCHLICK = 1
TEX_SCALAR, TEX_IMAGE, TEX_SUB, TEX_DIV, TEX_SRGB, TEX_MODIFIER = 0, 1, 3, 5, 6, 7
MAT_LAMBERT, MAT_CONDUCTOR, MAT_DIELECTRIC, MAT_PLASTIC, MAT_PBR_METALLIC, MAT_PBR_SPECULAR, MAT_SUBSURFACE, MAT_PNDF_CONDUCTOR, MAT_PNDF_PLASTIC = range(9)
C0_IS_TEX0 = (MAT_LAMBERT, MAT_PLASTIC, MAT_SUBSURFACE, MAT_PBR_SPECULAR, MAT_PNDF_CONDUCTOR, MAT_PNDF_PLASTIC)


def constant_albedo(mt):
    """The albedo rule of spt_abi.h on one material record (a numpy record of spt.Material)."""
    b = int(mt["bxdf"])
    if b == BXDF_LAMBERT or b in PLASTIC_LOBES or (b in CONDUCTORS and int(mt["fresnel"]) == FRESNEL_SCHLICK):
        return np.array(mt["c0"], dtype=f32)
    return np.ones(3, dtype=f32)


def _nodes_below(textures, root):
    """The texture nodes `root` evaluates: itself and its children, as far as each node type reads them."""
    seen, todo = set(), [int(root)]
    while todo:
        k = todo.pop()
        if k in seen:
            continue
        seen.add(k)
        t = int(textures[k]["type"])
        if t in (TEX_SRGB, TEX_MODIFIER):
            todo.append(int(textures[k]["a"]))
        elif t not in (TEX_SCALAR, TEX_IMAGE):       # the four binary operations
            todo += [int(textures[k]["a"]), int(textures[k]["b"])]
    return seen


def channel_bounds(textures, node):
    """(lo, hi), three float64 each: bounds of the RGB value texture `node` can take.  IEEE operations are monotone, so the
    bounds of the operands bound the rounded result of the operation.  Raises AssertionError on a divisor that may be 0."""
    t = textures[int(node)]
    kind = int(t["type"])
    if kind == TEX_SCALAR:
        v = np.array(t["value"], dtype=np.float64)
        return v, v
    if kind == TEX_IMAGE:
        return np.zeros(3), np.ones(3)
    lo, hi = channel_bounds(textures, t["a"])
    if kind == TEX_MODIFIER:
        return lo, hi
    if kind == TEX_SRGB:                                   # srgb_to_linear (srgb_tex.rs:53-59) is increasing
        to_linear = lambda x: np.where(x <= 0.04045, x / 12.92, ((np.maximum(x, 0.04045) + 0.055) / 1.055) ** 2.4)
        return to_linear(lo), to_linear(hi)
    lo_b, hi_b = channel_bounds(textures, t["b"])
    if kind == TEX_SUB:
        return lo - hi_b, hi - lo_b
    if kind == TEX_DIV:
        assert (lo_b > 0).all(), "a DIV node whose divisor may be 0 or negative"
    ends = [f(x, y) for f in ([np.divide] if kind == TEX_DIV else [np.add] if kind == 2 else [np.multiply]) for x in (lo, hi) for y in (lo_b, hi_b)]
    return np.min(ends, axis=0), np.max(ends, axis=0)


class StandIn:
    """What _util.oracle_render_samples takes for a scene: `desc` and `get_camera`.  Keeps the arrays the descriptor points to."""

    def __init__(self, scene):
        self._scene = scene
        d = scene.desc
        textures, recipes = scene.array("textures"), scene.array("material_recipes")
        materials, surfaces, instances = scene.array("materials"), scene.array("surfaces"), scene.array("instances")
        for s in surfaces:
            mt = materials[int(s["material"])]
            s["emissive_map"] = 0
            if int(mt["recipe"]) == 0:
                a = constant_albedo(mt)
                lum = (f32(0.299) * a[0] + f32(0.587) * a[1]) + f32(0.114) * a[2]
                assert (a.view(np.uint32) == 0).all() or lum > 0, "a constant albedo must be +0 or have luminance > 0: %r" % (a,)
                s["emissive"] = a
                continue
            r = recipes[int(mt["recipe"]) - 1]
            kind, tex0 = int(r["type"]), int(r["tex"][0])
            if kind in (MAT_CONDUCTOR, MAT_DIELECTRIC):      # ConductorFresnel / dielectric lobes: white
                s["emissive"] = np.ones(3, dtype=f32)
                continue
            assert kind in C0_IS_TEX0 or kind == MAT_PBR_METALLIC, kind
            lo, _ = channel_bounds(textures, tex0)
            assert (lo >= 0).all() or 0.299 * lo[0] + 0.587 * lo[1] + 0.114 * lo[2] > 1e-4, \
                "an albedo texture may have a texel that is neither +0 nor of luminance > 0: lower bounds %r" % (lo,)
            s["emissive_map"] = tex0 + 1
            if kind == MAT_PBR_METALLIC:
                m_nodes = _nodes_below(textures, int(r["tex"][1]))
                assert not any(int(textures[k]["type"]) == TEX_IMAGE for k in m_nodes), "PBR_METALLIC needs a scalar metallic here"
                metallic = f32(_util.oracle_tex_eval(scene, int(r["tex"][1]), [[0.25, 0.75]])[0, int(r["metal_chan"])])
                assert 0 <= metallic <= 1, metallic
                s["emissive"] = np.full(3, f32(1) - metallic, dtype=f32)
            else:
                s["emissive"] = np.ones(3, dtype=f32)
        materials["bxdf"] = BXDF_SPECULAR_CONDUCTOR
        materials["recipe"] = 0
        materials["c0"] = 1.0
        materials["c1"] = 1.0
        materials["fresnel"] = FRESNEL_SCHLICK
        instances["light"] = -1
        self._keep = (materials, surfaces, instances)
        nd = spt.SceneDesc()
        C.memmove(C.byref(nd), C.byref(d), C.sizeof(spt.SceneDesc))
        nd.materials = materials.ctypes.data_as(C.POINTER(spt.Material))
        nd.surfaces = surfaces.ctypes.data_as(C.POINTER(spt.Surface))
        nd.instances = instances.ctypes.data_as(C.POINTER(spt.Instance))
        nd.n_lights = 0
        nd.env_light_index = -1
        nd.env.width = nd.env.height = 0
        self.desc = nd

    def get_camera(self, name=None):
        return self._scene.get_camera(name)


def albedo_sums(scene, renderer, width, height, first_sample, n_samples, camera=None, flags=0, **layout):
    """S and Q of an albedo film of the plan `renderer` after its samples [first_sample, first_sample + n_samples), added one
    at a time in sample order; (rows, width, 3) f32 each."""
    plan = spt.PathTracer(max_depth=1, sampler=renderer.sampler, spp=renderer.spp, division_x=renderer.division_x,
                          division_y=renderer.division_y, filter_radius=renderer.filter_radius, seed=renderer.seed)
    x = _util.oracle_render_samples(StandIn(scene), plan, width, height, first_sample, n_samples, camera=camera, flags=flags, **layout)
    s, q = np.zeros_like(x[0]), np.zeros_like(x[0])
    for k in range(n_samples):
        s, q = _util.film_add_sample(s, q, x[k])
    return s, q


def albedo_film(scene, renderer, width, height, n_samples, camera=None, flags=0):
    """MEAN and VAR_OF_MEAN of an albedo film that holds the plan's first n samples."""
    s, q = albedo_sums(scene, renderer, width, height, 0, n_samples, camera=camera, flags=flags)
    return _util.film_mean_and_variance(s, q, n_samples)
