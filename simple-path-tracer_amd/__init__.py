"""simple-path-tracer hot path, MI355X-native — Python binding over the C ABIs.

Mirrors the reference's host-side surface for the path
(reference src/main.rs:43-66, src/loader/mod.rs:9-31, src/renderer/mod.rs:9-38):

    scene    = load_scene("scene.json")          # loader::load_scene
    renderer = load_renderer("pt.json")          # loader::load_renderer -> PathTracer
    film     = renderer.render(scene, OutputConfig(width, height, output, camera))

`render` runs the hand-written HIP kernels of libspt_hip.so.  There is no CPU
fallback: if the library or a gfx950 device is missing the call raises.
ctypes + numpy only; PyTorch is imported in one place, when DeviceScene.radiance is handed torch tensors.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from dataclasses import dataclass
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.environ.get("SPT_LIB_DIR") or os.path.join(_HERE, "lib")   # (SPT_LIB_DIR: A/B runs against another build, tools/ only)
REPO_ROOT = os.path.dirname(_HERE)

SPT_ABI_VERSION = 14
SPT_LEAF_FLAG = 0x80000000

STATUS_NAMES = {
    0: "SPT_OK", 1: "SPT_ERR_INVALID_ARG", 2: "SPT_ERR_NO_DEVICE", 3: "SPT_ERR_HIP", 4: "SPT_ERR_UNSUPPORTED",
    5: "SPT_ERR_OUT_OF_MEMORY", 100: "SPT_HOST_ERR_IO", 101: "SPT_HOST_ERR_PARSE", 102: "SPT_HOST_ERR_SCHEMA",
    103: "SPT_HOST_ERR_UNSUPPORTED",
}


class SptError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__("%s: %s" % (STATUS_NAMES.get(status, str(status)), message))
        self.status = status
        self.message = message


# ---- ctypes mirrors of include/spt_abi.h ---------------------------------------------

class BvhNode(C.Structure):
    _fields_ = [("bmin", C.c_float * 3), ("a", C.c_uint32), ("bmax", C.c_float * 3), ("b", C.c_uint32)]


class TriPos(C.Structure):
    _fields_ = [("p0", C.c_float * 3), ("pad0", C.c_float), ("p1", C.c_float * 3), ("pad1", C.c_float),
                ("p2", C.c_float * 3), ("pad2", C.c_float)]


class TriAttr(C.Structure):
    _fields_ = [("n", (C.c_float * 3) * 3), ("t", (C.c_float * 3) * 3), ("b", (C.c_float * 3) * 3),
                ("uv", (C.c_float * 2) * 3), ("pad", C.c_float * 3)]


class Sphere(C.Structure):
    _fields_ = [("center", C.c_float * 3), ("radius", C.c_float)]


class BezierPatch(C.Structure):
    _fields_ = [("cp", ((C.c_float * 4) * 4) * 4)]


class Mesh(C.Structure):
    _fields_ = [("root", C.c_uint32), ("node_count", C.c_uint32), ("tri_first", C.c_uint32), ("tri_count", C.c_uint32)]


class Instance(C.Structure):
    _fields_ = [("inv", C.c_float * 12), ("fwd", C.c_float * 12), ("nrm", C.c_float * 9),
                ("prim_type", C.c_uint32), ("prim_id", C.c_uint32), ("surface", C.c_uint32), ("light", C.c_int32),
                ("bmin", C.c_float * 3), ("bmax", C.c_float * 3), ("pad", C.c_float * 5)]


class Material(C.Structure):
    _fields_ = [("bxdf", C.c_uint32), ("c0", C.c_float * 3), ("c1", C.c_float * 3), ("ax", C.c_float),
                ("ay", C.c_float), ("ior", C.c_float), ("c2", C.c_float * 3), ("fresnel", C.c_uint32),
                ("substrate", C.c_uint32), ("recipe", C.c_uint32)]


class Texture(C.Structure):
    _fields_ = [("type", C.c_uint32), ("a", C.c_uint32), ("b", C.c_uint32), ("image", C.c_uint32),
                ("value", C.c_float * 3), ("mode", C.c_int32), ("wrap", C.c_int32), ("tiling", C.c_float * 3),
                ("offset", C.c_float * 3), ("pad", C.c_uint32)]


class Image(C.Structure):
    _fields_ = [("first_level", C.c_uint32), ("n_levels", C.c_uint32)]


class ImageLevel(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("first_texel", C.c_uint32), ("pad", C.c_uint32)]


class MaterialRecipe(C.Structure):
    _fields_ = [("type", C.c_uint32), ("tex", C.c_uint32 * 4), ("rough_chan", C.c_uint32), ("metal_chan", C.c_uint32),
                ("ior", C.c_float)]


class Surface(C.Structure):
    _fields_ = [("material", C.c_uint32), ("flags", C.c_uint32), ("inside_medium", C.c_int32),
                ("emissive", C.c_float * 3), ("normal_map", C.c_uint32), ("emissive_map", C.c_uint32)]


class Medium(C.Structure):
    _fields_ = [("sigma_t", C.c_float * 3), ("sigma_s", C.c_float * 3), ("g", C.c_float), ("pad", C.c_float)]


class Light(C.Structure):
    _fields_ = [("type", C.c_uint32), ("pos", C.c_float * 3), ("dir", C.c_float * 3), ("strength", C.c_float * 3),
                ("cos_inner", C.c_float), ("cos_outer", C.c_float), ("instance", C.c_uint32), ("power", C.c_float),
                ("pad", C.c_float * 2)]


class AliasTable(C.Structure):
    _fields_ = [("n", C.c_uint32), ("props", C.POINTER(C.c_float)), ("u", C.POINTER(C.c_float)),
                ("k", C.POINTER(C.c_uint32))]


class Env(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("texels", C.POINTER(C.c_float)),
                ("scale", C.c_float * 3), ("alias", AliasTable)]


class PndfTerm(C.Structure):
    _fields_ = [("u", C.c_float * 2), ("s", C.c_float * 2), ("jacobian", C.c_float * 4), ("mat_a", C.c_float * 4),
                ("mat_s", C.c_float * 4), ("mat_mu", C.c_float * 4)]


class PndfNode(C.Structure):
    _fields_ = [("bmin", C.c_float * 4), ("bmax", C.c_float * 4), ("start", C.c_uint32), ("end", C.c_uint32),
                ("lc", C.c_uint32), ("rc", C.c_uint32)]


class Pndf(C.Structure):
    _fields_ = [("first_term", C.c_uint32), ("n_terms", C.c_uint32), ("s_block_count", C.c_uint32), ("first_root", C.c_uint32),
                ("uv_root", C.c_uint32), ("uv_first_ref", C.c_uint32), ("sigma_r", C.c_float), ("sigma_hx", C.c_float),
                ("sigma_hy", C.c_float), ("tiling", C.c_float * 2), ("offset", C.c_float * 2), ("pad", C.c_uint32 * 3)]


class SceneDesc(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32), ("aggregate", C.c_uint32),
        ("n_tlas_nodes", C.c_uint32), ("tlas_nodes", C.POINTER(BvhNode)),
        ("n_instances", C.c_uint32), ("instances", C.POINTER(Instance)),
        ("n_meshes", C.c_uint32), ("meshes", C.POINTER(Mesh)),
        ("n_blas_nodes", C.c_uint32), ("blas_nodes", C.POINTER(BvhNode)),
        ("n_tris", C.c_uint32), ("tri_pos", C.POINTER(TriPos)), ("tri_attr", C.POINTER(TriAttr)),
        ("n_spheres", C.c_uint32), ("spheres", C.POINTER(Sphere)),
        ("n_surfaces", C.c_uint32), ("surfaces", C.POINTER(Surface)),
        ("n_materials", C.c_uint32), ("materials", C.POINTER(Material)),
        ("n_mediums", C.c_uint32), ("mediums", C.POINTER(Medium)),
        ("n_lights", C.c_uint32), ("lights", C.POINTER(Light)),
        ("light_sampler", C.c_uint32), ("env_light_index", C.c_int32),
        ("light_alias", AliasTable), ("env", Env),
        ("n_textures", C.c_uint32), ("textures", C.POINTER(Texture)),
        ("n_images", C.c_uint32), ("images", C.POINTER(Image)),
        ("n_image_levels", C.c_uint32), ("image_levels", C.POINTER(ImageLevel)),
        ("n_texels", C.c_uint32), ("texels", C.POINTER(C.c_uint32)),
        ("n_material_recipes", C.c_uint32), ("material_recipes", C.POINTER(MaterialRecipe)),
        ("n_bezier_patches", C.c_uint32), ("bezier_patches", C.POINTER(BezierPatch)),
        ("n_pndfs", C.c_uint32), ("pndfs", C.POINTER(Pndf)),
        ("n_pndf_terms", C.c_uint32), ("pndf_terms", C.POINTER(PndfTerm)),
        ("n_pndf_nodes", C.c_uint32), ("pndf_nodes", C.POINTER(PndfNode)),
        ("n_pndf_refs", C.c_uint32), ("pndf_refs", C.POINTER(C.c_uint32)),
        ("n_pndf_roots", C.c_uint32), ("pndf_roots", C.POINTER(C.c_uint32)),
    ]


class Camera(C.Structure):
    _fields_ = [("eye", C.c_float * 3), ("forward", C.c_float * 3), ("up", C.c_float * 3), ("right", C.c_float * 3),
                ("half_cot_half_fov", C.c_float)]


SAMPLER_RANDOM, SAMPLER_JITTERED, SAMPLER_RECURRENCE = 0, 1, 2
CAMERA_PERSPECTIVE, CAMERA_THIN_LENS, CAMERA_ORTHOGRAPHIC, CAMERA_PANORAMA = 0, 1, 2, 3   # SPT_CAMERA_*
CAMERA_SEED_SALT = 0x4C454E5343414D31   # SPT_CAMERA_SEED_SALT: the lens draws' stream is (seed ^ salt, pixel, plan index)


class CameraModel(C.Structure):
    """spt_camera_model (include/spt_abi.h, "camera models"): what PathTracer.render / render_shard / progressive take as
    camera_model=.  `base` is a pinhole Camera (Scene.get_camera); fields that do not belong to a type are ignored."""
    _fields_ = [("size", C.c_uint32), ("type", C.c_uint32), ("base", Camera), ("lens_radius", C.c_float), ("focus_distance", C.c_float),
                ("view_height", C.c_float), ("pad", C.c_uint32)]

    @classmethod
    def _make(cls, kind: int, cam: "Camera", **fields) -> "CameraModel":
        m = cls()
        m.size = C.sizeof(cls)
        m.type = kind
        C.memmove(C.byref(m.base), C.byref(cam), C.sizeof(Camera))
        for k, v in fields.items():
            setattr(m, k, v)
        return m

    @classmethod
    def perspective(cls, cam: "Camera") -> "CameraModel":
        return cls._make(CAMERA_PERSPECTIVE, cam)

    @classmethod
    def thin_lens(cls, cam: "Camera", lens_radius: float, focus_distance: float) -> "CameraModel":
        """A pinhole behind a thin lens of `lens_radius`, sharp at `focus_distance` along cam.forward from the eye."""
        return cls._make(CAMERA_THIN_LENS, cam, lens_radius=lens_radius, focus_distance=focus_distance)

    @classmethod
    def orthographic(cls, cam: "Camera", view_height: float) -> "CameraModel":
        """Parallel rays along cam.forward; the image is `view_height` world units high."""
        return cls._make(CAMERA_ORTHOGRAPHIC, cam, view_height=view_height)

    @classmethod
    def panorama(cls, eye) -> "CameraModel":
        """Equirectangular probe at `eye` in the environment map's axes: row 0 at the +y pole, the image centre looks along +z."""
        cam = Camera()
        cam.eye[:] = [float(v) for v in eye]
        cam.forward[:] = [0.0, 0.0, 1.0]
        cam.up[:] = [0.0, 1.0, 0.0]
        cam.right[:] = [1.0, 0.0, 0.0]
        cam.half_cot_half_fov = 1.0
        return cls._make(CAMERA_PANORAMA, cam)


RENDER_PROFILE = 1
RENDER_BOX_RADIUS = 2
RENDER_COUNT_VISITS = 4
RENDER_ASYNC = 8
RENDER_DEBUG_NORMAL = 16   # the reference's cargo feature `debug_normal` (Cargo.toml:34-36, pt.rs:113-118)
RENDER_AOV_ALBEDO = 32     # a path's colour is the albedo of the first surface it reaches (spt_abi.h); see render_flags_supported()
DENOISE_DEMODULATE, DENOISE_OUT_RGB8 = 1, 2   # spt_denoise_job.flags
READ_SOURCES = {"mean": 0, "mon": 1, "gmon": 2, "denoised": 3}   # SPT_READ_* of spt_film_read_rgb8
FILM_MOMENTS = 1          # spt_film_create: also keep the per-channel sum of squared sample radiance (ABI v14)
FILM_KEEP_SAMPLES = 2     # spt_film_create: keep every sample's radiance (any box radius; spt_film_read_samples)
FILM_MEAN, FILM_SUM, FILM_SUM_SQ, FILM_VAR_OF_MEAN = 0, 1, 2, 3   # spt_film_read
FILTER_TYPES = {"box": 0, "tent": 1, "gaussian": 2, "mitchell": 3}   # SPT_FILTER_* of spt_film_filter
ROBUST_MON, ROBUST_GMON = 0, 1   # spt_film_read_robust: median of the bucket means, Gini-adaptive trimmed mean of them
N_KERNELS = 7
KERNEL_NAMES = ("primary", "shade", "shadow", "extend", "resolve", "other", "shade_first")


class RenderParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("spp", C.c_uint32), ("max_depth", C.c_uint32),
                ("sampler", C.c_uint32), ("division_x", C.c_uint32), ("division_y", C.c_uint32),
                ("seed", C.c_uint64), ("shard_index", C.c_uint32), ("shard_count", C.c_uint32),
                ("strip_rows", C.c_uint32), ("samples_per_pass", C.c_uint32), ("flags", C.c_uint32),
                ("out_strip_stride", C.c_uint64), ("filter_radius", C.c_float), ("stats_size", C.c_uint32)]


class FilterDesc(C.Structure):
    """spt_filter_desc (spt_film_filter): p0 is the Gaussian's alpha or Mitchell's B, p1 Mitchell's C."""
    _fields_ = [("size", C.c_uint32), ("type", C.c_uint32), ("radius", C.c_float), ("p0", C.c_float), ("p1", C.c_float), ("pad", C.c_uint32)]


def filter_desc(kind: str, radius: Optional[float] = None, alpha: float = 2.0, b: float = 1.0 / 3.0, c: float = 1.0 / 3.0) -> FilterDesc:
    """The FilterDesc of a filter by name ("box", "tent", "gaussian", "mitchell") with the renderer file's defaults: alpha 2,
    b = c = 1/3, Mitchell's radius 2."""
    if kind not in FILTER_TYPES:
        raise ValueError("filter: kind is one of %s, not %r" % (", ".join(repr(k) for k in FILTER_TYPES), kind))
    if radius is None:
        if kind in ("tent", "gaussian"):
            raise ValueError("filter: %r needs a radius" % (kind,))
        radius = 2.0 if kind == "mitchell" else 0.0   # (the box ignores it)
    p0, p1 = (alpha, 0.0) if kind == "gaussian" else (b, c) if kind == "mitchell" else (0.0, 0.0)
    return FilterDesc(C.sizeof(FilterDesc), FILTER_TYPES[kind], radius, p0, p1, 0)


class RenderStats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("segments_closest", C.c_uint64), ("segments_shadow", C.c_uint64),
                ("gpu_ms", C.c_double), ("kernel_ms", C.c_double * N_KERNELS),
                ("kernel_launches", C.c_uint32 * N_KERNELS), ("primary_hits", C.c_uint64),
                ("path_vertices", C.c_uint64), ("shadow_first", C.c_uint64), ("vertices_second", C.c_uint64), ("live_samples", C.c_uint64),
                ("node_visits", C.c_uint64), ("tri_tests", C.c_uint64), ("instance_visits", C.c_uint64), ("node_bytes", C.c_uint64),
                ("class_visits", (C.c_uint64 * 3) * 3)]


class DenoiseParams(C.Structure):
    """spt_denoise_params (spt_film_denoise); `size` is sizeof of the struct."""
    _fields_ = [("size", C.c_uint32), ("iterations", C.c_uint32), ("k_color", C.c_float), ("k_guide", C.c_float),
                ("eps_color", C.c_float), ("eps_guide", C.c_float)]


class DenoiseJob(C.Structure):
    """spt_denoise_job (spt_film_denoise_job); `size` is sizeof of the struct."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("guide", C.c_void_p), ("albedo", C.c_void_p),
                ("params", C.POINTER(DenoiseParams)), ("k_albedo", C.c_float), ("eps_albedo", C.c_float), ("eps_demod", C.c_float),
                ("pad", C.c_uint32)]


class ImageDenoiseJob(C.Structure):
    """spt_image_denoise_job (spt_denoise_image); `size` is sizeof of the struct."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("width", C.c_uint32), ("rows", C.c_uint32),
                ("mean", C.c_void_p), ("var", C.c_void_p), ("guide_mean", C.c_void_p), ("guide_var", C.c_void_p),
                ("albedo_mean", C.c_void_p), ("albedo_var", C.c_void_p), ("params", C.POINTER(DenoiseParams)),
                ("k_albedo", C.c_float), ("eps_albedo", C.c_float), ("eps_demod", C.c_float), ("pad", C.c_uint32)]


class MultiFilmDenoiseJob(C.Structure):
    """spt_host_multi_film_denoise_job (spt_host_multi_film_denoise): spt_denoise_job with multi films."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("guide", C.c_void_p), ("albedo", C.c_void_p),
                ("params", C.POINTER(DenoiseParams)), ("k_albedo", C.c_float), ("eps_albedo", C.c_float), ("eps_demod", C.c_float),
                ("pad", C.c_uint32)]


HIT_DTYPE = np.dtype([("t", "<f4"), ("instance", "<i4"), ("prim", "<i4"), ("v", "<f4"), ("w", "<f4")])
RAY_DTYPE = np.dtype([("o", "<f4", 3), ("t_min", "<f4"), ("d", "<f4", 3), ("t_max", "<f4")])
# spt_radiance: spt_path_ray (48 B) and spt_ray_aux (64 B)
PATH_RAY_DTYPE = np.dtype([("o", "<f4", 3), ("t_min", "<f4"), ("d", "<f4", 3), ("stream_a", "<u4"), ("stream_b", "<u4"), ("pad", "<u4", 3)])
RAY_AUX_DTYPE = np.dtype([("rx_o", "<f4", 3), ("pad0", "<f4"), ("rx_d", "<f4", 3), ("pad1", "<f4"), ("ry_o", "<f4", 3), ("pad2", "<f4"),
                          ("ry_d", "<f4", 3), ("pad3", "<f4")])
RADIANCE_DEVICE_POINTERS = 1
CAMERA_T_MIN = 1e-4   # Ray::T_MIN_EPS, the t_min of a camera ray (kTMinEps)


class RadianceJob(C.Structure):
    """spt_radiance_job (spt_radiance); `size` is sizeof of the struct."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("n_rays", C.c_uint64), ("rays", C.c_void_p), ("aux", C.c_void_p),
                ("repeats", C.c_uint32), ("max_depth", C.c_uint32), ("seed", C.c_uint64), ("rng_skip", C.c_uint32),
                ("rays_per_pass", C.c_uint32), ("rgb_out", C.c_void_p), ("hits_out", C.c_void_p)]


# spt_gbuffer: spt_gbuffer_rec (64 B) and the bits of its `flags` (bits 8..15: the instance's prim_type)
GBUFFER_DTYPE = np.dtype([("p", "<f4", 3), ("t", "<f4"), ("n", "<f4", 3), ("instance", "<i4"), ("albedo", "<f4", 3), ("prim", "<i4"),
                          ("v", "<f4"), ("w", "<f4"), ("surface", "<u4"), ("flags", "<u4")])
GBUFFER_DEVICE_POINTERS = 1
GBUF_BACKFACING, GBUF_LIGHT = 1, 2


class GBufferJob(C.Structure):
    """spt_gbuffer_job (spt_gbuffer); `size` is sizeof of the struct."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("n_rays", C.c_uint64), ("rays", C.c_void_p), ("aux", C.c_void_p),
                ("rays_per_pass", C.c_uint32), ("pad", C.c_uint32), ("out", C.c_void_p)]


CAMERA_RAYS_DEVICE_POINTERS = 1
CAMERA_GBUFFER_DEVICE_POINTERS = 1


class CameraRaysJob(C.Structure):
    """spt_camera_rays_job (spt_camera_rays); `size` is sizeof of the struct."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("model", C.c_void_p), ("plan", C.c_void_p), ("first", C.c_uint32),
                ("count", C.c_uint32), ("rays", C.c_void_p), ("aux", C.c_void_p), ("rays_per_pass", C.c_uint32), ("pad", C.c_uint32)]


class CameraGBufferJob(C.Structure):
    """spt_camera_gbuffer_job (spt_camera_gbuffer); `size` is sizeof of the struct."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("model", C.c_void_p), ("plan", C.c_void_p), ("first", C.c_uint32),
                ("count", C.c_uint32), ("albedo", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p), ("coverage", C.c_void_p),
                ("rays_per_pass", C.c_uint32), ("pad", C.c_uint32)]


# spt_bake: spt_bake_point (16 B: spt_hit without t) and spt_bake_world_point (32 B)
BAKE_POINT_DTYPE = np.dtype([("instance", "<u4"), ("prim", "<u4"), ("v", "<f4"), ("w", "<f4")])
BAKE_WORLD_DTYPE = np.dtype([("p", "<f4", 3), ("pad0", "<f4"), ("n", "<f4", 3), ("pad1", "<f4")])
BAKE_POINTS_SURFACE, BAKE_POINTS_WORLD = 0, 1
BAKE_DEVICE_POINTERS, BAKE_FLIP = 1, 2


class BakeJob(C.Structure):
    """spt_bake_job (spt_bake); `size` is sizeof of the struct."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("kind", C.c_uint32), ("pad", C.c_uint32), ("n_points", C.c_uint64),
                ("points", C.c_void_p), ("rgb_out", C.c_void_p), ("samples", C.c_uint32), ("max_depth", C.c_uint32), ("seed", C.c_uint64),
                ("first_point", C.c_uint32), ("first_sample", C.c_uint32), ("points_per_pass", C.c_uint32), ("pad1", C.c_uint32)]


# spt_occluded / spt_ao: visibility along caller rays (spt_ray records) and at bake points; spt_ao_rec (32 B)
OCCLUDED_DEVICE_POINTERS, OCCLUDED_PACKED = 1, 2
AO_DEVICE_POINTERS, AO_FLIP = 1, 2
AO_DTYPE = np.dtype([("sum", "<f4", 3), ("open", "<f4"), ("bent", "<f4", 3), ("count", "<u4")])


class OccludedJob(C.Structure):
    """spt_occluded_job (spt_occluded); `size` is sizeof of the struct."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("n_rays", C.c_uint64), ("rays", C.c_void_p), ("out", C.c_void_p),
                ("rays_per_pass", C.c_uint32), ("pad", C.c_uint32)]


class AoJob(C.Structure):
    """spt_ao_job (spt_ao); `size` is sizeof of the struct."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("kind", C.c_uint32), ("pad", C.c_uint32), ("n_points", C.c_uint64),
                ("points", C.c_void_p), ("out", C.c_void_p), ("samples", C.c_uint32), ("max_distance", C.c_float), ("seed", C.c_uint64),
                ("first_point", C.c_uint32), ("first_sample", C.c_uint32), ("points_per_pass", C.c_uint32), ("pad1", C.c_uint32)]


# spt_hits: the K nearest crossings of caller segments and the crossing counts; spt_hit_rec (32 B), spt_hit_count (8 B)
HITS_DEVICE_POINTERS, HITS_COUNT_ALL = 1, 2
HIT_BACKFACING = 1
HIT_REC_DTYPE = np.dtype([("t", "<f4"), ("instance", "<i4"), ("prim", "<i4"), ("flags", "<u4"), ("v", "<f4"), ("w", "<f4"), ("pad", "<u4", 2)])
HIT_COUNT_DTYPE = np.dtype([("total", "<u4"), ("back", "<u4")])


class HitsJob(C.Structure):
    """spt_hits_job (spt_hits); `size` is sizeof of the struct."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("n_rays", C.c_uint64), ("rays", C.c_void_p), ("hits", C.c_void_p),
                ("counts", C.c_void_p), ("max_hits", C.c_uint32), ("rays_per_pass", C.c_uint32)]


def pack_occluded(occ) -> np.ndarray:
    """The words spt_occluded writes with SPT_OCCLUDED_PACKED for the bytes `occ`: ray i is bit i & 63 of word i >> 6, the bits past
    the last ray are 0."""
    occ = np.asarray(occ).reshape(-1) != 0
    padded = np.zeros((occ.shape[0] + 63) // 64 * 64, dtype=np.uint8)
    padded[:occ.shape[0]] = occ
    return np.packbits(padded.reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1)


def unpack_occluded(words, n: int) -> np.ndarray:
    """The n bytes (1 occluded, 0 not) behind the packed words of spt_occluded."""
    words = np.ascontiguousarray(words).reshape(-1).view("<u8")
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].copy()


# spt_probe: spt_probe_point (16 B)
PROBE_DTYPE = np.dtype([("p", "<f4", 3), ("pad", "<f4")])
PROBE_DEVICE_POINTERS = 1


class ProbeJob(C.Structure):
    """spt_probe_job (spt_probe); `size` is sizeof of the struct."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("n_points", C.c_uint64), ("points", C.c_void_p), ("sh_out", C.c_void_p),
                ("aux_out", C.c_void_p), ("samples", C.c_uint32), ("max_depth", C.c_uint32), ("seed", C.c_uint64), ("first_point", C.c_uint32),
                ("first_sample", C.c_uint32), ("points_per_pass", C.c_uint32), ("pad", C.c_uint32)]


# ---- library loading -----------------------------------------------------------------

class SceneUpdateDesc(C.Structure):
    """spt_scene_update_desc (spt_scene_update); `size` is sizeof of the struct."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32),
                ("n_tlas_nodes", C.c_uint32), ("tlas_nodes", C.POINTER(BvhNode)),
                ("n_instances", C.c_uint32), ("instances", C.POINTER(Instance)),
                ("n_lights", C.c_uint32), ("lights", C.POINTER(Light)),
                ("light_alias", AliasTable)]


class MeshDeform(C.Structure):
    """spt_mesh_deform (spt_scene_deform): new tri_pos (and tri_attr, or NULL) records for the whole range of one mesh."""
    _fields_ = [("mesh", C.c_uint32), ("tri_count", C.c_uint32), ("tri_pos", C.POINTER(TriPos)), ("tri_attr", C.POINTER(TriAttr))]


class MeshTopology(C.Structure):
    """spt_mesh_topology (spt_scene_mesh_topology); `size` is sizeof of the struct."""
    _fields_ = [("size", C.c_uint32), ("mesh", C.c_uint32), ("n_vertices", C.c_uint32), ("tri_count", C.c_uint32),
                ("indices", C.POINTER(C.c_uint32)), ("face_of_tri", C.POINTER(C.c_uint32)), ("uv", C.POINTER(C.c_float)),
                ("normals", C.POINTER(C.c_float))]


class MeshVertices(C.Structure):
    """spt_mesh_vertices (spt_scene_deform_vertices): new positions (and normals, or NULL) for every vertex of one mesh."""
    _fields_ = [("mesh", C.c_uint32), ("n_vertices", C.c_uint32), ("positions", C.POINTER(C.c_float)), ("normals", C.POINTER(C.c_float))]


def _load(name: str) -> C.CDLL:
    path = os.path.join(LIB_DIR, name)
    if not os.path.exists(path):
        raise SptError(2 if "hip" in name else 100,
                       "%s is not built (run `make` or `python -c 'import __graft_entry__ as g; g.build()'`)" % path)
    return C.CDLL(path, mode=C.RTLD_GLOBAL)


_host_lib: Optional[C.CDLL] = None
_hip_lib: Optional[C.CDLL] = None


def host_lib() -> C.CDLL:
    global _host_lib
    if _host_lib is None:
        lib = _load("libspt_host.so")
        lib.spt_host_last_error.restype = C.c_char_p
        lib.spt_host_scene_set_bezier_newton.argtypes = [C.c_void_p, C.c_int32]
        lib.spt_host_multi_create.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p)]
        lib.spt_host_multi_render.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.spt_host_multi_device_count.argtypes = [C.c_void_p]
        lib.spt_host_multi_device_count.restype = C.c_uint32
        lib.spt_host_multi_destroy.argtypes = [C.c_void_p]
        lib.spt_host_multi_destroy.restype = None
        if hasattr(lib, "spt_host_multi_film_create"):   # additive: an older library (SPT_LIB_DIR, A/B runs) may lack them
            lib.spt_host_multi_film_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                                       C.c_uint32, C.POINTER(C.c_void_p)]
            lib.spt_host_multi_film_render.argtypes = [C.c_void_p, C.c_uint32]
            lib.spt_host_multi_film_adapt.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_uint32, C.POINTER(C.c_uint32)]
            lib.spt_host_multi_film_samples.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
            lib.spt_host_multi_film_read.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
            lib.spt_host_multi_film_read_counts.argtypes = [C.c_void_p, C.c_void_p]
            lib.spt_host_multi_film_read_robust.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
            lib.spt_host_multi_film_read_rgb8.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
            lib.spt_host_multi_film_denoise.argtypes = [C.c_void_p, C.POINTER(MultiFilmDenoiseJob), C.c_void_p]
            lib.spt_host_multi_film_destroy.argtypes = [C.c_void_p]
            lib.spt_host_multi_film_destroy.restype = None
        lib.spt_host_load_scene.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        lib.spt_host_scene_desc.argtypes = [C.c_void_p]
        lib.spt_host_scene_desc.restype = C.POINTER(SceneDesc)
        lib.spt_host_scene_camera.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(Camera)]
        lib.spt_host_scene_free.argtypes = [C.c_void_p]
        lib.spt_host_scene_free.restype = None
        if hasattr(lib, "spt_host_scene_set_transforms"):   # (the same)
            lib.spt_host_scene_instance_index.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint32)]
            lib.spt_host_scene_set_transforms.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_char_p), C.c_void_p]
            lib.spt_host_scene_set_light.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(Light)]
        if hasattr(lib, "spt_host_scene_set_mesh_positions"):   # (the same)
            lib.spt_host_scene_mesh_positions.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint32), C.c_void_p]
            lib.spt_host_scene_set_mesh_positions.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p]
            lib.spt_host_scene_mesh_index.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint32)]
        if hasattr(lib, "spt_host_scene_set_mesh_vertices"):   # (the same)
            lib.spt_host_scene_mesh_topology.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(MeshTopology)]
            lib.spt_host_scene_set_mesh_vertices.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p]
            lib.spt_host_scene_dynamic.argtypes = [C.c_void_p, C.POINTER(SceneUpdateDesc)]
        if hasattr(lib, "spt_host_origin_candidates"):   # (the same)
            lib.spt_host_origin_candidates.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_void_p]
        if hasattr(lib, "spt_host_block_candidates"):   # (the same)
            lib.spt_host_block_candidates.argtypes = [C.POINTER(Camera)] + [C.c_uint32] * 7 + [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                                                                             C.POINTER(C.c_uint64)]
        if hasattr(lib, "spt_host_camera_rays"):
            lib.spt_host_camera_rays.argtypes = [C.POINTER(CameraModel), C.POINTER(RenderParams), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        if hasattr(lib, "spt_host_bake_rays"):
            lib.spt_host_bake_rays.argtypes = [C.POINTER(SceneDesc), C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32,
                                               C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            lib.spt_host_lightmap_points.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64,
                                                     C.POINTER(C.c_uint64)]
        if hasattr(lib, "spt_host_probe_rays"):
            lib.spt_host_probe_rays.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            lib.spt_host_probe_basis.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p]
        lib.spt_host_load_renderer.argtypes = [C.c_char_p, C.POINTER(RenderParams), C.POINTER(C.c_float)]
        if hasattr(lib, "spt_host_load_renderer_filter"):   # (a library built before the weighted filters lacks it)
            lib.spt_host_load_renderer_filter.argtypes = [C.c_char_p, C.POINTER(RenderParams), C.POINTER(FilterDesc)]
        lib.spt_host_film_to_rgb8.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        lib.spt_host_film_to_rgb8.restype = None
        lib.spt_host_write_png.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32]
        lib.spt_host_write_image.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32]
        lib.spt_host_write_jpeg.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32]
        lib.spt_host_read_exr.argtypes = [C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                          C.POINTER(C.POINTER(C.c_float))]
        lib.spt_host_write_exr.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32]
        lib.spt_host_catmull_clark.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.POINTER(C.c_float))]
        lib.spt_host_free.argtypes = [C.c_void_p]
        lib.spt_host_free.restype = None
        _host_lib = lib
    return _host_lib


def hip_lib() -> C.CDLL:
    """The product path.  Raises if libspt_hip.so is missing — never falls back."""
    global _hip_lib
    if _hip_lib is None:
        lib = _load("libspt_hip.so")
        lib.spt_last_error.restype = C.c_char_p
        lib.spt_abi_version.restype = C.c_uint32
        got = lib.spt_abi_version()
        if got != SPT_ABI_VERSION:   # the ctypes mirrors above would mis-size every struct: fail before any call uses them
            raise SptError(1, "libspt_hip.so exports ABI version %d, this binding mirrors version %d (rebuild: `make`)" % (got, SPT_ABI_VERSION))
        lib.spt_device_count.argtypes = [C.POINTER(C.c_int32)]
        lib.spt_scene_create.argtypes = [C.POINTER(SceneDesc), C.c_int32, C.POINTER(C.c_void_p)]
        lib.spt_scene_destroy.argtypes = [C.c_void_p]
        lib.spt_scene_destroy.restype = None
        lib.spt_render.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.c_void_p,
                                   C.POINTER(RenderStats)]
        lib.spt_render_wait.argtypes = [C.c_void_p]
        lib.spt_shard_rows.argtypes = [C.POINTER(RenderParams), C.POINTER(C.c_uint32)]
        lib.spt_trace_closest.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.spt_trace_any.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.spt_alloc_pinned.argtypes = [C.c_uint64, C.POINTER(C.c_void_p)]
        lib.spt_free_pinned.argtypes = [C.c_void_p]
        lib.spt_free_pinned.restype = None
        lib.spt_pin_host.argtypes = [C.c_void_p, C.c_uint64]
        lib.spt_unpin_host.argtypes = [C.c_void_p]
        lib.spt_unpin_host.restype = None
        lib.spt_film_create.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
        lib.spt_film_render.argtypes = [C.c_void_p, C.c_uint32]
        lib.spt_film_samples.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        lib.spt_film_read.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        lib.spt_film_destroy.argtypes = [C.c_void_p]
        lib.spt_film_destroy.restype = None
        lib.spt_film_adapt.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_uint32, C.POINTER(C.c_uint32)]
        lib.spt_film_read_counts.argtypes = [C.c_void_p, C.c_void_p]
        if hasattr(lib, "spt_film_denoise"):   # additive to ABI v14: an older library (SPT_LIB_DIR, A/B runs) may lack it
            lib.spt_film_denoise.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(DenoiseParams), C.c_void_p]
        if hasattr(lib, "spt_film_buckets"):   # (the same)
            lib.spt_film_buckets.argtypes = [C.c_void_p, C.c_uint32]
            lib.spt_film_read_buckets.argtypes = [C.c_void_p, C.c_void_p]
            lib.spt_film_read_robust.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        if hasattr(lib, "spt_film_denoise_job"):   # (the same)
            lib.spt_film_denoise_job.argtypes = [C.c_void_p, C.POINTER(DenoiseJob), C.c_void_p]
            lib.spt_render_flags_supported.argtypes = [C.POINTER(C.c_uint32)]
        if hasattr(lib, "spt_film_read_rgb8"):   # (the same)
            lib.spt_film_read_rgb8.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(DenoiseParams), C.c_void_p]
            lib.spt_debug_pack_rgb8.argtypes = [C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p]
        if hasattr(lib, "spt_film_filter"):   # (the same)
            lib.spt_film_filter.argtypes = [C.c_void_p, C.POINTER(FilterDesc)]
        if hasattr(lib, "spt_film_read_samples"):   # (the same)
            lib.spt_film_read_samples.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        if hasattr(lib, "spt_denoise_image"):   # (the same)
            lib.spt_denoise_image.argtypes = [C.c_void_p, C.POINTER(ImageDenoiseJob), C.c_void_p]
        if hasattr(lib, "spt_radiance"):   # (the same)
            lib.spt_radiance.argtypes = [C.c_void_p, C.POINTER(RadianceJob)]
        if hasattr(lib, "spt_bake"):   # (the same)
            lib.spt_bake.argtypes = [C.c_void_p, C.POINTER(BakeJob)]
        if hasattr(lib, "spt_probe"):   # (the same)
            lib.spt_probe.argtypes = [C.c_void_p, C.POINTER(ProbeJob)]
        if hasattr(lib, "spt_gbuffer"):   # (the same)
            lib.spt_gbuffer.argtypes = [C.c_void_p, C.POINTER(GBufferJob)]
        if hasattr(lib, "spt_occluded"):   # (the same)
            lib.spt_occluded.argtypes = [C.c_void_p, C.POINTER(OccludedJob)]
        if hasattr(lib, "spt_hits"):   # (the same)
            lib.spt_hits.argtypes = [C.c_void_p, C.POINTER(HitsJob)]
        if hasattr(lib, "spt_ao"):   # (the same)
            lib.spt_ao.argtypes = [C.c_void_p, C.POINTER(AoJob)]
        if hasattr(lib, "spt_camera_rays"):   # (the same)
            lib.spt_camera_rays.argtypes = [C.c_void_p, C.POINTER(CameraRaysJob)]
        if hasattr(lib, "spt_camera_gbuffer"):   # (the same)
            lib.spt_camera_gbuffer.argtypes = [C.c_void_p, C.POINTER(CameraGBufferJob)]
        if hasattr(lib, "spt_scene_update"):   # (the same)
            lib.spt_scene_update.argtypes = [C.c_void_p, C.POINTER(SceneUpdateDesc)]
        if hasattr(lib, "spt_scene_deform"):   # (the same)
            lib.spt_scene_deform.argtypes = [C.c_void_p, C.POINTER(SceneUpdateDesc), C.c_uint32, C.POINTER(MeshDeform)]
        if hasattr(lib, "spt_scene_deform_vertices"):   # (the same)
            lib.spt_scene_mesh_topology.argtypes = [C.c_void_p, C.POINTER(MeshTopology)]
            lib.spt_scene_deform_vertices.argtypes = [C.c_void_p, C.POINTER(SceneUpdateDesc), C.c_uint32, C.POINTER(MeshVertices)]
            lib.spt_scene_read_triangles.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        if hasattr(lib, "spt_render_camera"):
            lib.spt_render_camera.argtypes = [C.c_void_p, C.POINTER(CameraModel), C.POINTER(RenderParams), C.c_void_p, C.POINTER(RenderStats)]
            lib.spt_film_create_camera.argtypes = [C.c_void_p, C.POINTER(CameraModel), C.POINTER(RenderParams), C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
        lib.spt_debug_detmath.argtypes = [C.c_int32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.spt_debug_bxdf.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Material), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(lib, "spt_debug_render_info"):   # (the same)
            lib.spt_debug_render_info.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]
        if hasattr(lib, "spt_scene_origin_candidates"):   # (the same)
            lib.spt_scene_origin_candidates.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]
        _hip_lib = lib
    return _hip_lib


def _check_host(status: int) -> None:
    if status != 0:
        raise SptError(status, host_lib().spt_host_last_error().decode("utf-8", "replace"))


def _check_hip(status: int) -> None:
    if status != 0:
        raise SptError(status, hip_lib().spt_last_error().decode("utf-8", "replace"))


# ---- host side: Scene / renderer loading -----------------------------------------------

class Scene:
    """Flattened scene (reference `Scene`, src/core/scene.rs:9-14) owned by libspt_host."""

    def __init__(self, path: str):
        self._h = C.c_void_p()
        _check_host(host_lib().spt_host_load_scene(os.fspath(path).encode(), C.byref(self._h)))
        self.path = os.fspath(path)
        self._device_scenes = {}
        self._mesh_gen = {}   # mesh index -> how often set_mesh_positions / set_mesh_vertices has edited it (a DeviceScene compares with what it has seen)
        self._mesh_nrm_gen = {}    # ... and how often one of them gave it new normals
        self._mesh_by_vertices = {}   # mesh index -> the primitive's name while its latest edit came by set_mesh_vertices

    @property
    def desc(self) -> SceneDesc:
        return host_lib().spt_host_scene_desc(self._h).contents

    def get_camera(self, name=None) -> Camera:
        """Scene::get_camera (src/core/scene.rs): by name, the first one for None; a Camera instance is passed through
        (callers that place their own camera, e.g. tests)."""
        if isinstance(name, Camera):
            return name
        cam = Camera()
        _check_host(host_lib().spt_host_scene_camera(self._h, name.encode() if name else None, C.byref(cam)))
        return cam

    def array(self, field: str) -> np.ndarray:
        """Copy of one desc array as a structured / float numpy array (for tests)."""
        d = self.desc
        table = {
            "tlas_nodes": (d.tlas_nodes, d.n_tlas_nodes, BvhNode), "blas_nodes": (d.blas_nodes, d.n_blas_nodes, BvhNode),
            "instances": (d.instances, d.n_instances, Instance), "meshes": (d.meshes, d.n_meshes, Mesh),
            "tri_pos": (d.tri_pos, d.n_tris, TriPos), "tri_attr": (d.tri_attr, d.n_tris, TriAttr),
            "spheres": (d.spheres, d.n_spheres, Sphere), "surfaces": (d.surfaces, d.n_surfaces, Surface),
            "materials": (d.materials, d.n_materials, Material), "mediums": (d.mediums, d.n_mediums, Medium),
            "lights": (d.lights, d.n_lights, Light),
            "textures": (d.textures, d.n_textures, Texture), "images": (d.images, d.n_images, Image),
            "image_levels": (d.image_levels, d.n_image_levels, ImageLevel), "texels": (d.texels, d.n_texels, C.c_uint32),
            "material_recipes": (d.material_recipes, d.n_material_recipes, MaterialRecipe),
            "bezier_patches": (d.bezier_patches, d.n_bezier_patches, BezierPatch),
            "pndfs": (d.pndfs, d.n_pndfs, Pndf), "pndf_terms": (d.pndf_terms, d.n_pndf_terms, PndfTerm),
            "pndf_nodes": (d.pndf_nodes, d.n_pndf_nodes, PndfNode), "pndf_refs": (d.pndf_refs, d.n_pndf_refs, C.c_uint32),
            "pndf_roots": (d.pndf_roots, d.n_pndf_roots, C.c_uint32),
        }
        ptr, n, ty = table[field]
        if n == 0:
            return np.zeros((0,), dtype=np.dtype(ty))
        buf = C.string_at(ptr, n * C.sizeof(ty))
        return np.frombuffer(buf, dtype=np.dtype(ty)).copy()

    def _dynamic_host(self):
        lib = host_lib()
        if not hasattr(lib, "spt_host_scene_set_transforms"):
            raise SptError(4, "this libspt_host.so cannot edit a loaded scene (no spt_host_scene_set_transforms)")
        return lib

    def lightmap_points(self, name: str, width: int, height: int):
        """spt_host_lightmap_points: the covered texels of a width x height lightmap of the mesh instance `name` as (points, texels):
        BAKE_POINT_DTYPE records for DeviceScene.bake and the texels' linear indices y * width + x, in texel order.  The centre of
        texel (x, y) is uv ((x + 0.5) / W, (y + 0.5) / H); the lowest triangle index that contains it wins; no dilation."""
        lib = host_lib()
        if not hasattr(lib, "spt_host_lightmap_points"):
            raise SptError(4, "libspt_host.so does not export spt_host_lightmap_points")
        n = C.c_uint64(0)
        _check_host(lib.spt_host_lightmap_points(self._h, name.encode(), width, height, None, None, 0, C.byref(n)))
        points, texels = np.zeros(n.value, dtype=BAKE_POINT_DTYPE), np.zeros(n.value, dtype=np.uint32)
        if n.value:
            _check_host(lib.spt_host_lightmap_points(self._h, name.encode(), width, height, points.ctypes.data, texels.ctypes.data, n.value, C.byref(n)))
        return points, texels

    def instance_index(self, name: str) -> int:
        """The index of the instance called `name` in the CURRENT descriptor (set_transforms reorders the instances)."""
        index = C.c_uint32(0)
        _check_host(self._dynamic_host().spt_host_scene_instance_index(self._h, name.encode(), C.byref(index)))
        return int(index.value)

    def set_transforms(self, transforms) -> None:
        """spt_host_scene_set_transforms: {instance name: object-to-world transform}, each 12 floats in the layout of
        spt_instance::fwd (three columns, then the translation) or a 3x4 matrix [M | t].  The descriptor becomes the one the
        loader makes of the scene file with these transforms written in; a refused call leaves it as it was.  A DeviceScene
        keeps rendering the old state until its update()."""
        lib = self._dynamic_host()
        names = list(transforms)
        fwd = np.zeros((len(names), 12), dtype=np.float32)
        for i, name in enumerate(names):
            m = np.asarray(transforms[name], dtype=np.float32)
            if m.shape == (3, 4):
                m = m.T.reshape(12)      # rows of [M | t] -> columns
            if m.shape != (12,):
                raise ValueError("%s: 12 floats or a 3x4 matrix are expected" % name)
            fwd[i] = m
        c_names = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
        _check_host(lib.spt_host_scene_set_transforms(self._h, len(names), c_names, fwd.ctypes.data))

    def set_light(self, name: str, light: "Light") -> None:
        """spt_host_scene_set_light: replaces the directional, point or spot light called `name` (same type)."""
        _check_host(self._dynamic_host().spt_host_scene_set_light(self._h, name.encode(), C.byref(light)))

    def _mesh_host(self):
        lib = host_lib()
        if not hasattr(lib, "spt_host_scene_set_mesh_positions"):
            raise SptError(4, "this libspt_host.so cannot deform a loaded mesh (no spt_host_scene_set_mesh_positions)")
        return lib

    def mesh_index(self, name: str) -> int:
        """The index in the descriptor's meshes[] of the trimesh primitive called `name`."""
        index = C.c_uint32(0)
        _check_host(self._mesh_host().spt_host_scene_mesh_index(self._h, name.encode(), C.byref(index)))
        return int(index.value)

    def mesh_positions(self, name: str) -> np.ndarray:
        """spt_host_scene_mesh_positions: the (n_vertices, 3) f32 vertex positions of the trimesh primitive `name`, in the OBJ
        loader's single-index vertex order."""
        lib = self._mesh_host()
        n = C.c_uint32(0)
        _check_host(lib.spt_host_scene_mesh_positions(self._h, name.encode(), C.byref(n), None))
        out = np.zeros((n.value, 3), dtype=np.float32)
        _check_host(lib.spt_host_scene_mesh_positions(self._h, name.encode(), C.byref(n), out.ctypes.data))
        return out

    def set_mesh_positions(self, name: str, positions, normals=None) -> None:
        """spt_host_scene_set_mesh_positions: new vertex positions (and normals, or None to keep them) for the trimesh primitive
        `name`; triangles, uvs and counts stay.  The descriptor becomes the one the loader makes of these vertices (tangents,
        triangle records, the caller-side BLAS boxes, instance boxes, TLAS, shape-light power, alias table); a refused call leaves
        it as it was.  The mesh is marked dirty: a DeviceScene keeps the old geometry until its update()."""
        lib = self._mesh_host()
        mesh = self.mesh_index(name)
        pos = np.ascontiguousarray(positions, dtype=np.float32)
        if pos.ndim != 2 or pos.shape[1] != 3:
            raise ValueError("positions: an (n_vertices, 3) array is expected")
        nrm = None
        if normals is not None:
            nrm = np.ascontiguousarray(normals, dtype=np.float32)
            if nrm.shape != pos.shape:
                raise ValueError("normals: one normal per position is expected")
        _check_host(lib.spt_host_scene_set_mesh_positions(self._h, name.encode(), pos.shape[0], pos.ctypes.data, nrm.ctypes.data if nrm is not None else None))
        self._mesh_gen[mesh] = self._mesh_gen.get(mesh, 0) + 1
        if nrm is not None:
            self._mesh_nrm_gen[mesh] = self._mesh_nrm_gen.get(mesh, 0) + 1
        self._mesh_by_vertices.pop(mesh, None)

    def _vertices_host(self):
        lib = host_lib()
        if not hasattr(lib, "spt_host_scene_set_mesh_vertices"):
            raise SptError(4, "this libspt_host.so cannot deform a loaded mesh by its vertices (no spt_host_scene_set_mesh_vertices)")
        return lib

    def _mesh_topology(self, name: str) -> "MeshTopology":
        """spt_host_scene_mesh_topology: the struct, its pointers into the host scene (valid until close())."""
        t = MeshTopology()
        _check_host(self._vertices_host().spt_host_scene_mesh_topology(self._h, name.encode(), C.byref(t)))
        return t

    def mesh_topology(self, name: str) -> dict:
        """spt_host_scene_mesh_topology as numpy copies: mesh, indices (tri_count, 3) in face order, face_of_tri (tri_count,), uv
        (n_vertices, 2) and the normals in force (n_vertices, 3) - what DeviceScene.set_topology takes."""
        t = self._mesh_topology(name)
        nv, nt = int(t.n_vertices), int(t.tri_count)
        return {"mesh": int(t.mesh),
                "indices": np.ctypeslib.as_array(t.indices, shape=(nt, 3)).copy(),
                "face_of_tri": np.ctypeslib.as_array(t.face_of_tri, shape=(nt,)).copy(),
                "uv": np.ctypeslib.as_array(t.uv, shape=(nv, 2)).copy(),
                "normals": np.ctypeslib.as_array(t.normals, shape=(nv, 3)).copy()}

    def set_mesh_vertices(self, name: str, positions, normals=None) -> None:
        """spt_host_scene_set_mesh_vertices: set_mesh_positions with the mesh's triangle records and BLAS boxes left to be made
        when somebody reads the descriptor (`desc`, `array`); instances, TLAS, lights and alias table follow at once.  A
        DeviceScene.update() after it sends the vertices, not records, and the device makes its own records."""
        lib = self._vertices_host()
        mesh = self.mesh_index(name)
        pos = np.ascontiguousarray(positions, dtype=np.float32)
        if pos.ndim != 2 or pos.shape[1] != 3:
            raise ValueError("positions: an (n_vertices, 3) array is expected")
        nrm = None
        if normals is not None:
            nrm = np.ascontiguousarray(normals, dtype=np.float32)
            if nrm.shape != pos.shape:
                raise ValueError("normals: one normal per position is expected")
        _check_host(lib.spt_host_scene_set_mesh_vertices(self._h, name.encode(), pos.shape[0], pos.ctypes.data, nrm.ctypes.data if nrm is not None else None))
        self._mesh_gen[mesh] = self._mesh_gen.get(mesh, 0) + 1
        if nrm is not None:
            self._mesh_nrm_gen[mesh] = self._mesh_nrm_gen.get(mesh, 0) + 1
        self._mesh_by_vertices[mesh] = name

    def device_scene(self, device: int = 0) -> "DeviceScene":
        if device not in self._device_scenes:
            self._device_scenes[device] = DeviceScene(self, device)
        return self._device_scenes[device]

    def close_device_scene(self, device: int = 0) -> None:
        """Destroys the device scene on `device`, if there is one (spt_render_wait + spt_scene_destroy); the next device_scene(device)
        creates it again from the descriptor as it then stands."""
        ds = self._device_scenes.pop(device, None)
        if ds is not None:
            ds.close()

    def close(self) -> None:
        for ds in self._device_scenes.values():
            ds.close()
        self._device_scenes.clear()
        if self._h:
            host_lib().spt_host_scene_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def load_scene(path: str, bezier_newton: Optional[bool] = None) -> Scene:
    """loader::load_scene (src/loader/mod.rs:20-31).  bezier_newton: True = the reference built with `--features bezier_ni`
    (patches intersected by Newton's iteration), False = Bezier clipping, None = the process default (clipping unless the
    environment variable SPT_BEZIER_NI is set).  Per scene: two scenes of one process may differ."""
    sc = Scene(path)
    if bezier_newton is not None:
        _check_host(host_lib().spt_host_scene_set_bezier_newton(sc._h, 1 if bezier_newton else 0))
    return sc


class DeviceScene:
    """HBM-resident copy of a Scene (spt_scene_create)."""

    def __init__(self, scene: Scene, device: int = 0):
        self._h = C.c_void_p()
        self.scene = scene
        self.device = device
        self._pinned = {}
        self._films = weakref.WeakSet()   # ProgressiveFilm objects on this scene: destroyed before it
        desc = scene.desc
        self._mesh_seen = dict(scene._mesh_gen)
        self._mesh_ranges = [(int(desc.meshes[m].tri_first), int(desc.meshes[m].tri_count)) for m in range(desc.n_meshes)]
        self._topology_nrm = {}   # mesh index -> Scene._mesh_nrm_gen of the normals this device scene's registration holds
        _check_hip(hip_lib().spt_scene_create(C.byref(desc), device, C.byref(self._h)))

    def film_buffer(self, rows: int, width: int) -> np.ndarray:
        """Reusable page-locked (rows, width, 3) f32 output buffer (spt_alloc_pinned)."""
        key = (rows, width)
        if key not in self._pinned:
            nbytes = max(rows * width * 3 * 4, 4)
            ptr = C.c_void_p()
            _check_hip(hip_lib().spt_alloc_pinned(nbytes, C.byref(ptr)))
            buf = (C.c_float * (rows * width * 3)).from_address(ptr.value)
            self._pinned[key] = (ptr, np.ctypeslib.as_array(buf).reshape(rows, width, 3))
        return self._pinned[key][1]

    def trace_closest(self, rays: np.ndarray) -> np.ndarray:
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        hits = np.zeros(rays.shape[0], dtype=HIT_DTYPE)
        _check_hip(hip_lib().spt_trace_closest(self._h, rays.shape[0], rays.ctypes.data, hits.ctypes.data))
        return hits

    def trace_any(self, rays: np.ndarray) -> np.ndarray:
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        occ = np.zeros(rays.shape[0], dtype=np.uint8)
        _check_hip(hip_lib().spt_trace_any(self._h, rays.shape[0], rays.ctypes.data, occ.ctypes.data))
        return occ

    @staticmethod
    def _entry(name: str):
        """The HIP library, which must export `name` (additive to ABI v14: an older library may lack it)."""
        lib = hip_lib()
        if not hasattr(lib, name):
            raise SptError(4, "this libspt_hip.so has no %s" % name)
        return lib

    def _check_tensor(self, t, what: str, widths) -> None:
        """`t` holds one record of one of `widths` float32 words per row, contiguous, on the scene's device."""
        import torch
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] not in widths or not t.is_contiguous():
            raise ValueError("%s: a contiguous float32 %s tensor is expected" % (what, " or ".join("(n, %d)" % w for w in widths)))
        if t.device.type != "cuda" or t.device.index != self.device:
            raise ValueError("%s: the tensor must live on the scene's device (cuda:%d)" % (what, self.device))

    @staticmethod
    def _producer_done(t) -> None:
        """The records of `t` are complete before the library's stream reads them."""
        import torch
        torch.cuda.current_stream(t.device).synchronize()

    def radiance(self, rays, aux=None, repeats: int = 1, max_depth: int = 8, seed: int = 1, rng_skip: int = 0, rays_per_pass: int = 0,
                 hits: bool = False):
        """spt_radiance: the radiance arriving along caller rays, (n, 3) f32; with `hits` also the closest hit of every ray's first
        segment, as a second result.  rays / aux are PATH_RAY_DTYPE / RAY_AUX_DTYPE arrays (see perspective_rays and the other
        generators), or contiguous float32 torch tensors on the scene's device of shape (n, 12) / (n, 16) holding the same records
        (stream_a / stream_b as bit patterns): then the producer's current stream is synchronised, the library reads and writes
        device memory and the results are tensors, the hits an (n, 5) int32 tensor of the spt_hit words."""
        lib = self._entry("spt_radiance")
        job = RadianceJob(size=C.sizeof(RadianceJob), repeats=repeats, max_depth=max_depth, seed=seed, rng_skip=rng_skip, rays_per_pass=rays_per_pass)
        if type(rays).__module__.split(".")[0] == "torch":
            import torch
            self._check_tensor(rays, "rays", (12,))
            if aux is not None:
                self._check_tensor(aux, "aux", (16,))
            n = rays.shape[0]
            if aux is not None and aux.shape[0] != n:
                raise ValueError("aux: one record per ray is expected")
            out = torch.empty((n, 3), dtype=torch.float32, device=rays.device)
            hit = torch.empty((n, 5), dtype=torch.int32, device=rays.device) if hits else None
            self._producer_done(rays)
            job.flags, job.n_rays = RADIANCE_DEVICE_POINTERS, n
            job.rays, job.aux = rays.data_ptr() if n else None, aux.data_ptr() if aux is not None and n else None
            job.rgb_out, job.hits_out = out.data_ptr() if n else None, hit.data_ptr() if hits and n else None
            _check_hip(lib.spt_radiance(self._h, C.byref(job)))
            return (out, hit) if hits else out
        rays = np.ascontiguousarray(rays, dtype=PATH_RAY_DTYPE).reshape(-1)
        n = rays.shape[0]
        if aux is not None:
            aux = np.ascontiguousarray(aux, dtype=RAY_AUX_DTYPE).reshape(-1)
            if aux.shape[0] != n:
                raise ValueError("aux: one record per ray is expected")
        out = np.zeros((n, 3), dtype=np.float32)
        hit = np.zeros(n, dtype=HIT_DTYPE) if hits else None
        job.n_rays = n
        job.rays, job.aux = rays.ctypes.data, aux.ctypes.data if aux is not None else None
        job.rgb_out, job.hits_out = out.ctypes.data, hit.ctypes.data if hits else None
        _check_hip(lib.spt_radiance(self._h, C.byref(job)))
        return (out, hit) if hits else out

    def gbuffer(self, rays, aux=None, rays_per_pass: int = 0):
        """spt_gbuffer: per caller ray the surface it sees first, n GBUFFER_DTYPE records (p, t, n, instance, albedo, prim, v, w,
        surface, flags; a miss has t = f32::MAX, instance = prim = -1 and zeros elsewhere).  rays / aux are PATH_RAY_DTYPE /
        RAY_AUX_DTYPE arrays as radiance takes them (the streams are ignored), or contiguous float32 torch tensors on the scene's
        device of shape (n, 12) / (n, 16): then the producer's current stream is synchronised, the library reads and writes device
        memory and the result is an (n, 16) float32 tensor holding the same 64-byte records; its integer fields (columns 7
        instance, 11 prim, 14 surface, 15 flags) are read through .view(torch.int32)."""
        lib = self._entry("spt_gbuffer")
        job = GBufferJob(size=C.sizeof(GBufferJob), flags=0, rays_per_pass=rays_per_pass)
        if type(rays).__module__.split(".")[0] == "torch":
            import torch
            self._check_tensor(rays, "rays", (12,))
            if aux is not None:
                self._check_tensor(aux, "aux", (16,))
            n = rays.shape[0]
            if aux is not None and aux.shape[0] != n:
                raise ValueError("aux: one record per ray is expected")
            out = torch.empty((n, 16), dtype=torch.float32, device=rays.device)
            self._producer_done(rays)
            job.flags, job.n_rays = GBUFFER_DEVICE_POINTERS, n
            job.rays, job.aux = rays.data_ptr() if n else None, aux.data_ptr() if aux is not None and n else None
            job.out = out.data_ptr() if n else None
            _check_hip(lib.spt_gbuffer(self._h, C.byref(job)))
            return out
        rays = np.ascontiguousarray(rays, dtype=PATH_RAY_DTYPE).reshape(-1)
        n = rays.shape[0]
        if aux is not None:
            aux = np.ascontiguousarray(aux, dtype=RAY_AUX_DTYPE).reshape(-1)
            if aux.shape[0] != n:
                raise ValueError("aux: one record per ray is expected")
        out = np.zeros(n, dtype=GBUFFER_DTYPE)
        job.n_rays = n
        job.rays, job.aux, job.out = rays.ctypes.data, aux.ctypes.data if aux is not None else None, out.ctypes.data
        _check_hip(lib.spt_gbuffer(self._h, C.byref(job)))
        return out

    def camera_rays(self, model: "CameraModel", renderer: "PathTracer", width: int, height: int, first: int = 0, count: Optional[int] = None,
                    aux: bool = False, on_device: bool = False, rays_per_pass: int = 0):
        """spt_camera_rays: the records of the module's camera_rays, word for word, made by a kernel on the scene's device:
        (count, height, width) PATH_RAY_DTYPE records, with aux=True (rays, aux) with their RAY_AUX_DTYPE records.  on_device=True:
        float32 torch tensors on the scene's device instead, (count, height, width, 12) and (count, height, width, 16) holding the
        same records; reshaped to (n, 12) / (n, 16) they are what radiance and gbuffer take, and the first eight columns with a
        t_max written into the last of them what occluded takes."""
        lib = self._entry("spt_camera_rays")
        if count is None:
            count = renderer.spp - first
        p = renderer.params(width, height)
        job = CameraRaysJob(size=C.sizeof(CameraRaysJob), model=C.addressof(model), plan=C.addressof(p), first=first, count=count, rays_per_pass=rays_per_pass)
        if on_device:
            import torch
            dev = torch.device("cuda", self.device)
            rays = torch.empty((count, height, width, 12), dtype=torch.float32, device=dev)
            ax = torch.empty((count, height, width, 16), dtype=torch.float32, device=dev) if aux else None
            self._producer_done(rays)   # (the allocator may hand out memory that work queued on torch's stream still uses)
            job.flags = CAMERA_RAYS_DEVICE_POINTERS
            job.rays, job.aux = rays.data_ptr() if rays.numel() else None, ax.data_ptr() if aux and ax.numel() else None
        else:
            rays = np.zeros((count, height, width), dtype=PATH_RAY_DTYPE)
            ax = np.zeros((count, height, width), dtype=RAY_AUX_DTYPE) if aux else None
            job.rays, job.aux = rays.ctypes.data, ax.ctypes.data if aux else None
        _check_hip(lib.spt_camera_rays(self._h, C.byref(job)))
        return (rays, ax) if aux else rays

    def camera_gbuffer(self, model: "CameraModel", renderer: "PathTracer", width: int, height: int, samples: int = 1, first: int = 0,
                       on_device: bool = False, rays_per_pass: int = 0) -> dict:
        """spt_camera_gbuffer: the first-hit images of the plan samples first .. first + samples - 1 of a camera model, made on the
        device from the rays camera_rays makes: the dict the module's camera_gbuffer returns ("albedo" and "normal" (height, width,
        3), "depth" and "coverage" (height, width), float32), word for word.  on_device=True: torch tensors on the scene's device."""
        if samples < 1:
            raise ValueError("samples must be >= 1")
        lib = self._entry("spt_camera_gbuffer")
        p = renderer.params(width, height)
        job = CameraGBufferJob(size=C.sizeof(CameraGBufferJob), model=C.addressof(model), plan=C.addressof(p), first=first, count=samples,
                               rays_per_pass=rays_per_pass)
        shapes = {"albedo": (height, width, 3), "normal": (height, width, 3), "depth": (height, width), "coverage": (height, width)}
        if on_device:
            import torch
            dev = torch.device("cuda", self.device)
            out = {k: torch.empty(s, dtype=torch.float32, device=dev) for k, s in shapes.items()}
            self._producer_done(out["albedo"])
            job.flags = CAMERA_GBUFFER_DEVICE_POINTERS
            for k, t in out.items():
                setattr(job, k, t.data_ptr())
        else:
            out = {k: np.zeros(s, dtype=np.float32) for k, s in shapes.items()}
            for k, a in out.items():
                setattr(job, k, a.ctypes.data)
        _check_hip(lib.spt_camera_gbuffer(self._h, C.byref(job)))
        return out

    def bake(self, points, samples: int = 16, max_depth: int = 8, seed: int = 1, first_point: int = 0, first_sample: int = 0,
             points_per_pass: int = 0, world: bool = False, flip: bool = False):
        """spt_bake: per point on the scene's surfaces the radiance a white Lambert surface would emit there (E / pi), (n, 3) f32.
        points are BAKE_POINT_DTYPE records (instance, prim, v, w: the fields of a hit), or BAKE_WORLD_DTYPE records (p, n) with
        world=True; or contiguous float32 torch tensors on the scene's device of shape (n, 4) / (n, 8) holding the same records
        (instance / prim as bit patterns): then the producer's current stream is synchronised, the library reads and writes device
        memory and the result is a tensor.  flip negates every normal."""
        lib = self._entry("spt_bake")
        job = BakeJob(size=C.sizeof(BakeJob), flags=BAKE_FLIP if flip else 0, kind=BAKE_POINTS_WORLD if world else BAKE_POINTS_SURFACE, samples=samples,
                      max_depth=max_depth, seed=seed, first_point=first_point & 0xffffffff, first_sample=first_sample, points_per_pass=points_per_pass)
        if type(points).__module__.split(".")[0] == "torch":
            import torch
            self._check_tensor(points, "points", (8 if world else 4,))
            n = points.shape[0]
            out = torch.empty((n, 3), dtype=torch.float32, device=points.device)
            self._producer_done(points)
            job.flags |= BAKE_DEVICE_POINTERS
            job.n_points, job.points, job.rgb_out = n, points.data_ptr() if n else None, out.data_ptr() if n else None
            _check_hip(lib.spt_bake(self._h, C.byref(job)))
            return out
        points = np.ascontiguousarray(points, dtype=BAKE_WORLD_DTYPE if world else BAKE_POINT_DTYPE).reshape(-1)
        n = points.shape[0]
        out = np.zeros((n, 3), dtype=np.float32)
        job.n_points, job.points, job.rgb_out = n, points.ctypes.data, out.ctypes.data
        _check_hip(lib.spt_bake(self._h, C.byref(job)))
        return out

    def occluded(self, rays, packed: bool = False, rays_per_pass: int = 0):
        """spt_occluded: whether anything lies on each caller segment (o, t_min, d, t_max), byte for byte what trace_any returns:
        uint8 (n,), 1 occluded; with packed=True ceil(n / 64) uint64 words instead, ray i at bit i & 63 of word i >> 6 (see
        pack_occluded / unpack_occluded).  rays are RAY_DTYPE records, or a contiguous float32 (n, 8) torch tensor on the scene's
        device holding the same records: then the producer's current stream is synchronised, the library reads and writes device
        memory and the result is a uint8 tensor, packed an int64 tensor holding the same words."""
        lib = self._entry("spt_occluded")
        job = OccludedJob(size=C.sizeof(OccludedJob), flags=OCCLUDED_PACKED if packed else 0, rays_per_pass=rays_per_pass)
        if type(rays).__module__.split(".")[0] == "torch":
            import torch
            self._check_tensor(rays, "rays", (8,))
            n = rays.shape[0]
            out = torch.empty(((n + 63) // 64,), dtype=torch.int64, device=rays.device) if packed else torch.empty((n,), dtype=torch.uint8, device=rays.device)
            self._producer_done(rays)
            job.flags |= OCCLUDED_DEVICE_POINTERS
            job.n_rays, job.rays, job.out = n, rays.data_ptr() if n else None, out.data_ptr() if n else None
            _check_hip(lib.spt_occluded(self._h, C.byref(job)))
            return out
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE).reshape(-1)
        n = rays.shape[0]
        out = np.zeros((n + 63) // 64, dtype=np.uint64) if packed else np.zeros(n, dtype=np.uint8)
        job.n_rays, job.rays, job.out = n, rays.ctypes.data, out.ctypes.data
        _check_hip(lib.spt_occluded(self._h, C.byref(job)))
        return out

    def all_hits(self, rays, max_hits: int = 4, count_all: bool = False, rays_per_pass: int = 0):
        """spt_hits: what each caller segment (o, t_min, d, t_max) crosses, nearest first: (records, counts), an (n, max_hits) array of
        HIT_REC_DTYPE (t, instance, prim, flags, v, w; flags & HIT_BACKFACING: the ray leaves through the face, or the far root of a
        sphere; bits 8..15 the primitive type; past the last crossing t = f32::MAX, instance = prim = -1) in ascending order of (t,
        instance, prim, backfacing), and n HIT_COUNT_DTYPE (total, back): the records written and the back-facing ones among them, or
        with count_all=True EVERY crossing of the segment (the records are the same either way).  A sphere gives up to two crossings,
        a ray through a shared edge both triangles.  max_hits is 0 .. 64, 0 (counters alone) only with count_all.  Record 0 is what
        trace_closest returns.  rays are RAY_DTYPE records, or a contiguous float32 (n, 8) torch tensor on the scene's device holding
        the same records: then the producer's current stream is synchronised, the library reads and writes device memory and the
        results are an (n, max_hits, 8) float32 tensor holding the 32-byte records (instance, prim and flags read through
        .view(torch.int32)) and an (n, 2) int32 tensor.  Scenes with Bezier patches are refused."""
        lib = self._entry("spt_hits")
        job = HitsJob(size=C.sizeof(HitsJob), flags=HITS_COUNT_ALL if count_all else 0, max_hits=max_hits, rays_per_pass=rays_per_pass)
        k = max(0, min(int(max_hits), 64))   # (the shape of the buffers only: the library judges max_hits itself)
        if type(rays).__module__.split(".")[0] == "torch":
            import torch
            self._check_tensor(rays, "rays", (8,))
            n = rays.shape[0]
            recs = torch.empty((n, k, 8), dtype=torch.float32, device=rays.device)
            counts = torch.empty((n, 2), dtype=torch.int32, device=rays.device)
            self._producer_done(rays)
            job.flags |= HITS_DEVICE_POINTERS
            job.n_rays, job.rays, job.counts = n, rays.data_ptr() if n else None, counts.data_ptr() if n else None
            job.hits = recs.data_ptr() if n and k else None
            _check_hip(lib.spt_hits(self._h, C.byref(job)))
            return recs, counts
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE).reshape(-1)
        n = rays.shape[0]
        recs = np.zeros((n, k), dtype=HIT_REC_DTYPE)
        counts = np.zeros(n, dtype=HIT_COUNT_DTYPE)
        job.n_rays, job.rays, job.counts = n, rays.ctypes.data, counts.ctypes.data
        job.hits = recs.ctypes.data if n and k else None
        _check_hip(lib.spt_hits(self._h, C.byref(job)))
        return recs, counts

    def enclosed(self, points, direction=(0.0, 0.0, 1.0)) -> np.ndarray:
        """Whether each of the (n, 3) points lies inside the scene's geometry: one all_hits call that counts every crossing of the ray
        from the point along `direction` (max_hits=0, count_all=True) and answers back > total - back, more crossings that leave a
        surface than enter one.  Valid for closed meshes whose faces point outward and for spheres; open or inward-facing meshes give
        no meaningful answer.  bool (n,)."""
        points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        rays = np.zeros(points.shape[0], dtype=RAY_DTYPE)
        rays["o"] = points
        rays["d"] = np.asarray(direction, dtype=np.float32)
        rays["t_min"] = 0.0
        rays["t_max"] = np.finfo(np.float32).max
        _, counts = self.all_hits(rays, max_hits=0, count_all=True)
        total, back = counts["total"].astype(np.int64), counts["back"].astype(np.int64)
        return back > total - back

    def ambient_occlusion(self, points, samples: int = 16, max_distance: float = float("inf"), seed: int = 1, first_point: int = 0,
                          first_sample: int = 0, points_per_pass: int = 0, world: bool = False, flip: bool = False):
        """spt_ao: cosine-weighted ambient occlusion and the bent normal at bake's points, n AO_DTYPE records: `count` of the
        `samples` gather rays of bake (the same seed, first_point, first_sample) found nothing within max_distance, `sum` adds their
        directions in sample order, open = count / samples, bent = normalize(sum) or 0.  points as bake takes them; torch tensors give
        an (n, 8) float32 tensor holding the same 32-byte records, `count` (column 7) read through .view(torch.int32)."""
        lib = self._entry("spt_ao")
        job = AoJob(size=C.sizeof(AoJob), flags=AO_FLIP if flip else 0, kind=BAKE_POINTS_WORLD if world else BAKE_POINTS_SURFACE, samples=samples,
                    max_distance=max_distance, seed=seed, first_point=first_point & 0xffffffff, first_sample=first_sample, points_per_pass=points_per_pass)
        if type(points).__module__.split(".")[0] == "torch":
            import torch
            self._check_tensor(points, "points", (8 if world else 4,))
            n = points.shape[0]
            out = torch.empty((n, 8), dtype=torch.float32, device=points.device)
            self._producer_done(points)
            job.flags |= AO_DEVICE_POINTERS
            job.n_points, job.points, job.out = n, points.data_ptr() if n else None, out.data_ptr() if n else None
            _check_hip(lib.spt_ao(self._h, C.byref(job)))
            return out
        points = np.ascontiguousarray(points, dtype=BAKE_WORLD_DTYPE if world else BAKE_POINT_DTYPE).reshape(-1)
        n = points.shape[0]
        out = np.zeros(n, dtype=AO_DTYPE)
        job.n_points, job.points, job.out = n, points.ctypes.data, out.ctypes.data
        _check_hip(lib.spt_ao(self._h, C.byref(job)))
        return out

    def probes(self, points, samples: int = 64, max_depth: int = 8, seed: int = 1, first_point: int = 0, first_sample: int = 0, aux: bool = False,
               points_per_pass: int = 0):
        """spt_probe: per free point in space the incident radiance projected onto the nine real SH of bands 0 .. 2, (n, 9, 3) f32
        (coefficient j = l(l+1)+m, RGB innermost); with aux=True also the (n, 4) visibility record (fraction of first segments that hit,
        fraction that hit a mesh from behind, mean and smallest hit distance).  points: an (n, 3) float array, PROBE_DTYPE records, or
        a contiguous float32 torch tensor on the scene's device of shape (n, 3) or (n, 4): then the producer's current stream is
        synchronised, the library reads and writes device memory and the results are tensors."""
        lib = self._entry("spt_probe")
        job = ProbeJob(size=C.sizeof(ProbeJob), flags=0, samples=samples, max_depth=max_depth, seed=seed, first_point=first_point & 0xffffffff,
                       first_sample=first_sample, points_per_pass=points_per_pass)
        if type(points).__module__.split(".")[0] == "torch":
            import torch
            self._check_tensor(points, "points", (3, 4))
            n = points.shape[0]
            if points.shape[1] == 3:   # the 16-byte records of the ABI
                points = torch.cat([points, torch.zeros((n, 1), dtype=torch.float32, device=points.device)], dim=1).contiguous()
            sh = torch.empty((n, 9, 3), dtype=torch.float32, device=points.device)
            vis = torch.empty((n, 4), dtype=torch.float32, device=points.device) if aux else None
            self._producer_done(points)
            job.flags |= PROBE_DEVICE_POINTERS
            job.n_points, job.points, job.sh_out = n, points.data_ptr() if n else None, sh.data_ptr() if n else None
            job.aux_out = vis.data_ptr() if aux and n else None
            _check_hip(lib.spt_probe(self._h, C.byref(job)))
            return (sh, vis) if aux else sh
        points = _probe_records(points)
        n = points.shape[0]
        sh = np.zeros((n, 9, 3), dtype=np.float32)
        vis = np.zeros((n, 4), dtype=np.float32) if aux else None
        job.n_points, job.points, job.sh_out = n, points.ctypes.data, sh.ctypes.data
        job.aux_out = vis.ctypes.data if aux else None
        _check_hip(lib.spt_probe(self._h, C.byref(job)))
        return (sh, vis) if aux else sh

    def update(self) -> None:
        """spt_scene_update with the Scene's current tlas_nodes, instances, lights and light alias table (after
        Scene.set_transforms / set_light): the device scene then behaves like one freshly created from the Scene.  Frames queued
        before with SPT_RENDER_ASYNC still deliver the old state.  The scene's films must be closed first.  Meshes edited since the
        last update go along: by spt_scene_deform_vertices when the latest edit of every one of them came by Scene.set_mesh_vertices
        (their topology is registered on first use), else by spt_scene_deform with the Scene's records."""
        dirty = sorted(m for m, gen in self.scene._mesh_gen.items() if self._mesh_seen.get(m) != gen)
        if dirty and all(m in self.scene._mesh_by_vertices for m in dirty) and hasattr(hip_lib(), "spt_scene_deform_vertices"):
            self._update_vertices(dirty)
            return
        d = self.scene.desc
        u = SceneUpdateDesc(size=C.sizeof(SceneUpdateDesc), flags=0, n_tlas_nodes=d.n_tlas_nodes, tlas_nodes=d.tlas_nodes,
                            n_instances=d.n_instances, instances=d.instances, n_lights=d.n_lights, lights=d.lights, light_alias=d.light_alias)
        if not dirty:
            self._update(u)
            return
        # meshes edited by Scene.set_mesh_positions since this device scene last saw them: their records as the Scene has them now
        edits = (MeshDeform * len(dirty))()
        for e, m in zip(edits, dirty):
            mesh = d.meshes[m]
            e.mesh, e.tri_count = m, mesh.tri_count
            e.tri_pos = C.cast(C.addressof(d.tri_pos[mesh.tri_first]), C.POINTER(TriPos))
            e.tri_attr = C.cast(C.addressof(d.tri_attr[mesh.tri_first]), C.POINTER(TriAttr))
        self._deform(u, edits)
        for m in dirty:
            self._mesh_seen[m] = self.scene._mesh_gen[m]

    def _update_vertices(self, dirty) -> None:
        """update() when every dirty mesh's latest edit came by Scene.set_mesh_vertices: spt_scene_deform_vertices with the
        Scene's stored vertices; nothing of the host scene is materialised."""
        scene, lib = self.scene, hip_lib()
        for m in dirty:   # the topology of meshes this device scene has not registered yet, straight from the host scene's arrays
            if m not in self._topology_nrm:
                t = scene._mesh_topology(scene._mesh_by_vertices[m])
                _check_hip(lib.spt_scene_mesh_topology(self._h, C.byref(t)))
                self._topology_nrm[m] = scene._mesh_nrm_gen.get(m, 0)
        u = SceneUpdateDesc()
        _check_host(host_lib().spt_host_scene_dynamic(scene._h, C.byref(u)))
        keep = []
        verts = (MeshVertices * len(dirty))()
        for v, m in zip(verts, dirty):
            name = scene._mesh_by_vertices[m]
            pos = scene.mesh_positions(name)
            keep.append(pos)
            v.mesh, v.n_vertices = m, pos.shape[0]
            v.positions = C.cast(pos.ctypes.data, C.POINTER(C.c_float))
            if self._topology_nrm[m] != scene._mesh_nrm_gen.get(m, 0):   # normals newer than the ones the device holds
                v.normals = scene._mesh_topology(name).normals
        _check_hip(lib.spt_scene_deform_vertices(self._h, C.byref(u), len(dirty), verts))
        for m in dirty:
            self._mesh_seen[m] = scene._mesh_gen[m]
            self._topology_nrm[m] = scene._mesh_nrm_gen.get(m, 0)

    def set_topology(self, mesh: int, indices, face_of_tri, uv, normals) -> None:
        """spt_scene_mesh_topology for callers with their own arrays (see Scene.mesh_topology): indices (tri_count, 3) in face
        order, face_of_tri (tri_count,) or None for the identity, uv (n_vertices, 2), normals (n_vertices, 3).  Everything is
        copied by the call; a second call for a mesh replaces its registration."""
        lib = hip_lib()
        if not hasattr(lib, "spt_scene_mesh_topology"):
            raise SptError(4, "this libspt_hip.so has no spt_scene_mesh_topology")
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1)
        nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1)
        if idx.shape[0] % 3 != 0 or uv.shape[0] % 2 != 0 or nrm.shape[0] != uv.shape[0] // 2 * 3:
            raise ValueError("indices (tri_count, 3), uv (n_vertices, 2) and normals (n_vertices, 3) are expected")
        t = MeshTopology(size=C.sizeof(MeshTopology), mesh=mesh, n_vertices=uv.shape[0] // 2, tri_count=idx.shape[0] // 3)
        t.indices = C.cast(idx.ctypes.data, C.POINTER(C.c_uint32))
        t.uv = C.cast(uv.ctypes.data, C.POINTER(C.c_float))
        t.normals = C.cast(nrm.ctypes.data, C.POINTER(C.c_float))
        if face_of_tri is not None:
            fot = np.ascontiguousarray(face_of_tri, dtype=np.uint32).reshape(-1)
            if fot.shape[0] != t.tri_count:
                raise ValueError("face_of_tri: one face per triangle is expected")
            t.face_of_tri = C.cast(fot.ctypes.data, C.POINTER(C.c_uint32))
        _check_hip(lib.spt_scene_mesh_topology(self._h, C.byref(t)))
        self._topology_nrm[mesh] = None   # (normals of the caller's: the next update() by vertices sends the Scene's)

    def read_triangles(self, mesh_index: int):
        """spt_scene_read_triangles: the (tri_pos, tri_attr) record arrays of mesh `mesh_index` as the device holds them, behind
        every update queued so far."""
        lib = hip_lib()
        if not hasattr(lib, "spt_scene_read_triangles"):
            raise SptError(4, "this libspt_hip.so has no spt_scene_read_triangles")
        first, count = self._mesh_ranges[mesh_index]
        tri_pos = np.zeros(count, dtype=np.dtype(TriPos))
        tri_attr = np.zeros(count, dtype=np.dtype(TriAttr))
        _check_hip(lib.spt_scene_read_triangles(self._h, first, count, tri_pos.ctypes.data, tri_attr.ctypes.data))
        return tri_pos, tri_attr

    def update_arrays(self, instances, lights, tlas_nodes=None, light_alias=None, meshes=None, vertices=None) -> None:
        """spt_scene_update for callers who edit the records themselves: `instances` / `lights` / `tlas_nodes` are arrays of the
        Instance / Light / BvhNode records (as Scene.array returns them; the instances in the leaf order of tlas_nodes),
        light_alias the (props, u, k) arrays of a power_is scene.  None: the Scene's current ones.  `meshes`: {mesh index:
        (tri_pos, tri_attr or None)} arrays of TriPos / TriAttr records for the mesh's whole range - then the call is
        spt_scene_deform.  `vertices`: {mesh index: (positions, normals or None)} for meshes registered with set_topology - then
        it is spt_scene_deform_vertices; giving both is a ValueError."""
        if meshes is not None and vertices is not None:
            raise ValueError("meshes= and vertices= exclude each other: one call deforms by records or by vertices")
        if vertices is not None and hasattr(host_lib(), "spt_host_scene_dynamic"):   # (the Scene's defaults without materialising it)
            d = SceneUpdateDesc()
            _check_host(host_lib().spt_host_scene_dynamic(self.scene._h, C.byref(d)))
        else:
            d = self.scene.desc
        keep = []

        def records(a, ty):
            a = np.ascontiguousarray(a, dtype=np.dtype(ty)).reshape(-1)
            keep.append(a)
            return a.shape[0], C.cast(a.ctypes.data, C.POINTER(ty))

        u = SceneUpdateDesc(size=C.sizeof(SceneUpdateDesc), flags=0)
        u.n_instances, u.instances = records(instances, Instance)
        u.n_lights, u.lights = records(lights, Light)
        if tlas_nodes is None:
            u.n_tlas_nodes, u.tlas_nodes = d.n_tlas_nodes, d.tlas_nodes
        else:
            u.n_tlas_nodes, u.tlas_nodes = records(tlas_nodes, BvhNode)
        if light_alias is None:
            u.light_alias = d.light_alias
        else:
            props, uu, k = light_alias
            n, u.light_alias.props = records(props, C.c_float)
            _, u.light_alias.u = records(uu, C.c_float)
            _, u.light_alias.k = records(k, C.c_uint32)
            u.light_alias.n = n
        if vertices is not None:
            lib = hip_lib()
            if not hasattr(lib, "spt_scene_deform_vertices"):
                raise SptError(4, "this libspt_hip.so has no spt_scene_deform_vertices")
            verts = (MeshVertices * max(len(vertices), 1))()
            for v, (m, (positions, normals)) in zip(verts, vertices.items()):
                pos = np.ascontiguousarray(positions, dtype=np.float32)
                if pos.ndim != 2 or pos.shape[1] != 3:
                    raise ValueError("mesh %d: an (n_vertices, 3) array of positions is expected" % m)
                keep.append(pos)
                v.mesh, v.n_vertices = m, pos.shape[0]
                v.positions = C.cast(pos.ctypes.data, C.POINTER(C.c_float))
                if normals is not None:
                    nrm = np.ascontiguousarray(normals, dtype=np.float32)
                    if nrm.shape != pos.shape:
                        raise ValueError("mesh %d: one normal per position is expected" % m)
                    keep.append(nrm)
                    v.normals = C.cast(nrm.ctypes.data, C.POINTER(C.c_float))
            _check_hip(lib.spt_scene_deform_vertices(self._h, C.byref(u), len(vertices), verts))
            return
        if meshes is None:
            self._update(u)
            return
        edits = (MeshDeform * max(len(meshes), 1))()
        for e, (m, (tri_pos, tri_attr)) in zip(edits, meshes.items()):
            e.mesh = m
            e.tri_count, e.tri_pos = records(tri_pos, TriPos)
            if tri_attr is not None:
                n_attr, e.tri_attr = records(tri_attr, TriAttr)
                if n_attr != e.tri_count:
                    raise ValueError("mesh %d: one tri_attr record per tri_pos record is expected" % m)
        self._deform(u, edits, len(meshes))

    def _update(self, u: "SceneUpdateDesc") -> None:
        lib = hip_lib()
        if not hasattr(lib, "spt_scene_update"):
            raise SptError(4, "this libspt_hip.so has no spt_scene_update")
        _check_hip(lib.spt_scene_update(self._h, C.byref(u)))

    def _deform(self, u: "SceneUpdateDesc", edits, n=None) -> None:
        lib = hip_lib()
        if not hasattr(lib, "spt_scene_deform"):
            raise SptError(4, "this libspt_hip.so has no spt_scene_deform")
        _check_hip(lib.spt_scene_deform(self._h, C.byref(u), len(edits) if n is None else n, edits))

    def render_info(self, what: int) -> int:
        """Test seam (spt_debug_render_info): 0 passes resolved on the film stream, 1 passes on the single-stream path;
        2 the ns the kernels of the last read-out of a sample-keeping film of the scene took on the device; 3 frames whose
        finish kernel stored the image into the (page-locked) output buffer itself, without the runtime's copy; 4 the
        spt_scene_update / spt_scene_deform calls applied to the scene; 5 the bytes the last of them copied to the device; 6 the
        ns the copies and kernels of the last spt_scene_deform that named a mesh took on the device (waits for them); 7 passes whose
        bounce launches ran on the second stream beside the next pass's camera rays (the pass pipeline; counted under 0 too); 8 passes whose camera rays came from
        the camera-model kernel (a camera_model=, or any render under SPT_CAMERA_GENERAL=1)."""
        v = C.c_uint64(0)
        _check_hip(hip_lib().spt_debug_render_info(self._h, what, C.byref(v)))
        return int(v.value)

    def origin_candidates(self):
        """spt_scene_origin_candidates: None when the scene's shade kernels do not take the per-origin-triangle candidate path (or
        SPT_NO_ORIGIN_CANDIDATES=1), else (words, info): words (n_rows, 4) uint64 as the device holds them - loose up, loose
        down, tight up, tight down per triangle index, bit k = slot k - and info, a dict with center, radius, reach, delta, tight
        and build_ns."""
        lib = hip_lib()
        if not hasattr(lib, "spt_scene_origin_candidates"):
            raise SptError(4, "this libspt_hip.so has no spt_scene_origin_candidates")
        words = np.zeros((64, 4), dtype=np.uint64)
        info = np.zeros(8, dtype=np.float64)
        n = C.c_uint32(0)
        _check_hip(lib.spt_scene_origin_candidates(self._h, words.ctypes.data, C.byref(n), info.ctypes.data))
        if n.value == 0:
            return None
        return words[:n.value].copy(), {"center": info[0:3].copy(), "radius": float(info[3]), "reach": float(info[4]), "delta": float(info[5]),
                                        "tight": bool(info[6]), "build_ns": int(info[7])}

    def close(self) -> None:
        # an asynchronous frame may still be copying into one of the pinned film buffers: the scene goes first (its destroy
        # drains the render and the copy stream), the buffers after it
        for film in list(self._films):
            film.close()
        if self._h:
            hip_lib().spt_render_wait(self._h)
            hip_lib().spt_scene_destroy(self._h)
            self._h = C.c_void_p()
        for ptr, _ in self._pinned.values():
            hip_lib().spt_free_pinned(ptr)
        self._pinned.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _camera_entry(name: str):
    """spt_render_camera / spt_film_create_camera of the device library; a library without camera models is an error."""
    fn = getattr(hip_lib(), name, None)
    if fn is None:
        raise SptError(4, "libspt_hip.so does not export %s (no camera models)" % name)
    return fn


def bake_rays(scene: "Scene", points, samples: int = 16, seed: int = 1, first_point: int = 0, first_sample: int = 0, world: bool = False,
              flip: bool = False):
    """spt_host_bake_rays: spt_bake's specification (include/spt_bake.h) evaluated on the host over the Scene's descriptor.  Returns
    a dict: "rays" (n, samples) PATH_RAY_DTYPE gather rays (radiance input), "pos" / "nrm" (n, 3) f32 the resolved points,
    "delta_rays" (n, n_lights) RAY_DTYPE shadow rays and "delta_li" (n, n_lights, 3) f32 per delta light (zeros where skipped).
    A bake is D + the in-order mean over k of DeviceScene.radiance(rays[:, k]), D the in-order sum of delta_li where
    DeviceScene.trace_any(delta_rays) finds nothing."""
    lib = host_lib()
    if not hasattr(lib, "spt_host_bake_rays"):
        raise SptError(4, "libspt_host.so does not export spt_host_bake_rays")
    points = np.ascontiguousarray(points, dtype=BAKE_WORLD_DTYPE if world else BAKE_POINT_DTYPE).reshape(-1)
    n, desc = points.shape[0], scene.desc
    nl = int(desc.n_lights)
    out = {"rays": np.zeros((n, samples), dtype=PATH_RAY_DTYPE), "pos": np.zeros((n, 3), dtype=np.float32), "nrm": np.zeros((n, 3), dtype=np.float32),
           "delta_rays": np.zeros((n, nl), dtype=RAY_DTYPE), "delta_li": np.zeros((n, nl, 3), dtype=np.float32)}
    _check_host(lib.spt_host_bake_rays(C.byref(desc), BAKE_POINTS_WORLD if world else BAKE_POINTS_SURFACE, BAKE_FLIP if flip else 0, n, points.ctypes.data,
                                       samples, seed, first_point & 0xffffffff, first_sample, out["rays"].ctypes.data, out["pos"].ctypes.data,
                                       out["nrm"].ctypes.data, out["delta_rays"].ctypes.data, out["delta_li"].ctypes.data))
    return out


def _probe_records(points) -> np.ndarray:
    """PROBE_DTYPE records from records or an (n, 3) float array."""
    if isinstance(points, np.ndarray) and points.dtype == PROBE_DTYPE:
        return np.ascontiguousarray(points).reshape(-1)
    xyz = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    out = np.zeros(xyz.shape[0], dtype=PROBE_DTYPE)
    out["p"] = xyz
    return out


def probe_rays(scene: "Scene", points, samples: int = 64, seed: int = 1, first_point: int = 0, first_sample: int = 0):
    """spt_host_probe_rays: spt_probe's specification (include/spt_probe.h) evaluated on the host over the Scene's lights.  Returns a
    dict: "rays" (n, samples) PATH_RAY_DTYPE gather rays (radiance input), "weights" (n, samples, 9) f32 the basis of each ray's
    direction, "delta_rays" (n, n_lights) RAY_DTYPE shadow rays, "delta_li" (n, n_lights, 3) and "delta_basis" (n, n_lights, 9) f32 per
    delta light (zeros where skipped).  A probe is D + w * the in-order sum over k of DeviceScene.radiance(rays[:, k]) * weights[:, k],
    w = 4 pi / samples, D the in-order sum of delta_li * delta_basis where DeviceScene.trace_any(delta_rays) finds nothing."""
    lib = host_lib()
    if not hasattr(lib, "spt_host_probe_rays"):
        raise SptError(4, "libspt_host.so does not export spt_host_probe_rays")
    points = _probe_records(points)
    n, desc = points.shape[0], scene.desc
    nl = int(desc.n_lights)
    out = {"rays": np.zeros((n, samples), dtype=PATH_RAY_DTYPE), "weights": np.zeros((n, samples, 9), dtype=np.float32),
           "delta_rays": np.zeros((n, nl), dtype=RAY_DTYPE), "delta_li": np.zeros((n, nl, 3), dtype=np.float32),
           "delta_basis": np.zeros((n, nl, 9), dtype=np.float32)}
    _check_host(lib.spt_host_probe_rays(nl, C.cast(desc.lights, C.c_void_p), n, points.ctypes.data, samples, seed, first_point & 0xffffffff, first_sample,
                                        out["rays"].ctypes.data, out["weights"].ctypes.data, out["delta_rays"].ctypes.data, out["delta_li"].ctypes.data,
                                        out["delta_basis"].ctypes.data))
    return out


def sh_basis(dirs) -> np.ndarray:
    """spt_host_probe_basis: the nine real SH of bands 0 .. 2 (no Condon-Shortley sign, j = l(l+1)+m) of directions (..., 3), in f32
    exactly as spt_probe evaluates them: (..., 9)."""
    lib = host_lib()
    if not hasattr(lib, "spt_host_probe_basis"):
        raise SptError(4, "libspt_host.so does not export spt_host_probe_basis")
    dirs = np.ascontiguousarray(dirs, dtype=np.float32)
    out = np.zeros(dirs.shape[:-1] + (9,), dtype=np.float32)
    _check_host(lib.spt_host_probe_basis(dirs.size // 3, dirs.ctypes.data, out.ctypes.data))
    return out


_SH_CONST = (0.282094792, 0.488602512, 1.092548431, 0.315391565, 0.546274215)


def sh_irradiance(coeffs, normals) -> np.ndarray:
    """Irradiance from probe coefficients, in float64: the convolution with the clamped cosine lobe, A = pi, 2 pi / 3, pi / 4 per
    band.  coeffs (..., 9, 3), normals (..., 3) unit vectors, broadcast against each other; returns (..., 3).  A constant radiance L
    (coeffs[0] = L / Y0, the rest 0) gives pi * L for every normal."""
    c = np.asarray(coeffs, dtype=np.float64)
    n = np.asarray(normals, dtype=np.float64)
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    k0, k1, k2, k3, k4 = _SH_CONST
    Y = np.stack([np.full_like(x, k0), k1 * y, k1 * z, k1 * x, k2 * (x * y), k2 * (y * z), k3 * (3.0 * (z * z) - 1.0), k2 * (x * z), k4 * (x * x - y * y)], axis=-1)
    A = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)
    return np.sum((Y * A)[..., None] * c, axis=-2)


def vertex_points(scene: "Scene", name: str) -> np.ndarray:
    """One bake point per triangle corner of the mesh instance `name`, (tri_count, 3) BAKE_POINT_DTYPE: corner c of a triangle has
    (v, w) = (0, 0), (1, 0), (0, 1).  Per-vertex lighting is a bake over these, averaged over the corners that share a vertex."""
    inst = scene.instance_index(name)
    d = scene.desc
    rec = d.instances[inst]
    if rec.prim_type != 1:
        raise ValueError("%s is not a triangle-mesh instance" % name)
    mesh = d.meshes[rec.prim_id]
    pts = np.zeros((int(mesh.tri_count), 3), dtype=BAKE_POINT_DTYPE)
    pts["instance"] = inst
    pts["prim"] = (int(mesh.tri_first) + np.arange(int(mesh.tri_count), dtype=np.uint32))[:, None]
    pts["v"] = np.array([0.0, 1.0, 0.0], dtype=np.float32)[None, :]
    pts["w"] = np.array([0.0, 0.0, 1.0], dtype=np.float32)[None, :]
    return pts


def camera_rays(model: "CameraModel", renderer: "PathTracer", width: int, height: int, first: int = 0, count: Optional[int] = None,
                aux: bool = False):
    """spt_host_camera_rays: the rays of a camera model for the samples [first, first + count) of the renderer's plan, as
    (count, height, width) PATH_RAY_DTYPE records with streams (pixel, plan index); aux=True: (rays, aux) with their auxiliary rays
    as RAY_AUX_DTYPE.  rays == radiance input: DeviceScene.radiance(rays, aux, max_depth=, seed=, rng_skip=2 (recurrence: 0))
    returns the samples a film of the model holds.  Made on the host from the header the device kernel includes."""
    lib = host_lib()
    if not hasattr(lib, "spt_host_camera_rays"):
        raise SptError(4, "libspt_host.so does not export spt_host_camera_rays")
    if count is None:
        count = renderer.spp - first
    p = renderer.params(width, height)
    rays = np.zeros((count, height, width), dtype=PATH_RAY_DTYPE)
    ax = np.zeros((count, height, width), dtype=RAY_AUX_DTYPE) if aux else None
    _check_host(lib.spt_host_camera_rays(C.byref(model), C.byref(p), first, count, rays.ctypes.data, ax.ctypes.data if aux else None))
    return (rays, ax) if aux else rays


def camera_gbuffer(scene, model: "CameraModel", renderer: "PathTracer", width: int, height: int, samples: int = 1, device: int = 0,
                   host_rays: bool = False) -> dict:
    """First-hit images of a camera model for the plan samples k = 0 .. samples - 1.  `scene` is a Scene (its device scene on
    `device` serves the call) or a DeviceScene.  Returns float32 images: "albedo" and "normal" (height, width, 3), the sums in
    sample order (a miss adds 0) times 1 / samples; "depth" (height, width), the sum of t over the hit samples divided by their
    count, 0 without one; "coverage" (height, width), hits / samples.
    One spt_camera_gbuffer call (DeviceScene.camera_gbuffer) when the library exports it.  Otherwise, and with host_rays=True, the
    route it replaces, which gives the same words: camera_rays(model, renderer, width, height, k, 1, aux=True) through
    DeviceScene.gbuffer, one sample at a time, summed on the host."""
    if samples < 1:
        raise ValueError("samples must be >= 1")
    ds = scene if isinstance(scene, DeviceScene) else scene.device_scene(device)
    if not host_rays and hasattr(hip_lib(), "spt_camera_gbuffer"):
        return ds.camera_gbuffer(model, renderer, width, height, samples)
    albedo = np.zeros((height, width, 3), dtype=np.float32)
    normal = np.zeros((height, width, 3), dtype=np.float32)
    t_sum = np.zeros((height, width), dtype=np.float32)
    hits = np.zeros((height, width), dtype=np.float32)
    for k in range(samples):
        rays, aux = camera_rays(model, renderer, width, height, k, 1, aux=True)
        rec = ds.gbuffer(rays, aux).reshape(height, width)
        hit = rec["instance"] >= 0
        albedo += rec["albedo"]
        normal += rec["n"]
        t_sum += np.where(hit, rec["t"], np.float32(0.0))
        hits += hit.astype(np.float32)
    inv = np.float32(1.0) / np.float32(samples)
    depth = np.where(hits > 0, t_sum / np.maximum(hits, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
    return {"albedo": albedo * inv, "normal": normal * inv, "depth": depth, "coverage": hits / np.float32(samples)}


@dataclass
class OutputConfig:
    """reference src/renderer/mod.rs:9-14"""
    width: int = 512
    height: int = 512
    output_filename: Optional[str] = None
    used_camera_name: Optional[str] = None


def shard_rows(height: int, shard_index: int, shard_count: int, strip_rows: int) -> np.ndarray:
    """Image rows (top = 0) rendered by one shard: interleaved strips of `strip_rows` rows."""
    j = np.arange(height)
    return j[(j // strip_rows) % shard_count == shard_index]


class PathTracer:
    """reference PathTracer{max_depth, pixel_sampler, filter} (src/renderer/pt.rs:24-37)."""

    def __init__(self, max_depth: int = 8, sampler: int = SAMPLER_RECURRENCE, spp: int = 256,
                 division_x: int = 0, division_y: int = 0, filter_radius: float = 0.5, seed: int = 1, debug_normal: bool = False,
                 aov_albedo: bool = False, filter_type: str = "box", filter_params: Optional[dict] = None):
        self.max_depth = max_depth
        self.sampler = sampler
        self.spp = spp
        self.division_x = division_x
        self.division_y = division_y
        self.filter_radius = filter_radius
        # the reconstruction filter: "box" (the reference's, at filter_radius) or a weighted one of spt_film_filter ("tent",
        # "gaussian", "mitchell") with support radius filter_radius and filter_params (alpha / b, c).  A weighted filter is served
        # by films that keep their samples: progressive(keep_samples=True) and render_shard
        if filter_type not in FILTER_TYPES:
            raise ValueError("PathTracer: filter_type is one of %s, not %r" % (", ".join(repr(k) for k in FILTER_TYPES), filter_type))
        self.filter_type = filter_type
        self.filter_params = dict(filter_params or {})
        self.seed = seed
        self.debug_normal = debug_normal   # a build of the reference with `--features debug_normal`: colour = normal * 0.5 + 0.5
        self.aov_albedo = aov_albedo       # RENDER_AOV_ALBEDO: colour = the albedo of the first surface (not together with debug_normal)
        self.last_stats: Optional[RenderStats] = None

    def params(self, width: int, height: int, shard_index: int = 0, shard_count: int = 1, strip_rows: int = 16,
               samples_per_pass: int = 0, flags: int = 0) -> RenderParams:
        """The plan of a shard.  It carries filter_radius only: a weighted filter_type is no field of spt_render_params, it is
        applied by spt_film_filter to a sample-keeping film of this plan, so whoever hands the plan to spt_render refuses a
        weighted filter first (render_shard goes through such a film, MultiDevice.render raises)."""
        p = RenderParams()
        p.width, p.height, p.spp, p.max_depth = width, height, self.spp, self.max_depth
        p.sampler, p.division_x, p.division_y = self.sampler, self.division_x, self.division_y
        p.seed = self.seed
        p.shard_index, p.shard_count, p.strip_rows = shard_index, shard_count, strip_rows
        p.samples_per_pass, p.flags = samples_per_pass, flags | (RENDER_DEBUG_NORMAL if self.debug_normal else 0) | (RENDER_AOV_ALBEDO if self.aov_albedo else 0)
        p.stats_size = C.sizeof(RenderStats)
        if self.filter_radius != 0.5:
            # BoxFilter of any radius (src/filter/boxf.rs): Film::filter_pixel sums the UNWEIGHTED colours of the
            # (2 ceil(radius - 0.5) + 1)^2 pixels around a pixel and divides by the number of those samples whose
            # offset lies within the radius (reference quirk Q1, src/core/film.rs:82-91); 0.5 is the plain mean
            p.flags |= RENDER_BOX_RADIUS
            p.filter_radius = self.filter_radius
        return p

    def render_shard(self, scene: Scene, config: OutputConfig, device: int = 0, shard_index: int = 0,
                     shard_count: int = 1, strip_rows: int = 16, samples_per_pass: int = 0,
                     profile: bool = False, reuse_output: bool = False, film: Optional[np.ndarray] = None,
                     count_visits: bool = False, wait: bool = True, camera_model: Optional["CameraModel"] = None) -> np.ndarray:
        """Mean radiance of this shard's rows, shape (rows, width, 3) f32, via the HIP path.
        reuse_output=True returns a page-locked buffer owned by the device scene that the next call
        with the same shape overwrites (no per-call allocation, DMA-speed copy-out).
        count_visits=True runs the counting instantiations of the traversal kernels (last_stats.node_visits, ...).
        wait=False (SPT_RENDER_ASYNC): returns once the work is queued; the returned buffer is valid after `self.wait(scene)`
        or after a later wait=True call on the scene; no stats (last_stats keeps the previous synchronous call's).
        With a weighted filter_type the shard is rendered through a sample-keeping film (one increment, one read-out): film=,
        wait=False, profile and count_visits are refused (SptError), reuse_output is ignored (the result is a fresh array, not
        the scene's pinned buffer) and last_stats is left as it was.
        camera_model: a CameraModel in the place of the scene's camera (spt_render_camera)."""
        if self.filter_type != "box":
            # a weighted filter reads kept samples: one sample-keeping film, one increment, one read-out
            if film is not None or not wait or profile or count_visits:
                raise SptError(2, "render_shard: a %s filter renders through a sample-keeping film, which takes no film=, wait=False, "
                                  "profile or count_visits" % self.filter_type)
            with self.progressive(scene, config, device, 0, False, shard_index, shard_count, strip_rows, samples_per_pass, keep_samples=True,
                                  camera_model=camera_model) as pf:
                return pf.render(self.spp).mean()
        ds = scene.device_scene(device)
        cam = scene.get_camera(config.used_camera_name)
        p = self.params(config.width, config.height, shard_index, shard_count, strip_rows, samples_per_pass,
                        (RENDER_PROFILE if profile else 0) | (RENDER_COUNT_VISITS if count_visits else 0) | (0 if wait else RENDER_ASYNC))
        rows = C.c_uint32()
        _check_hip(hip_lib().spt_shard_rows(C.byref(p), C.byref(rows)))

        def call(dst, stats_ref):
            if camera_model is None:
                return hip_lib().spt_render(ds._h, C.byref(cam), C.byref(p), dst, stats_ref)
            return _camera_entry("spt_render_camera")(ds._h, C.byref(camera_model), C.byref(p), dst, stats_ref)

        if film is not None:
            # write this shard's strips in place into a full-image (height, width, 3) f32 film (e.g. SharedFilm.film)
            assert film.shape == (config.height, config.width, 3) and film.dtype == np.float32 and film.flags["C_CONTIGUOUS"]
            row_bytes = config.width * 12
            p.out_strip_stride = shard_count * strip_rows * row_bytes
            stats = RenderStats()
            first = film.ctypes.data + shard_index * strip_rows * row_bytes
            _check_hip(call(first if rows.value else film.ctypes.data, C.byref(stats) if wait else None))
            if wait:
                self.last_stats = stats
            return film
        if reuse_output and rows.value:
            out = ds.film_buffer(rows.value, config.width)
        else:
            if not wait and rows.value:
                # a fresh pageable array would be the target of a copy that is still queued when this call returns, with
                # nothing keeping it alive until wait(): the asynchronous form needs a buffer that outlives the call
                # (a shard without rows - more shards than strips - copies nothing: the empty array below is fine)
                raise SptError(1, "render_shard(wait=False) needs reuse_output=True (the scene's pinned buffer) or a caller-owned film=")
            out = np.zeros((rows.value, config.width, 3), dtype=np.float32)
        stats = RenderStats()
        _check_hip(call(out.ctypes.data, C.byref(stats) if wait else None))
        if wait:
            self.last_stats = stats
        return out

    def progressive(self, scene: Scene, config: OutputConfig, device: int = 0, first_sample: int = 0, moments: bool = False,
                    shard_index: int = 0, shard_count: int = 1, strip_rows: int = 16, samples_per_pass: int = 0,
                    flags: int = 0, keep_samples: bool = False, camera_model: Optional["CameraModel"] = None,
                    buckets: int = 0) -> "ProgressiveFilm":
        """A film that takes this renderer's samples in increments (spt_film_*): `spp` is the plan's total, each
        ProgressiveFilm.render(n) adds the next n samples, and after increments summing to spp (first_sample 0) mean() has the
        bits of render_shard with the same arguments.  moments=True also keeps the sums of squares (sum_sq, variance_of_mean).
        `flags` are extra SPT_RENDER_* bits of the plan.  buckets=K (odd, 3 .. 15) also keeps K bucket sums per pixel (sample s of
        the plan goes to bucket s % K) for bucket_sums() and robust_mean().  keep_samples=True keeps every sample's radiance
        instead of running sums (FILM_KEEP_SAMPLES): the film then takes a box radius that reaches neighbouring pixels, kept()
        returns the samples, and moments, buckets, adapt and denoise are refused.  Such a film is read under this renderer's
        filter_type (ProgressiveFilm.set_filter changes it later); without keep_samples a weighted filter is refused.
        camera_model: a CameraModel in the place of the scene's camera (spt_film_create_camera); the film remembers it."""
        return ProgressiveFilm(self, scene, config, device, first_sample, moments, shard_index, shard_count, strip_rows,
                               samples_per_pass, flags, keep_samples=keep_samples, buckets=buckets, camera_model=camera_model)

    def guide_film(self, scene: Scene, config: OutputConfig, device: int = 0) -> "ProgressiveFilm":
        """The guide of ProgressiveFilm.denoise: a film of the same plan with debug_normal (its mean is the first-hit normal
        * 0.5 + 0.5) and moments (its variance tells the filter how far to trust it).  Render a few samples into it."""
        return ProgressiveFilm(self, scene, config, device, moments=True, flags=RENDER_DEBUG_NORMAL)

    def albedo_film(self, scene: Scene, config: OutputConfig, device: int = 0) -> "ProgressiveFilm":
        """The albedo film of ProgressiveFilm.denoise_job: a film of the same plan with RENDER_AOV_ALBEDO (its mean is the
        first-hit albedo) and moments.  Render a few samples into it."""
        return ProgressiveFilm(self, scene, config, device, moments=True, flags=RENDER_AOV_ALBEDO)

    def wait(self, scene: Scene, device: int = 0) -> None:
        """spt_render_wait: every render_shard(..., wait=False) queued on the scene has delivered its film."""
        _check_hip(hip_lib().spt_render_wait(scene.device_scene(device)._h))

    def render(self, scene: Scene, config: OutputConfig, device: int = 0, camera_model: Optional["CameraModel"] = None) -> np.ndarray:
        """RendererT::render (src/renderer/pt.rs:237-296): full image on one GPU; writes the PNG
        when config.output_filename is set and returns the float film (H, W, 3).  camera_model: see render_shard."""
        film = self.render_shard(scene, config, device, camera_model=camera_model)
        if config.output_filename:
            write_image(config.output_filename, film)
        return film


class ProgressiveFilm:
    """One shard's running sums of a fixed render plan on the device (spt_film_create); see PathTracer.progressive.
    Keeps its DeviceScene alive; closing the scene closes the film first."""

    def __init__(self, renderer: PathTracer, scene: Scene, config: OutputConfig, device: int = 0, first_sample: int = 0,
                 moments: bool = False, shard_index: int = 0, shard_count: int = 1, strip_rows: int = 16,
                 samples_per_pass: int = 0, flags: int = 0, keep_samples: bool = False, camera_model: Optional["CameraModel"] = None,
                 buckets: int = 0):
        self._h = C.c_void_p()
        # tests/test_robust_abi.py pins `buckets` as the last parameter here and in PathTracer.progressive, so camera_model sits before it:
        # a bucket count passed by position lands in camera_model and is named as what it is, before anything is created
        if camera_model is not None and not isinstance(camera_model, CameraModel):
            raise TypeError("camera_model takes a CameraModel, not %r; pass buckets= by keyword" % (camera_model,))
        if renderer.filter_type != "box" and not keep_samples:
            raise SptError(1, "a %s filter needs a film that keeps its samples (keep_samples=True)" % renderer.filter_type)
        self._ds = scene.device_scene(device)
        self.scene = scene
        self.first_sample = first_sample
        self.width = config.width
        self._cam = scene.get_camera(config.used_camera_name)
        self._params = renderer.params(config.width, config.height, shard_index, shard_count, strip_rows, samples_per_pass, flags)
        rows = C.c_uint32()
        _check_hip(hip_lib().spt_shard_rows(C.byref(self._params), C.byref(rows)))
        self.rows = rows.value
        film_flags = (FILM_MOMENTS if moments else 0) | (FILM_KEEP_SAMPLES if keep_samples else 0)
        if camera_model is None:
            _check_hip(hip_lib().spt_film_create(self._ds._h, C.byref(self._cam), C.byref(self._params), first_sample, film_flags, C.byref(self._h)))
        else:
            _check_hip(_camera_entry("spt_film_create_camera")(self._ds._h, C.byref(camera_model), C.byref(self._params), first_sample, film_flags,
                                                               C.byref(self._h)))
        self._ds._films.add(self)
        self.n_buckets = 0
        if buckets:
            self.set_buckets(buckets)
        if renderer.filter_type != "box":
            try:
                self.set_filter(renderer.filter_type, radius=renderer.filter_radius, **renderer.filter_params)
            except Exception:
                self.close()
                raise

    def set_filter(self, kind: str, radius: Optional[float] = None, alpha: float = 2.0, b: float = 1.0 / 3.0, c: float = 1.0 / 3.0) -> None:
        """spt_film_filter: the reconstruction filter of later mean(), sum() and read_rgb8("mean") calls of a keep_samples=True
        film: "tent" and "gaussian" (alpha) of support `radius`, "mitchell" (b, c; radius 2 by default), or "box", which
        restores the reference's box at the plan's radius.  Nothing is traced again; the radius may not reach past the halo rows
        the plan's filter_radius made the film store (SptError, and the film keeps its filter)."""
        lib = hip_lib()
        if not hasattr(lib, "spt_film_filter"):
            raise SptError(2, "libspt_hip.so does not export spt_film_filter")
        desc = filter_desc(kind, radius, alpha, b, c)
        _check_hip(lib.spt_film_filter(self._handle(), C.byref(desc)))

    def set_buckets(self, n_buckets: int) -> None:
        """spt_film_buckets: K = n_buckets bucket sums per pixel (K odd, 3 .. 15) from the film's first sample on.  What the
        `buckets=` keyword calls after the film is created; public for a caller that decides after creating the film, which
        works until the first render and once (SptError otherwise, and for a box radius other than 0.5; the film stays usable)."""
        _check_hip(hip_lib().spt_film_buckets(self._handle(), n_buckets))
        self.n_buckets = n_buckets

    def bucket_sums(self) -> np.ndarray:
        """(K, rows, width, 3) f32: B_j, the sum of the covered samples whose plan index s has s % K == j, in sample order."""
        out = np.zeros((self.n_buckets, self.rows, self.width, 3), dtype=np.float32)
        _check_hip(hip_lib().spt_film_read_buckets(self._handle(), out.ctypes.data))
        return out

    def robust_mean(self, estimator: str = "gmon") -> np.ndarray:
        """spt_film_read_robust: "mon", the median of the K bucket means, or "gmon", their mean without the t lowest and t highest,
        t growing with their Gini coefficient (the plain mean of the bucket means where they agree, the median where they do
        not).  A sample that is not finite spoils one bucket, not the pixel.  (rows, width, 3) f32."""
        if estimator not in ("mon", "gmon"):
            raise ValueError("robust_mean: estimator is 'mon' or 'gmon', not %r" % (estimator,))
        out = np.zeros((self.rows, self.width, 3), dtype=np.float32)
        _check_hip(hip_lib().spt_film_read_robust(self._handle(), ROBUST_MON if estimator == "mon" else ROBUST_GMON, out.ctypes.data))
        return out

    def read_rgb8(self, source: str = "mean", guide: Optional["ProgressiveFilm"] = None, **denoise_params) -> np.ndarray:
        """spt_film_read_rgb8: film_to_rgb8 of mean() ("mean"), robust_mean("mon" / "gmon") or denoise(guide, **denoise_params)
        ("denoised"), converted on the device: (rows, width, 3) u8, a quarter of the bytes of the float read-out.  Refused
        where the float call is; the film is not changed."""
        if source not in READ_SOURCES:
            raise ValueError("read_rgb8: source is one of %s, not %r" % (", ".join(repr(k) for k in READ_SOURCES), source))
        if source != "denoised" and (guide is not None or denoise_params):
            raise ValueError("read_rgb8: guide and the denoiser's parameters go with source='denoised'")
        params = None
        if source == "denoised":
            d = dict(iterations=5, k_color=2.0, k_guide=1.0, eps_color=1e-8, eps_guide=1e-2)
            unknown = set(denoise_params) - set(d)
            if unknown:
                raise TypeError("read_rgb8: unknown denoise parameter(s) %s" % ", ".join(sorted(unknown)))
            d.update(denoise_params)
            params = C.byref(DenoiseParams(C.sizeof(DenoiseParams), d["iterations"], d["k_color"], d["k_guide"], d["eps_color"], d["eps_guide"]))
        out = np.zeros((self.rows, self.width, 3), dtype=np.uint8)
        _check_hip(hip_lib().spt_film_read_rgb8(self._handle(), READ_SOURCES[source], guide._handle() if guide is not None else None,
                                                params, out.ctypes.data))
        return out

    def kept(self, first: Optional[int] = None, count: Optional[int] = None) -> np.ndarray:
        """spt_film_read_samples of a keep_samples=True film: (count, rows, width, 3) f32, the radiance of the samples with plan
        index first .. first + count - 1 on the own rows; by default everything the film covers."""
        if first is None:
            first = self.first_sample
        if count is None:
            count = self.first_sample + self.samples - first
        out = np.zeros((max(count, 0), self.rows, self.width, 3), dtype=np.float32)
        spare = np.zeros(1, dtype=np.float32)   # (an empty result: the call still wants a pointer, and checks its range)
        _check_hip(hip_lib().spt_film_read_samples(self._handle(), first, count, out.ctypes.data if out.size else spare.ctypes.data))
        return out

    def render(self, n: int) -> "ProgressiveFilm":
        """Adds the next n samples of the plan (synchronous)."""
        _check_hip(hip_lib().spt_film_render(self._handle(), n))
        return self

    @property
    def samples(self) -> int:
        """Samples covered so far: the plan's [first_sample, first_sample + samples)."""
        done = C.c_uint32()
        _check_hip(hip_lib().spt_film_samples(self._handle(), C.byref(done)))
        return done.value

    def read(self, what: int) -> np.ndarray:
        """(rows, width, 3) f32 of one FILM_* quantity."""
        out = np.zeros((self.rows, self.width, 3), dtype=np.float32)
        _check_hip(hip_lib().spt_film_read(self._handle(), what, out.ctypes.data))
        return out

    def mean(self) -> np.ndarray:
        return self.read(FILM_MEAN)

    def sum(self) -> np.ndarray:
        return self.read(FILM_SUM)

    def sum_sq(self) -> np.ndarray:
        return self.read(FILM_SUM_SQ)

    def variance_of_mean(self) -> np.ndarray:
        return self.read(FILM_VAR_OF_MEAN)

    def adapt(self, rel_error: float, abs_floor: float = 0.0, min_samples: int = 16) -> int:
        """spt_film_adapt: retires every active pixel whose variance of the mean v meets v <= (rel_error * |mean| + abs_floor)^2
        in all three channels, once the film covers max(min_samples, 2) samples; later render() calls trace only the active
        pixels.  Needs moments=True.  Returns the pixels still active."""
        active = C.c_uint32()
        _check_hip(hip_lib().spt_film_adapt(self._handle(), rel_error, abs_floor, min_samples, C.byref(active)))
        return active.value

    def sample_counts(self) -> np.ndarray:
        """(rows, width) u32: the samples each pixel covers (`samples` while it is active; mean() and variance_of_mean()
        follow these counts)."""
        out = np.zeros((self.rows, self.width), dtype=np.uint32)
        _check_hip(hip_lib().spt_film_read_counts(self._handle(), out.ctypes.data))
        return out

    def denoise(self, guide: Optional["ProgressiveFilm"] = None, iterations: int = 5, k_color: float = 2.0, k_guide: float = 1.0,
                eps_color: float = 1e-8, eps_guide: float = 1e-2) -> np.ndarray:
        """spt_film_denoise: the film's mean after `iterations` steps of an edge-aware 5x5 a-trous filter whose weights compare
        luminance differences with the variance of the mean and, with a `guide` film (PathTracer.guide_film), the guide's
        differences with its variance.  Needs moments=True and 2 samples on both films; changes neither.  (rows, width, 3) f32."""
        out = np.zeros((self.rows, self.width, 3), dtype=np.float32)
        params = DenoiseParams(C.sizeof(DenoiseParams), iterations, k_color, k_guide, eps_color, eps_guide)
        _check_hip(hip_lib().spt_film_denoise(self._handle(), guide._handle() if guide is not None else None, C.byref(params),
                                              out.ctypes.data))
        return out

    def denoise_job(self, guide: Optional["ProgressiveFilm"] = None, albedo: Optional["ProgressiveFilm"] = None, demodulate: bool = False,
                    rgb8: bool = False, **params) -> np.ndarray:
        """spt_film_denoise_job: denoise() with a second guide, an `albedo` film (PathTracer.albedo_film), and - demodulate - the
        filter run on mean / albedo with the albedo multiplied back, which keeps texture detail.  `params` are denoise()'s
        keywords plus k_albedo, eps_albedo (the albedo term) and eps_demod (the floor of the divisor).  Without albedo and
        demodulate it returns the bits of denoise(guide, ...).  (rows, width, 3) f32, or u8 with rgb8 (the conversion of read_rgb8)."""
        d = dict(iterations=5, k_color=2.0, k_guide=1.0, eps_color=1e-8, eps_guide=1e-2, k_albedo=1.0, eps_albedo=1e-2, eps_demod=1e-2)
        unknown = set(params) - set(d)
        if unknown:
            raise TypeError("denoise_job: unknown parameter(s) %s" % ", ".join(sorted(unknown)))
        d.update(params)
        dp = DenoiseParams(C.sizeof(DenoiseParams), d["iterations"], d["k_color"], d["k_guide"], d["eps_color"], d["eps_guide"])
        job = DenoiseJob(C.sizeof(DenoiseJob), (DENOISE_DEMODULATE if demodulate else 0) | (DENOISE_OUT_RGB8 if rgb8 else 0),
                         guide._handle() if guide is not None else None, albedo._handle() if albedo is not None else None, C.pointer(dp),
                         d["k_albedo"], d["eps_albedo"], d["eps_demod"], 0)
        out = np.zeros((self.rows, self.width, 3), dtype=np.uint8 if rgb8 else np.float32)
        _check_hip(hip_lib().spt_film_denoise_job(self._handle(), C.byref(job), out.ctypes.data))
        return out

    def _handle(self):
        if not self._h:
            raise SptError(1, "the progressive film is closed")
        return self._h

    def close(self) -> None:
        if self._h:
            hip_lib().spt_film_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self) -> "ProgressiveFilm":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceApi(C.Structure):
    """spt_device_api (include/spt_host.h): the device entry points the multi-device fan-out drives."""
    _fields_ = [("scene_create", C.c_void_p), ("scene_destroy", C.c_void_p), ("render", C.c_void_p), ("last_error", C.c_void_p),
                ("pin_host", C.c_void_p), ("unpin_host", C.c_void_p)]


def hip_device_api() -> DeviceApi:
    """The table filled with libspt_hip.so's own functions."""
    lib = hip_lib()
    addr = lambda f: C.cast(f, C.c_void_p).value
    return DeviceApi(addr(lib.spt_scene_create), addr(lib.spt_scene_destroy), addr(lib.spt_render), addr(lib.spt_last_error),
                     addr(lib.spt_pin_host), addr(lib.spt_unpin_host))


class DeviceFilmApi(C.Structure):
    """spt_device_film_api (include/spt_host.h): the film entry points a multi film drives; `size` is sizeof of the table."""
    _fields_ = [("size", C.c_uint32), ("pad", C.c_uint32), ("film_create", C.c_void_p), ("film_destroy", C.c_void_p),
                ("film_render", C.c_void_p), ("film_samples", C.c_void_p), ("film_read", C.c_void_p), ("film_read_counts", C.c_void_p),
                ("film_adapt", C.c_void_p), ("film_buckets", C.c_void_p), ("film_read_robust", C.c_void_p), ("film_read_rgb8", C.c_void_p),
                ("denoise_image", C.c_void_p), ("last_error", C.c_void_p)]


def hip_device_film_api() -> DeviceFilmApi:
    """The film table filled with libspt_hip.so's own functions.  An entry point an older library lacks (they are additive to ABI
    v14) stays NULL: the multi call that needs it then returns SPT_ERR_UNSUPPORTED."""
    lib = hip_lib()
    addr = lambda name: C.cast(getattr(lib, name), C.c_void_p).value if hasattr(lib, name) else None
    return DeviceFilmApi(C.sizeof(DeviceFilmApi), 0, addr("spt_film_create"), addr("spt_film_destroy"), addr("spt_film_render"),
                         addr("spt_film_samples"), addr("spt_film_read"), addr("spt_film_read_counts"), addr("spt_film_adapt"),
                         addr("spt_film_buckets"), addr("spt_film_read_robust"), addr("spt_film_read_rgb8"),
                         addr("spt_denoise_image"), addr("spt_last_error"))


_DENOISE_DEFAULTS = dict(iterations=5, k_color=2.0, k_guide=1.0, eps_color=1e-8, eps_guide=1e-2, k_albedo=1.0, eps_albedo=1e-2, eps_demod=1e-2)


def _denoise_keywords(who: str, params: dict) -> dict:
    unknown = set(params) - set(_DENOISE_DEFAULTS)
    if unknown:
        raise TypeError("%s: unknown parameter(s) %s" % (who, ", ".join(sorted(unknown))))
    d = dict(_DENOISE_DEFAULTS)
    d.update(params)
    return d


def denoise_image(scene, mean: np.ndarray, var: np.ndarray, guide=None, albedo=None, demodulate: bool = False, rgb8: bool = False,
                  **params) -> np.ndarray:
    """spt_denoise_image: the filter of ProgressiveFilm.denoise_job on images instead of films.  `scene` (a Scene, whose device 0
    replica is used, or a DeviceScene) names the device; `mean` / `var` are (rows, width, 3) f32 as mean() / variance_of_mean()
    return them, `guide` and `albedo` (mean, var) pairs of the same shape.  The result has the bits of denoise_job on films with
    those read-outs: (rows, width, 3) f32, or u8 with rgb8."""
    ds = scene.device_scene(0) if isinstance(scene, Scene) else scene
    d = _denoise_keywords("denoise_image", params)
    mean = np.ascontiguousarray(mean, dtype=np.float32)
    if mean.ndim != 3 or mean.shape[2] != 3:
        raise ValueError("denoise_image: mean must have the shape (rows, width, 3)")
    keep = [mean]

    def arr(a, what):
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.shape != mean.shape:
            raise ValueError("denoise_image: %s has the shape %r, the mean %r" % (what, a.shape, mean.shape))
        keep.append(a)
        return a.ctypes.data if a.size else keep[0].ctypes.data

    dp = DenoiseParams(C.sizeof(DenoiseParams), d["iterations"], d["k_color"], d["k_guide"], d["eps_color"], d["eps_guide"])
    job = ImageDenoiseJob(C.sizeof(ImageDenoiseJob), (DENOISE_DEMODULATE if demodulate else 0) | (DENOISE_OUT_RGB8 if rgb8 else 0),
                          mean.shape[1], mean.shape[0], arr(mean, "mean"), arr(var, "var"),
                          arr(guide[0], "guide mean") if guide is not None else None, arr(guide[1], "guide var") if guide is not None else None,
                          arr(albedo[0], "albedo mean") if albedo is not None else None, arr(albedo[1], "albedo var") if albedo is not None else None,
                          C.pointer(dp), d["k_albedo"], d["eps_albedo"], d["eps_demod"], 0)
    out = np.zeros(mean.shape, dtype=np.uint8 if rgb8 else np.float32)
    _check_hip(hip_lib().spt_denoise_image(ds._h, C.byref(job), out.ctypes.data if out.size else keep[0].ctypes.data))
    return out


class MultiFilm:
    """A progressive film over the replicas of a MultiDevice (spt_host_multi_film_*): one shard film per replica, driven as one;
    see MultiDevice.progressive.  The methods are ProgressiveFilm's and every read-out is the FULL image, with the bits of the
    single-device film of the same plan."""

    def __init__(self, multi: "MultiDevice", renderer: "PathTracer", config: OutputConfig, strip_rows: int = 0, first_sample: int = 0,
                 moments: bool = False, flags: int = 0, buckets: int = 0, film_api: Optional[DeviceFilmApi] = None,
                 keep_samples: bool = False, camera_model: Optional["CameraModel"] = None):
        self._h = C.c_void_p()
        if camera_model is not None:   # (the multi-device host layer copies a bare spt_camera)
            raise SptError(4, "MultiFilm: films over several devices take the scene's pinhole camera only, no camera_model")
        self.multi = multi
        self.first_sample = first_sample
        self.width, self.height = config.width, config.height
        self.n_buckets = buckets
        self._api = film_api if film_api is not None else hip_device_film_api()
        if renderer.filter_type != "box":   # (spt_device_film_api has no entry for spt_film_filter)
            raise SptError(2, "films over several devices are read under the box filter only, not %r" % (renderer.filter_type,))
        cam = multi.scene.get_camera(config.used_camera_name)
        p = renderer.params(config.width, config.height, 0, 1, 16, 0, flags)
        _check_host(host_lib().spt_host_multi_film_create(multi._h, C.byref(self._api), C.byref(cam), C.byref(p), strip_rows, first_sample,
                                                          (FILM_MOMENTS if moments else 0) | (FILM_KEEP_SAMPLES if keep_samples else 0), buckets,
                                                          C.byref(self._h)))
        multi._films.add(self)

    def _handle(self):
        if not self._h:
            raise SptError(1, "the multi film is closed")
        return self._h

    def render(self, n: int) -> "MultiFilm":
        """Adds the next n samples of the plan to every shard (synchronous)."""
        _check_host(host_lib().spt_host_multi_film_render(self._handle(), n))
        return self

    @property
    def samples(self) -> int:
        done = C.c_uint32()
        _check_host(host_lib().spt_host_multi_film_samples(self._handle(), C.byref(done)))
        return done.value

    def read(self, what: int) -> np.ndarray:
        """(height, width, 3) f32 of one FILM_* quantity."""
        out = np.zeros((self.height, self.width, 3), dtype=np.float32)
        _check_host(host_lib().spt_host_multi_film_read(self._handle(), what, out.ctypes.data))
        return out

    def mean(self) -> np.ndarray:
        return self.read(FILM_MEAN)

    def sum(self) -> np.ndarray:
        return self.read(FILM_SUM)

    def sum_sq(self) -> np.ndarray:
        return self.read(FILM_SUM_SQ)

    def variance_of_mean(self) -> np.ndarray:
        return self.read(FILM_VAR_OF_MEAN)

    def sample_counts(self) -> np.ndarray:
        out = np.zeros((self.height, self.width), dtype=np.uint32)
        _check_host(host_lib().spt_host_multi_film_read_counts(self._handle(), out.ctypes.data))
        return out

    def adapt(self, rel_error: float, abs_floor: float = 0.0, min_samples: int = 16) -> int:
        """ProgressiveFilm.adapt on every shard; returns the pixels still active, summed over the shards."""
        active = C.c_uint32()
        _check_host(host_lib().spt_host_multi_film_adapt(self._handle(), rel_error, abs_floor, min_samples, C.byref(active)))
        return active.value

    def robust_mean(self, estimator: str = "gmon") -> np.ndarray:
        if estimator not in ("mon", "gmon"):
            raise ValueError("robust_mean: estimator is 'mon' or 'gmon', not %r" % (estimator,))
        out = np.zeros((self.height, self.width, 3), dtype=np.float32)
        _check_host(host_lib().spt_host_multi_film_read_robust(self._handle(), ROBUST_MON if estimator == "mon" else ROBUST_GMON, out.ctypes.data))
        return out

    def read_rgb8(self, source: str = "mean") -> np.ndarray:
        """(height, width, 3) u8 of "mean", "mon" or "gmon"; "denoised" is refused: denoise_job(rgb8=True) returns those bytes."""
        if source not in READ_SOURCES:
            raise ValueError("read_rgb8: source is one of %s, not %r" % (", ".join(repr(k) for k in READ_SOURCES), source))
        out = np.zeros((self.height, self.width, 3), dtype=np.uint8)
        _check_host(host_lib().spt_host_multi_film_read_rgb8(self._handle(), READ_SOURCES[source], out.ctypes.data))
        return out

    def denoise_job(self, guide: Optional["MultiFilm"] = None, albedo: Optional["MultiFilm"] = None, demodulate: bool = False,
                    rgb8: bool = False, **params) -> np.ndarray:
        """ProgressiveFilm.denoise_job with multi films: mean and variance of the mean of the film, the guide and the albedo film
        are gathered into full images and filtered by one spt_denoise_image on the first replica."""
        d = _denoise_keywords("denoise_job", params)
        dp = DenoiseParams(C.sizeof(DenoiseParams), d["iterations"], d["k_color"], d["k_guide"], d["eps_color"], d["eps_guide"])
        job = MultiFilmDenoiseJob(C.sizeof(MultiFilmDenoiseJob), (DENOISE_DEMODULATE if demodulate else 0) | (DENOISE_OUT_RGB8 if rgb8 else 0),
                                  guide._handle() if guide is not None else None, albedo._handle() if albedo is not None else None, C.pointer(dp),
                                  d["k_albedo"], d["eps_albedo"], d["eps_demod"], 0)
        out = np.zeros((self.height, self.width, 3), dtype=np.uint8 if rgb8 else np.float32)
        _check_host(host_lib().spt_host_multi_film_denoise(self._handle(), C.byref(job), out.ctypes.data))
        return out

    def close(self) -> None:
        if self._h:
            host_lib().spt_host_multi_film_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self) -> "MultiFilm":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiDevice:
    """One call, N devices, one film (spt_host_multi_*): a scene replica and a worker thread per device, interleaved row strips,
    every device's rows DMA-ed straight into the caller's film.  The reference's counterpart is the thread fan-out of
    PathTracer::render (src/renderer/pt.rs:243-287) into one UnsafeFilm (src/core/film.rs:101-116).
    `api` defaults to libspt_hip.so's functions; tests pass stand-ins."""

    def __init__(self, scene: Scene, devices, api: Optional[DeviceApi] = None):
        self.scene = scene
        self.devices = [int(d) for d in devices]
        self._api = api if api is not None else hip_device_api()
        self._h = C.c_void_p()
        self._film = None   # the film the library holds page-locked (spt_host.h): kept alive until it pins another or is destroyed
        self._films = weakref.WeakSet()   # MultiFilm objects on these replicas: destroyed before them
        desc = scene.desc
        devs = (C.c_int32 * len(self.devices))(*self.devices)
        _check_host(host_lib().spt_host_multi_create(C.byref(desc), C.byref(self._api), len(self.devices), devs, C.byref(self._h)))

    def render(self, renderer: "PathTracer", config: OutputConfig, strip_rows: int = 0, film: Optional[np.ndarray] = None,
               samples_per_pass: int = 0, camera_model: Optional["CameraModel"] = None) -> np.ndarray:
        """RendererT::render over all devices: the (H, W, 3) f32 film (a caller-owned `film` is filled in place).  A renderer
        with a weighted filter_type is refused (SptError): spt_render knows the box only, and the plan carries just the radius.
        A camera_model is refused too: the multi-device host layer copies a bare spt_camera."""
        if camera_model is not None:
            raise SptError(4, "MultiDevice.render: renders over several devices take the scene's pinhole camera only, no camera_model")
        if renderer.filter_type != "box":   # (params() would hand spt_render the reference's box at the filter's radius)
            raise SptError(4, "MultiDevice.render: spt_render over several devices filters with the box only, not %r "
                              "(render_shard serves a weighted filter on one device)" % (renderer.filter_type,))
        cam = self.scene.get_camera(config.used_camera_name)
        p = renderer.params(config.width, config.height, 0, 1, 16, samples_per_pass)
        if film is None:
            film = np.zeros((config.height, config.width, 3), dtype=np.float32)
        assert film.shape == (config.height, config.width, 3) and film.dtype == np.float32 and film.flags["C_CONTIGUOUS"]
        stats = (RenderStats * len(self.devices))()
        # the library unpins the film of the previous call and pins this one inside the call (spt_host.h), so the previous
        # array may go once the call has succeeded; after a refusal either of the two may be the registered one: both stay
        previous, self._film = self._film, film
        try:
            _check_host(host_lib().spt_host_multi_render(self._h, C.byref(cam), C.byref(p), strip_rows, film.ctypes.data, C.byref(stats)))
        except SptError:
            self._film = (previous, film)
            raise
        self.last_stats = list(stats)
        if config.output_filename:
            write_image(config.output_filename, film)
        return film

    def progressive(self, renderer: "PathTracer", config: OutputConfig, strip_rows: int = 0, first_sample: int = 0, moments: bool = False,
                    flags: int = 0, buckets: int = 0, film_api: Optional[DeviceFilmApi] = None, keep_samples: bool = False,
                    camera_model: Optional["CameraModel"] = None) -> MultiFilm:
        """PathTracer.progressive over all devices: a MultiFilm, one shard film per replica (shard k of n, strips of `strip_rows`
        rows, 0 = render()'s default).  `flags` are extra SPT_RENDER_* bits of the plan: RENDER_DEBUG_NORMAL / RENDER_AOV_ALBEDO
        with moments=True make the guide / albedo multi film of MultiFilm.denoise_job.  `film_api` defaults to libspt_hip.so's
        functions; tests pass stand-ins.  keep_samples=True: shard films that keep their samples (PathTracer.progressive), each
        tracing its own halo rows, so a box radius that reaches neighbouring pixels works over several devices too."""
        return MultiFilm(self, renderer, config, strip_rows, first_sample, moments, flags, buckets, film_api, keep_samples, camera_model)

    def close(self) -> None:
        for film in list(getattr(self, "_films", ())):
            film.close()
        if self._h:
            host_lib().spt_host_multi_destroy(self._h)
            self._h = C.c_void_p()
        self._film = None   # after the destroy: it unpins the film

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def block_candidates(camera: Camera, width: int, height: int, block: int, inv, fwd, tri_pos, shard_index: int = 0, shard_count: int = 1,
                     strip_rows: int = 16, rows: Optional[int] = None) -> int:
    """The candidate mask of one block (16 columns x 4 local rows: block = 4 * tile + wave) of a shard, by the test the primary
    kernel's masks are made with (include/spt_block_cand.h), on the host.  inv / fwd: 12 floats each (spt_instance); tri_pos: (n, 9)
    object-space vertices, n <= 64.  Bit k is set unless no camera ray of the block can hit triangle k."""
    inv, fwd = (np.ascontiguousarray(m, dtype=np.float32).reshape(12) for m in (inv, fwd))
    tri = np.ascontiguousarray(tri_pos, dtype=np.float32).reshape(-1, 9)
    if rows is None:
        rows = len(shard_rows(height, shard_index, shard_count, strip_rows))
    mask = C.c_uint64(0)
    _check_host(host_lib().spt_host_block_candidates(C.byref(camera), width, height, shard_index, shard_count, strip_rows, rows, block,
                                                     inv.ctypes.data, fwd.ctypes.data, len(tri), tri.ctypes.data, C.byref(mask)))
    return int(mask.value)


def origin_candidates(inv, fwd, nrm, tri_instance, tri_pos, tri_nrm):
    """The per-origin-triangle candidate table (include/spt_origin_cand.h) on the host.  inv / fwd: (n_instances, 12), nrm:
    (n_instances, 9) (spt_instance); triangle k belongs to instance tri_instance[k], tri_pos (n, 9) object-space vertices, tri_nrm
    (n, 9) its vertex normals, n <= 64; slot and row of a triangle are both k.  Returns (words, info): words (n, 4) uint64 - loose
    up, loose down, tight up, tight down - and info, a dict with center, radius, reach, delta, delta_scene and tight."""
    inv, fwd = (np.ascontiguousarray(m, dtype=np.float32).reshape(-1, 12) for m in (inv, fwd))
    nrm = np.ascontiguousarray(nrm, dtype=np.float32).reshape(-1, 9)
    owner = np.ascontiguousarray(tri_instance, dtype=np.uint32).reshape(-1)
    tri = np.ascontiguousarray(tri_pos, dtype=np.float32).reshape(-1, 9)
    tn = np.ascontiguousarray(tri_nrm, dtype=np.float32).reshape(-1, 9)
    assert len(inv) == len(fwd) == len(nrm) and len(tri) == len(tn) == len(owner)
    words = np.zeros((max(len(tri), 1), 4), dtype=np.uint64)
    info = np.zeros(8, dtype=np.float64)
    _check_host(host_lib().spt_host_origin_candidates(len(inv), inv.ctypes.data, fwd.ctypes.data, nrm.ctypes.data, len(tri), owner.ctypes.data,
                                                      tri.ctypes.data, tn.ctypes.data, words.ctypes.data, info.ctypes.data))
    return words[:len(tri)], {"center": info[0:3].copy(), "radius": float(info[3]), "reach": float(info[4]), "delta": float(info[5]),
                              "delta_scene": float(info[6]), "tight": bool(info[7])}


def make_camera(eye, forward, up, fov_degrees: float) -> Camera:
    """PerspectiveCamera::new (src/camera/perspective.rs:15-27) from f32 vectors."""
    f32 = np.float32
    e, f, u = (np.asarray(v, dtype=f32) for v in (eye, forward, up))
    f = f / f32(np.sqrt(f32(np.dot(f, f))))
    r = np.cross(f, u).astype(f32)
    r = r / f32(np.sqrt(f32(np.dot(r, r))))
    u = np.cross(r, f).astype(f32)
    cam = Camera()
    for k in range(3):
        cam.eye[k], cam.forward[k], cam.up[k], cam.right[k] = float(e[k]), float(f[k]), float(u[k]), float(r[k])
    cam.half_cot_half_fov = float(f32(0.5) / f32(np.tan(f32(np.radians(fov_degrees)) * f32(0.5))))
    return cam


# ---- ray generators for DeviceScene.radiance ------------------------------------------------------------------------------
# Pixel offsets are (H, W, 2) or (count, H, W, 2) f32 in [0, 1); the rays come back as (count, H, W) PATH_RAY_DTYPE records with
# t_min = CAMERA_T_MIN and the streams of a camera plan: stream_a = j * W + i (the pixel), stream_b = first_sample + s.

def _offsets4(offsets, width: int, height: int) -> np.ndarray:
    off = np.asarray(offsets, dtype=np.float32)
    if off.ndim == 3:
        off = off[None]
    if off.ndim != 4 or off.shape[1:] != (height, width, 2):
        raise ValueError("offsets: (height, width, 2) or (count, height, width, 2) is expected")
    return off


def _plan_rays(count: int, width: int, height: int, first_sample: int) -> np.ndarray:
    rays = np.zeros((count, height, width), dtype=PATH_RAY_DTYPE)
    rays["t_min"] = np.float32(CAMERA_T_MIN)
    rays["stream_a"] = (np.arange(height, dtype=np.uint32)[:, None] * np.uint32(width) + np.arange(width, dtype=np.uint32)[None, :])[None]
    rays["stream_b"] = (np.uint32(first_sample) + np.arange(count, dtype=np.uint32))[:, None, None]
    return rays


def _unit64(v: np.ndarray) -> np.ndarray:
    """Directions normalised in float64 and rounded once: |d|^2 is within 2^-23 of 1."""
    v = np.asarray(v, dtype=np.float64)
    return (v / np.sqrt(np.sum(v * v, axis=-1, keepdims=True))).astype(np.float32)


def perspective_rays(camera: Camera, width: int, height: int, offsets, aux_spp: Optional[int] = None, *, first_sample: int = 0):
    """The camera rays of a plan, bit for bit: pt.rs:269-271 and PerspectiveCamera::generate_ray (camera/perspective.rs:40-47) in
    float32 numpy, one rounded operation at a time.  `offsets` are the plan's pixel offsets of the samples first_sample, ... .
    With aux_spp (the plan's spp) the auxiliary rays of generate_ray_with_aux_ray (pt.rs:272-275) come back too, as
    RAY_AUX_DTYPE records of the same shape: (rays, aux)."""
    f32 = np.float32
    off = _offsets4(offsets, width, height)
    fwd, up, right, eye = (np.array(list(v), dtype=f32) for v in (camera.forward, camera.up, camera.right, camera.eye))
    hc = f32(camera.half_cot_half_fov)
    aspect = f32(width) / f32(height)
    width_inv, height_inv = f32(1) / f32(width), f32(1) / f32(height)
    col = np.arange(width, dtype=np.uint32).astype(f32)[None, None, :]
    row = (np.uint32(height) - np.arange(height, dtype=np.uint32) - np.uint32(1)).astype(f32)[None, :, None]
    x = ((col + off[..., 0]) * width_inv - f32(0.5)) * aspect
    y = (row + off[..., 1]) * height_inv - f32(0.5)

    def direction(x, y):
        v = [(fwd[k] * hc + right[k] * x) + up[k] * y for k in range(3)]
        length = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        return np.stack([c / length for c in v], axis=-1).astype(f32)

    rays = _plan_rays(off.shape[0], width, height, first_sample)
    rays["o"] = eye
    rays["d"] = direction(x, y)
    if aux_spp is None:
        return rays
    spp_sqrt_inv = f32(1) / np.sqrt(f32(aux_spp))
    aux_dx, aux_dy = aspect * width_inv * spp_sqrt_inv, height_inv * spp_sqrt_inv
    aux = np.zeros(rays.shape, dtype=RAY_AUX_DTYPE)
    aux["rx_o"] = eye
    aux["ry_o"] = eye
    aux["rx_d"] = direction(x + aux_dx, y)
    aux["ry_d"] = direction(x, y + aux_dy)
    return rays, aux


def _screen_xy(off: np.ndarray, width: int, height: int):
    """x in [-aspect / 2, aspect / 2) to the right and y in (-0.5, 0.5] upwards (row 0 on top), as pt.rs:269-271, in float64."""
    col = np.arange(width, dtype=np.float64)[None, None, :]
    row = (height - 1 - np.arange(height, dtype=np.float64))[None, :, None]
    return ((col + off[..., 0]) / width - 0.5) * (width / height), (row + off[..., 1]) / height - 0.5


def orthographic_rays(camera: Camera, width: int, height: int, offsets, view_height: float, *, first_sample: int = 0) -> np.ndarray:
    """Parallel rays along camera.forward.  The image plane passes through camera.eye; screen coordinates are those of the
    perspective camera (x to camera.right, y to camera.up, row 0 on top) scaled so that the image is view_height world units
    high: o = eye + (right * x + up * y) * view_height, d = forward normalised.  half_cot_half_fov is not used."""
    off = _offsets4(offsets, width, height)
    x, y = _screen_xy(off, width, height)
    fwd, up, right, eye = (np.array(list(v), dtype=np.float64) for v in (camera.forward, camera.up, camera.right, camera.eye))
    rays = _plan_rays(off.shape[0], width, height, first_sample)
    rays["o"] = (eye + (right * x[..., None] + up * y[..., None]) * float(view_height)).astype(np.float32)
    rays["d"] = _unit64(fwd)
    return rays


def panorama_rays(origin, width: int, height: int, offsets, *, first_sample: int = 0) -> np.ndarray:
    """Equirectangular rays from `origin`, in the environment map's own parametrisation (environment.rs:128-133: theta =
    acos(d.y), phi = atan2(d.x, d.z) + pi): row j looks at theta = (j + oy) / height * pi, so row 0 starts at theta 0 (+y, the
    top pole) and the last row ends at theta pi (-y); column i looks at phi = (i + ox) / width * 2 pi, so the seam phi = 0 at the
    left edge of column 0 looks along -z, the image centre phi = pi along +z, and phi = pi / 2 along -x.
    This float64 helper counts the vertical offset downward (row j covers theta from j to j + 1); the device's panorama model
    (CameraModel.panorama, camera_rays) keeps the pinhole's convention, oy running upward inside the row, so the two agree on
    the pixel grid and differ in where inside its row a sample lies.  The helper stays as it is."""
    off = _offsets4(offsets, width, height)
    theta = (np.arange(height, dtype=np.float64)[None, :, None] + off[..., 1]) / height * np.pi
    phi = (np.arange(width, dtype=np.float64)[None, None, :] + off[..., 0]) / width * (2.0 * np.pi)
    st = np.sin(theta)
    d = np.stack([st * np.sin(phi - np.pi), np.cos(theta), st * np.cos(phi - np.pi)], axis=-1)
    rays = _plan_rays(off.shape[0], width, height, first_sample)
    rays["o"] = np.asarray(origin, dtype=np.float32)
    rays["d"] = _unit64(d)
    return rays


def thin_lens_rays(camera: Camera, width: int, height: int, offsets, lens_uv, lens_radius: float, focus_distance: float, *,
                   first_sample: int = 0) -> np.ndarray:
    """The perspective camera behind a thin lens.  The pinhole ray through screen point (x, y) meets the plane of focus -
    focus_distance along camera.forward from the eye - at F = eye + (forward * half_cot + right * x + up * y) * (focus_distance /
    half_cot); the ray starts on the lens at o = eye + (right * lx + up * ly) * lens_radius, where (lx, ly) is lens_uv (shaped like
    offsets, in [0, 1)^2) mapped to the unit disk by Shirley's concentric map, and d = normalize(F - o).  lens_radius 0 gives
    the pinhole's rays up to rounding."""
    off = _offsets4(offsets, width, height)
    uv = _offsets4(lens_uv, width, height).astype(np.float64) * 2.0 - 1.0
    if uv.shape != off.shape:
        raise ValueError("lens_uv: the shape of offsets is expected")
    a, b = uv[..., 0], uv[..., 1]
    wide = np.abs(a) > np.abs(b)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(wide, a, b)
        ang = np.where(wide, (np.pi / 4) * (b / a), np.pi / 2 - (np.pi / 4) * (a / b))
    ang = np.where((a == 0) & (b == 0), 0.0, ang)
    lx, ly = r * np.cos(ang), r * np.sin(ang)
    x, y = _screen_xy(off, width, height)
    fwd, up, right, eye = (np.array(list(v), dtype=np.float64) for v in (camera.forward, camera.up, camera.right, camera.eye))
    hc = float(camera.half_cot_half_fov)
    focus = eye + (fwd * hc + right * x[..., None] + up * y[..., None]) * (float(focus_distance) / hc)
    o = eye + (right * lx[..., None] + up * ly[..., None]) * float(lens_radius)
    rays = _plan_rays(off.shape[0], width, height, first_sample)
    rays["o"] = o.astype(np.float32)
    rays["d"] = _unit64(focus - o)
    return rays


def load_renderer(path: str, seed: int = 1) -> PathTracer:
    """loader::load_renderer (src/loader/json.rs:19-51)."""
    p = RenderParams()
    lib = host_lib()
    if hasattr(lib, "spt_host_load_renderer_filter"):   # also takes the weighted filters of spt_film_filter
        fd = FilterDesc()
        _check_host(lib.spt_host_load_renderer_filter(os.fspath(path).encode(), C.byref(p), C.byref(fd)))
        kind = [k for k, v in FILTER_TYPES.items() if v == fd.type][0]
        extra = {"alpha": fd.p0} if kind == "gaussian" else {"b": fd.p0, "c": fd.p1} if kind == "mitchell" else {}
        return PathTracer(p.max_depth, p.sampler, p.spp, p.division_x, p.division_y, fd.radius, seed, filter_type=kind, filter_params=extra)
    radius = C.c_float()
    _check_host(lib.spt_host_load_renderer(os.fspath(path).encode(), C.byref(p), C.byref(radius)))
    return PathTracer(p.max_depth, p.sampler, p.spp, p.division_x, p.division_y, radius.value, seed)


def film_to_rgb8(film: np.ndarray) -> np.ndarray:
    """color_to_rgb (src/core/film.rs:94-99): truncating, no gamma."""
    film = np.ascontiguousarray(film, dtype=np.float32)
    out = np.zeros(film.shape, dtype=np.uint8)
    host_lib().spt_host_film_to_rgb8(film.ctypes.data, film.size // 3, out.ctypes.data)
    return out


def _as_rgb8(film: np.ndarray) -> np.ndarray:
    """A float film through film_to_rgb8; a u8 image (ProgressiveFilm.read_rgb8) as it is."""
    if film.dtype == np.uint8:
        return np.ascontiguousarray(film)
    return film_to_rgb8(film)


def write_png(path: str, film: np.ndarray) -> None:
    rgb8 = _as_rgb8(film)
    h, w = rgb8.shape[:2]
    _check_host(host_lib().spt_host_write_png(os.fspath(path).encode(), rgb8.ctypes.data, w, h))


def write_image(path: str, film: np.ndarray) -> None:
    """`image.save(path)` (src/renderer/pt.rs:292-294): png or jpg / jpeg by extension.  `film`: f32, or the u8 image itself."""
    rgb8 = _as_rgb8(film)
    h, w = rgb8.shape[:2]
    _check_host(host_lib().spt_host_write_image(os.fspath(path).encode(), rgb8.ctypes.data, w, h))


def write_jpeg(path: str, rgb8: np.ndarray, quality: int = 75) -> None:
    rgb8 = np.ascontiguousarray(rgb8, dtype=np.uint8)
    h, w = rgb8.shape[:2]
    _check_host(host_lib().spt_host_write_jpeg(os.fspath(path).encode(), rgb8.ctypes.data, w, h, quality))


def read_png(path: str) -> np.ndarray:
    """(h, w, 4) uint8 RGBA as `image::open` + `get_pixel` present an image texture file (PNG or JPEG)."""
    w, h = C.c_uint32(), C.c_uint32()
    ptr = C.POINTER(C.c_uint32)()
    _check_host(host_lib().spt_host_read_png(os.fspath(path).encode(), C.byref(w), C.byref(h), C.byref(ptr)))
    arr = np.ctypeslib.as_array(ptr, shape=(h.value, w.value)).copy()
    host_lib().spt_host_free(ptr)
    return arr.view(np.uint8).reshape(h.value, w.value, 4)


def read_exr(path: str) -> np.ndarray:
    w, h = C.c_uint32(), C.c_uint32()
    ptr = C.POINTER(C.c_float)()
    _check_host(host_lib().spt_host_read_exr(os.fspath(path).encode(), C.byref(w), C.byref(h), C.byref(ptr)))
    arr = np.ctypeslib.as_array(ptr, shape=(h.value, w.value, 3)).copy()
    host_lib().spt_host_free(ptr)
    return arr


def catmull_clark_patches(ply_path: str, fas_times: int = 4) -> np.ndarray:
    """CatmullClark::load (src/primitive/catmull.rs:93-101): (n, 4, 4, 3) Bezier control points of the subdivision surface."""
    n = C.c_uint32()
    ptr = C.POINTER(C.c_float)()
    _check_host(host_lib().spt_host_catmull_clark(os.fspath(ply_path).encode(), fas_times, C.byref(n), C.byref(ptr)))
    arr = np.ctypeslib.as_array(ptr, shape=(max(n.value, 1), 4, 4, 3))[: n.value].copy()
    host_lib().spt_host_free(ptr)
    return arr


def write_exr(path: str, rgb: np.ndarray) -> None:
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    _check_host(host_lib().spt_host_write_exr(os.fspath(path).encode(), rgb.ctypes.data, rgb.shape[1], rgb.shape[0]))


def gather_shards(shard: np.ndarray, height: int, width: int, rank: int, world: int, strip_rows: int, dist=None):
    """Host-side gather of the per-rank row shards into the full (H, W, 3) film on rank 0.

    Shards are disjoint sets of image rows (interleaved strips), so this is a concatenation, not a
    reduction; `dist` is torch.distributed (its CPU/gloo path is used) or None for a single rank.
    Returns the film on rank 0 and None elsewhere.  (The reference has one address space and no
    counterpart; cf. UnsafeFilm, src/core/film.rs:101-116.)"""
    rows_all = [shard_rows(height, r, world, strip_rows) for r in range(world)]
    assert shard.shape == (len(rows_all[rank]), width, 3), (shard.shape, len(rows_all[rank]))
    if world == 1 or dist is None:
        full = np.zeros((height, width, 3), dtype=np.float32)
        full[rows_all[0]] = shard
        return full
    import torch
    max_rows = max(len(r) for r in rows_all)          # gather needs equal shapes: pad short shards
    padded = np.zeros((max_rows, width, 3), dtype=np.float32)
    padded[: shard.shape[0]] = shard
    t = torch.from_numpy(padded)
    if rank == 0:
        bufs = [torch.empty((max_rows, width, 3), dtype=torch.float32) for _ in range(world)]
        dist.gather(t, bufs, dst=0)
        full = np.zeros((height, width, 3), dtype=np.float32)
        for r in range(world):
            full[rows_all[r]] = bufs[r].numpy()[: len(rows_all[r])]
        return full
    dist.gather(t, None, dst=0)
    return None


class SharedFilm:
    """The full (H, W, 3) f32 film in POSIX shared memory, one mapping per rank of a node.

    Every rank writes the image rows of its own shard (disjoint interleaved strips), so assembling the
    image needs no collective and no copy through a socket: it is the multi-process counterpart of the
    reference's UnsafeFilm (src/core/film.rs:101-116), where all render threads write disjoint pixels of one
    film.  Rank 0 creates the segment and passes `name` to the others (e.g. dist.broadcast_object_list)."""

    def __init__(self, height: int, width: int, name: Optional[str] = None, create: bool = False):
        from multiprocessing import shared_memory
        self.height, self.width = height, width
        nbytes = height * width * 3 * 4
        if create:
            self._shm = shared_memory.SharedMemory(create=True, size=nbytes, name=name)
        else:
            self._shm = shared_memory.SharedMemory(name=name)
            # the creating rank owns the segment: keep this process' resource tracker from unlinking it
            try:
                from multiprocessing import resource_tracker
                resource_tracker.unregister(self._shm._name, "shared_memory")
            except Exception:
                pass
        self._owner = create
        self._pinned = False
        self.name = self._shm.name
        self.film = np.ndarray((height, width, 3), dtype=np.float32, buffer=self._shm.buf)

    def pin(self) -> None:
        """Page-lock this process' mapping (spt_pin_host) so that render_shard(film=self.film) copies out at DMA speed."""
        if not self._pinned:
            _check_hip(hip_lib().spt_pin_host(self.film.ctypes.data, self.film.nbytes))
            self._pinned = True

    def write_shard(self, shard: np.ndarray, rank: int, world: int, strip_rows: int) -> None:
        rows = shard_rows(self.height, rank, world, strip_rows)
        assert shard.shape == (len(rows), self.width, 3), (shard.shape, len(rows))
        # rows of one strip are contiguous in both arrays: one memcpy per strip
        k = 0
        while k < len(rows):
            e = k
            while e + 1 < len(rows) and rows[e + 1] == rows[e] + 1:
                e += 1
            self.film[rows[k]:rows[e] + 1] = shard[k:e + 1]
            k = e + 1

    def close(self) -> None:
        if self._pinned:
            hip_lib().spt_unpin_host(self.film.ctypes.data)
            self._pinned = False
        self.film = None
        self._shm.close()
        if self._owner:
            self._shm.unlink()


def device_detmath(fn: int, a: np.ndarray, b: Optional[np.ndarray] = None, device: int = 0) -> np.ndarray:
    """Test seam (spt_debug_detmath): include/spt_detmath.h evaluated on the GPU."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b if b is not None else np.zeros_like(a), dtype=np.float32)
    out = np.zeros_like(a)
    _check_hip(hip_lib().spt_debug_detmath(device, fn, a.size, a.ctypes.data, b.ctypes.data, out.ctypes.data))
    return out


def debug_pack_rgb8(values: np.ndarray, device: int = 0) -> np.ndarray:
    """Test seam (spt_debug_pack_rgb8): the device's conversion kernel on any number of f32 values; u8 of the same shape."""
    values = np.ascontiguousarray(values, dtype=np.float32)
    out = np.zeros(values.shape, dtype=np.uint8)
    _check_hip(hip_lib().spt_debug_pack_rgb8(device, values.size, values.ctypes.data, out.ctypes.data))
    return out


def device_bxdf_sample(mt: "Material", wo: np.ndarray, rng_state: np.ndarray, scene: Optional[Scene] = None, device: int = 0):
    """Test seam (spt_debug_bxdf op 0): Bxdf::sample of one constant material record on the GPU for n (wo, RNG state) pairs.
    Returns (wi (n, 3), f (n, 3), pdf (n,), dir (n,) 0 reflect / 1 transmit)."""
    wo = np.ascontiguousarray(wo, dtype=np.float32).reshape(-1, 3)
    st = np.ascontiguousarray(rng_state, dtype=np.uint64)
    n = wo.shape[0]
    assert st.shape == (n,)
    wi, f, pdf, dr = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32)
    h = scene.device_scene(device)._h if scene is not None else None
    _check_hip(hip_lib().spt_debug_bxdf(h, device, C.byref(mt), 0, n, wo.ctypes.data, None, st.ctypes.data, wi.ctypes.data, f.ctypes.data,
                                        pdf.ctypes.data, dr.ctypes.data))
    return wi, f, pdf, dr


def device_bxdf_eval(mt: "Material", wo: np.ndarray, wi: np.ndarray, scene: Optional[Scene] = None, device: int = 0):
    """Test seam (spt_debug_bxdf op 1): Bxdf::bxdf and Bxdf::pdf on the GPU for n (wo, wi) pairs -> (f (n, 3), pdf (n,))."""
    wo = np.ascontiguousarray(wo, dtype=np.float32).reshape(-1, 3)
    wi = np.ascontiguousarray(wi, dtype=np.float32).reshape(-1, 3)
    n = wo.shape[0]
    assert wi.shape == (n, 3)
    f, pdf = np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
    h = scene.device_scene(device)._h if scene is not None else None
    _check_hip(hip_lib().spt_debug_bxdf(h, device, C.byref(mt), 1, n, wo.ctypes.data, wi.ctypes.data, None, None, f.ctypes.data, pdf.ctypes.data, None))
    return f, pdf


def device_count() -> int:
    n = C.c_int32()
    _check_hip(hip_lib().spt_device_count(C.byref(n)))
    return n.value


def render_flags_supported() -> int:
    """spt_render_flags_supported: the RENDER_* bits the loaded library honours.  A library without the call (it ignores
    unknown bits silently) honours the five flags up to RENDER_DEBUG_NORMAL."""
    lib = hip_lib()
    if not hasattr(lib, "spt_render_flags_supported"):
        return RENDER_PROFILE | RENDER_BOX_RADIUS | RENDER_COUNT_VISITS | RENDER_ASYNC | RENDER_DEBUG_NORMAL
    mask = C.c_uint32()
    _check_hip(lib.spt_render_flags_supported(C.byref(mask)))
    return mask.value
