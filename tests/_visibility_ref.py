"""spt_occluded and spt_ao restated over calls that exist without them (include/spt_abi.h, "visibility along caller rays and at surface
points").  The rays of an AO call are the gather rays of the bake with the same (seed, first_point, first_sample): spt.bake_rays
returns them.  A `trace_any` callable (a DeviceScene's, or _util.OracleScene's) judges them; the record is then float32 numpy, one
rounded operation at a time in the written order: the in-order sums, open, and bent with true divisions."""
import numpy as np

import _bake_ref

f32 = np.float32
F32_MAX = np.finfo(f32).max


def scene_extent(scene):
    """The diagonal of the box around every instance."""
    inst = scene.array("instances")
    return f32(np.linalg.norm(inst["bmax"].max(axis=0).astype(np.float64) - inst["bmin"].min(axis=0).astype(np.float64)))


def segments(spt, rays, max_distance=np.inf):
    """The RAY_DTYPE segments (o, t_min, d, t_max) of PATH_RAY_DTYPE rays: t_max = max_distance when finite, else f32::MAX."""
    rays = np.asarray(rays)
    seg = np.zeros(rays.shape, dtype=spt.RAY_DTYPE)
    seg["o"], seg["t_min"], seg["d"] = rays["o"], rays["t_min"], rays["d"]
    seg["t_max"] = f32(max_distance) if np.isfinite(max_distance) else F32_MAX
    return seg


def occlusion(spt, made, trace_any, max_distance=np.inf):
    """(n, S) uint8: trace_any over the gather rays of `made` (a dict of spt.bake_rays)."""
    seg = segments(spt, made["rays"], max_distance)
    return np.asarray(trace_any(seg.reshape(-1))).reshape(seg.shape)


def ao_records(spt, made, trace_any, max_distance=np.inf, occ=None, start=None, finish=True):
    """The AO_DTYPE records of the points of `made`.  `start`: records whose sum and count the additions go on from (a call cut by
    first_sample); `finish`: make open and bent (over the S of `made`)."""
    if occ is None:
        occ = occlusion(spt, made, trace_any, max_distance)
    d = made["rays"]["d"]
    n, S = occ.shape
    acc = np.zeros((n, 3), dtype=f32) if start is None else start["sum"].copy()
    count = np.zeros(n, dtype=np.uint32) if start is None else start["count"].copy()
    for k in range(S):
        free = occ[:, k] == 0
        acc = np.where(free[:, None], acc + d[:, k], acc)
        count = count + free.astype(np.uint32)
    rec = np.zeros(n, dtype=spt.AO_DTYPE)
    rec["sum"], rec["count"] = acc, count
    if finish:
        rec["open"] = count.astype(f32) * (f32(1) / f32(S))
        some = (count > 0) & np.any(acc != 0, axis=-1)
        with np.errstate(invalid="ignore", divide="ignore"):
            bent = _bake_ref.normalize(acc)
        rec["bent"] = np.where(some[:, None], bent, f32(0))
    return rec


def words(rec):
    """AO_DTYPE records as (n, 8) uint32."""
    return np.ascontiguousarray(rec).view(np.uint32).reshape(-1, 8)
