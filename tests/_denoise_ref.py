"""spt_film_denoise in float32 numpy, one rounded operation at a time and in the order of spt_abi.h (numpy does not contract), so
its result has the bits of the device's.  exp is spt_detmath.h's spt_exp through the oracle (oracle_detmath(3, ...)).
"""
import numpy as np

import _util

f32 = np.float32
LW = (f32(0.299), f32(0.587), f32(0.114))
H = (f32(1) / f32(16), f32(1) / f32(4), f32(3) / f32(8), f32(1) / f32(4), f32(1) / f32(16))
DEFAULTS = dict(iterations=5, k_color=2.0, k_guide=1.0, eps_color=1e-8, eps_guide=1e-2)


def spt_exp(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty_like(x)
    _util.oracle_lib().oracle_detmath(3, x.size, x.ctypes.data, x.ctypes.data, out.ctypes.data)
    return out


def _lum(c):
    return (LW[0] * c[..., 0] + LW[1] * c[..., 1]) + LW[2] * c[..., 2]


def _shift(a, oy, ox, fill):
    """b[y, x] = a[y + oy, x + ox] inside the image, `fill` outside."""
    rows, w = a.shape[:2]
    b = np.full_like(a, fill)
    y0, y1, x0, x1 = max(0, -oy), min(rows, rows - oy), max(0, -ox), min(w, w - ox)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return b


def denoise(m, v, g=None, u=None, iterations=5, k_color=2.0, k_guide=1.0, eps_color=1e-8, eps_guide=1e-2):
    """m, v: SPT_FILM_MEAN and SPT_FILM_VAR_OF_MEAN of the colour film, (rows, width, 3) f32; g, u: those of the guide, or None."""
    m, v = np.asarray(m, f32), np.asarray(v, f32)
    kc2, kg2, eps_c, eps_g = f32(k_color) * f32(k_color), f32(k_guide) * f32(k_guide), f32(eps_color), f32(eps_guide)
    with np.errstate(all="ignore"):
        c = m.copy()
        lv = ((LW[0] * LW[0]) * v[..., 0] + (LW[1] * LW[1]) * v[..., 1]) + (LW[2] * LW[2]) * v[..., 2]
        if g is not None:
            g, u = np.asarray(g, f32), np.asarray(u, f32)
            gv = (u[..., 0] + u[..., 1]) + u[..., 2]
        for k in range(iterations):
            s = 1 << k
            l = _lum(c)
            ok = np.isfinite(c).all(axis=-1) & np.isfinite(lv)
            acc = np.zeros_like(c)
            ws = np.zeros_like(lv)
            va = np.zeros_like(lv)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    oy, ox = s * dy, s * dx
                    take = _shift(ok, oy, ox, False)            # inside the image and ok(q)
                    cq, lvq = _shift(c, oy, ox, f32(0)), _shift(lv, oy, ox, f32(0))
                    dl = l - _shift(l, oy, ox, f32(0))
                    d = (dl * dl) / (kc2 * (lv + lvq) + eps_c)
                    if g is not None:
                        e = g - _shift(g, oy, ox, f32(0))
                        d = d + ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]) / (kg2 * (gv + _shift(gv, oy, ox, f32(0))) + eps_g)
                    take &= d < f32(87.0)                       # (false for a NaN)
                    w = (H[dy + 2] * H[dx + 2]) * spt_exp(np.where(take, -d, f32(0)))
                    acc = np.where(take[..., None], acc + w[..., None] * cq, acc)
                    ws = np.where(take, ws + w, ws)
                    va = np.where(take, va + (w * w) * lvq, va)
            c = np.where(ok[..., None], acc / ws[..., None], c).astype(f32)
            lv = np.where(ok, va / (ws * ws), lv).astype(f32)
    return c


def rmse_ratio(noisy, denoised, reference):
    """RMSE(denoised) / RMSE(noisy) against `reference` over the pixels finite in all three, and how many pixels were left out."""
    keep = np.isfinite(noisy).all(axis=-1) & np.isfinite(denoised).all(axis=-1) & np.isfinite(reference).all(axis=-1)
    ref = reference[keep].astype(np.float64)
    rmse = lambda img: float(np.sqrt(((img[keep].astype(np.float64) - ref) ** 2).mean()))
    return rmse(denoised) / rmse(noisy), int((~keep).sum())


# the quality gate shared by the CPU (oracle films) and the GPU test: scene, camera, then the bounds with and without a guide
QUALITY_PLAN = dict(width=96, height=72, spp=16, seed=5, max_depth=5, ref_spp=2048, ref_seed=77)
QUALITY_SCENES = [
    ("cfg2_cube.json", None, 1.0, None),          # about 80 % black background: little to gain; without a guide the edges blur
    ("t_materials.json", "main", 0.75, 0.75),
    ("t_textured.json", None, 0.75, 0.75),
    ("t_plastic.json", None, 0.75, 0.75),
    ("t_medium.json", None, 0.75, 0.75),
]
MAX_LEFT_OUT = 0.001    # share of pixels that are not finite in one of the images


def oracle_film(scene, renderer, width, height, camera, n, flags):
    """MEAN and VAR_OF_MEAN of a moments film holding the plan's first n samples, from the oracle's single samples."""
    x = _util.oracle_render_samples(scene, renderer, width, height, 0, n, camera=camera, flags=flags)
    s, q = np.zeros_like(x[0]), np.zeros_like(x[0])
    with np.errstate(all="ignore"):
        for k in range(n):
            s, q = _util.film_add_sample(s, q, x[k])
        return _util.film_mean_and_variance(s, q, n)
