"""spt_film_denoise_job in float32 numpy: tests/_denoise_ref.py's filter with the albedo term and albedo demodulation of spt_abi.h,
one rounded operation at a time and in that order, so its result has the bits of the device's.  Without an albedo film it is
_denoise_ref.denoise operation for operation (tests/test_albedo_reference.py compares the two).
"""
import numpy as np

import _denoise_ref as D

f32 = np.float32
DEFAULTS = dict(D.DEFAULTS, k_albedo=1.0, eps_albedo=1e-2, eps_demod=1e-2)


def denoise_job(m, v, g=None, u=None, al=None, ua=None, demodulate=False, iterations=5, k_color=2.0, k_guide=1.0, eps_color=1e-8,
                eps_guide=1e-2, k_albedo=1.0, eps_albedo=1e-2, eps_demod=1e-2):
    """m, v: SPT_FILM_MEAN and SPT_FILM_VAR_OF_MEAN of the colour film, (rows, width, 3) f32; g, u: those of the guide, or None;
    al, ua: those of the albedo film, or None.  demodulate needs the albedo film."""
    assert not demodulate or al is not None
    m, v = np.asarray(m, f32), np.asarray(v, f32)
    kc2, kg2, eps_c, eps_g = f32(k_color) * f32(k_color), f32(k_guide) * f32(k_guide), f32(eps_color), f32(eps_guide)
    ka2, eps_a, eps_d = f32(k_albedo) * f32(k_albedo), f32(eps_albedo), f32(eps_demod)
    shift, LW, H = D._shift, D.LW, D.H
    with np.errstate(all="ignore"):
        c = m.copy()
        if al is not None:
            al, ua = np.asarray(al, f32), np.asarray(ua, f32)
            av = (ua[..., 0] + ua[..., 1]) + ua[..., 2]
        if demodulate:
            dem = np.where(al > eps_d, al, eps_d).astype(f32)       # a NaN albedo gives the floor
            c = (m / dem).astype(f32)
            v = (v / (dem * dem)).astype(f32)
        lv = ((LW[0] * LW[0]) * v[..., 0] + (LW[1] * LW[1]) * v[..., 1]) + (LW[2] * LW[2]) * v[..., 2]
        if g is not None:
            g, u = np.asarray(g, f32), np.asarray(u, f32)
            gv = (u[..., 0] + u[..., 1]) + u[..., 2]
        for k in range(iterations):
            s = 1 << k
            l = D._lum(c)
            ok = np.isfinite(c).all(axis=-1) & np.isfinite(lv)
            acc = np.zeros_like(c)
            ws = np.zeros_like(lv)
            va = np.zeros_like(lv)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    oy, ox = s * dy, s * dx
                    take = shift(ok, oy, ox, False)             # inside the image and ok(q)
                    cq, lvq = shift(c, oy, ox, f32(0)), shift(lv, oy, ox, f32(0))
                    dl = l - shift(l, oy, ox, f32(0))
                    d = (dl * dl) / (kc2 * (lv + lvq) + eps_c)
                    if g is not None:
                        e = g - shift(g, oy, ox, f32(0))
                        d = d + ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]) / (kg2 * (gv + shift(gv, oy, ox, f32(0))) + eps_g)
                    if al is not None:
                        e = al - shift(al, oy, ox, f32(0))
                        d = d + ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]) / (ka2 * (av + shift(av, oy, ox, f32(0))) + eps_a)
                    take &= d < f32(87.0)                       # (false for a NaN)
                    w = (H[dy + 2] * H[dx + 2]) * D.spt_exp(np.where(take, -d, f32(0)))
                    acc = np.where(take[..., None], acc + w[..., None] * cq, acc)
                    ws = np.where(take, ws + w, ws)
                    va = np.where(take, va + (w * w) * lvq, va)
            c = np.where(ok[..., None], acc / ws[..., None], c).astype(f32)
            lv = np.where(ok, va / (ws * ws), lv).astype(f32)
        if demodulate:
            c = (c * dem).astype(f32)                           # every pixel, those that passed through included
    return c
