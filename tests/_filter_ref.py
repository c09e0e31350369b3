"""The read-out of a sample-keeping film under a weighted reconstruction filter (spt_film_filter, include/spt_abi.h), restated in
float32 numpy:

    color = 0; wsum = 0
    for dj = -Rf .. Rf, for di = -Rf .. Rf (pixels outside the image skipped), for the pixel's samples in increasing plan index:
        ax = |(float)di + (ox - 0.5f)|;  ay = |(float)dj + (oy - 0.5f)|;  skipped unless ax <= r and ay <= r
        w = f(ax) * f(ay);  skipped when w == 0.0f
        color.c = color.c + w * x.c;  wsum = wsum + w
    sum = color;  mean = color * (1.0f / wsum)

with Rf = max(ceil(r - 0.5), 0).  Every operation is one rounded f32 operation (numpy does not contract); the loops over the output
pixels are vectorised, the loops the specification orders are not.  exp is spt_detmath.h's spt_exp through the oracle, as in
_denoise_ref.py; Mitchell's coefficients are made in Python floats (doubles) in the header's order and rounded once.
The sample offsets come from _wide_film_ref.offsets().
"""
import numpy as np

from _denoise_ref import spt_exp
from _wide_film_ref import offsets  # noqa: F401  (re-exported: the callers take both from here)

f32 = np.float32


def radius_int(radius):
    return max(int(np.ceil(f32(radius) - f32(0.5))), 0)


def mitchell_coefficients(b, c):
    """(c3, c2, c1, c0, q3, q2, q0) as f32: B and C are the desc's floats widened to double."""
    B, C = float(f32(b)), float(f32(c))
    return tuple(f32(v) for v in ((-B - 6 * C) / 6, (6 * B + 30 * C) / 6, (-12 * B - 48 * C) / 6, (8 * B + 24 * C) / 6,
                                  (12 - 9 * B - 6 * C) / 6, (-18 + 12 * B + 6 * C) / 6, (6 - 2 * B) / 6))


def filter_fn(kind, radius, alpha=2.0, b=1.0 / 3.0, c=1.0 / 3.0):
    """f(a) of the filter on f32 arrays of distances 0 <= a <= r."""
    r = f32(radius)
    if kind == "tent":
        return lambda a: r - np.asarray(a, dtype=f32)
    if kind == "gaussian":
        al = f32(alpha)
        e_r = spt_exp(np.array([-(al * (r * r))], dtype=f32))[0]

        def gaussian(a):
            a = np.asarray(a, dtype=f32)
            g = spt_exp(-(al * (a * a))).reshape(a.shape) - e_r
            return np.where(g < 0, f32(0), g).astype(f32)
        return gaussian
    assert kind == "mitchell", kind
    c3, c2, c1, c0, q3, q2, q0 = mitchell_coefficients(b, c)

    def mitchell(a):
        t = (f32(2) * np.asarray(a, dtype=f32)) / r
        outer = ((c3 * t + c2) * t + c1) * t + c0
        inner = ((q3 * t + q2) * t) * t + q0
        return np.where(t > 1, outer, inner).astype(f32)
    return mitchell


def filter_film(samples, off, kind, radius, **params):
    """samples (n, H, W, 3) f32 and their offsets (n, H, W, 2) -> (color, wsum, mean) of every pixel of the image."""
    samples = np.asarray(samples, dtype=f32)
    off = np.asarray(off, dtype=f32)
    n, H, W, _ = samples.shape
    R = radius_int(radius)
    rad = f32(radius)
    f = filter_fn(kind, radius, **params)
    color = np.zeros((H, W, 3), dtype=f32)
    wsum = np.zeros((H, W), dtype=f32)
    with np.errstate(all="ignore"):
        for dj in range(-R, R + 1):
            # output rows y with 0 <= y + dj < H, and the rows y + dj they read
            y0, y1 = max(0, -dj), min(H, H - dj)
            if y0 >= y1:
                continue
            for di in range(-R, R + 1):
                x0, x1 = max(0, -di), min(W, W - di)
                if x0 >= x1:
                    continue
                dst = (slice(y0, y1), slice(x0, x1))
                src = (slice(y0 + dj, y1 + dj), slice(x0 + di, x1 + di))
                for s in range(n):
                    ax = np.abs(f32(di) + (off[s][src][..., 0] - f32(0.5)))
                    ay = np.abs(f32(dj) + (off[s][src][..., 1] - f32(0.5)))
                    inside = (ax <= rad) & (ay <= rad)
                    w = (f(np.where(inside, ax, f32(0))) * f(np.where(inside, ay, f32(0)))).astype(f32)
                    use = inside & (w != 0)
                    color[dst] = np.where(use[..., None], color[dst] + w[..., None] * samples[s][src], color[dst])
                    wsum[dst] = np.where(use, wsum[dst] + w, wsum[dst])
        mean = (color * (f32(1) / wsum)[..., None]).astype(f32)
    return color, wsum, mean
