"""The read-out of a film that keeps its samples (SPT_FILM_KEEP_SAMPLES, include/spt_abi.h), restated in float32 numpy.

Film::filter_pixel (reference src/core/film.rs:71-92) with BoxFilter (src/filter/boxf.rs) over kept samples:

    color = 0; weight_sum = 0
    for dj = -R .. R, for di = -R .. R (pixels outside the image skipped), for the pixel's samples in increasing plan index:
        color += x;  weight_sum += 1.0f if |di + (ox - 0.5)| <= radius and |dj + (oy - 0.5)| <= radius else 0.0f
    mean = color * (1.0f / weight_sum)

with R = ceil(radius - 0.5).  Every addition is one rounded f32 operation (numpy does not contract); the loops over the output
pixels are vectorised, the loops the specification orders are not.
"""
import numpy as np

import _util

f32 = np.float32


def radius_int(radius):
    return int(np.ceil(f32(radius) - f32(0.5)))


def offsets(spt, seed, width, height, spp, sampler, first, count):
    """(count, height, width, 2) f32: the pixel offsets of the plan's samples first .. first + count - 1, from the oracle's RNG
    stream (random sampler) or its R2 sequence (recurrence sampler, which reads the plan's spp)."""
    lib = _util.oracle_lib()
    off = np.zeros((count, height, width, 2), dtype=f32)
    for j in range(height):
        for i in range(width):
            px = j * width + i
            if sampler == spt.SAMPLER_RECURRENCE:
                buf = np.zeros(2 * (first + count), dtype=f32)
                lib.oracle_r2_offsets(px, spp, first + count, buf.ctypes.data)
                off[:, j, i] = buf.reshape(first + count, 2)[first:]
            else:
                assert sampler == spt.SAMPLER_RANDOM
                for s in range(count):
                    buf = np.zeros(2, dtype=f32)
                    lib.oracle_rng_stream(seed, px, first + s, 2, buf.ctypes.data)
                    off[s, j, i] = buf
    return off


def filter_film(samples, off, radius):
    """samples (n, H, W, 3) f32 and their offsets (n, H, W, 2) -> (color, weight_sum, mean) of every pixel of the image."""
    samples = np.asarray(samples, dtype=f32)
    off = np.asarray(off, dtype=f32)
    n, H, W, _ = samples.shape
    R = radius_int(radius)
    rad = f32(radius)
    color = np.zeros((H, W, 3), dtype=f32)
    wsum = np.zeros((H, W), dtype=f32)
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
                color[dst] = color[dst] + samples[s][src]
                wx = f32(di) + (off[s][src][..., 0] - f32(0.5))
                wy = f32(dj) + (off[s][src][..., 1] - f32(0.5))
                w = np.where((np.abs(wx) <= rad) & (np.abs(wy) <= rad), f32(1), f32(0))
                wsum[dst] = wsum[dst] + w
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = (color * (f32(1) / wsum)[..., None]).astype(f32)
    return color, wsum, mean
