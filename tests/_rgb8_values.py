"""Inputs and the numpy statement of the 8-bit conversion (color_to_rgb, reference src/core/film.rs:94-99), shared by
test_rgb8_reference.py (the host's spt_host_film_to_rgb8) and test_gpu_rgb8.py (the device's k_pack_rgb8)."""
import numpy as np

f32 = np.float32


def rgb8_numpy(x):
    """c = x * 255.0f; cl = c < 0 ? 0 : (c > 255 ? 255 : c); byte = (cl != cl) ? 0 : (uint8_t)cl - one rounded f32 operation at a
    time (numpy does not contract), the conversion truncates."""
    x = np.asarray(x, dtype=f32)
    with np.errstate(invalid="ignore", over="ignore"):
        c = (x * f32(255)).astype(f32)
        cl = np.where(c < 0, f32(0), np.where(c > 255, f32(255), c))
    cl = np.where(cl != cl, f32(0), cl)                       # a NaN gives 0
    return np.trunc(cl).astype(np.uint8)                      # (in 0 .. 255 by now)


def hand_values():
    """0, -0, 1, k/255 and its two f32 neighbours, the last value below 255, values outside [0, 1], denormals, infinities and
    both NaN signs."""
    v = [0.0, -0.0, 1.0]
    for k in (1, 2, 3, 17, 64, 127, 128, 129, 200, 253, 254, 255):
        q = f32(k) / f32(255)
        v += [np.nextafter(q, f32(-1)), q, np.nextafter(q, f32(2))]
    v += [f32(254.999) / f32(255), 2.0, 1.0000001, 0.99999994, -1e-30, 1e-30, -1.0, 3.4e38, -3.4e38]
    v += [1e-45, -1e-45, 1e-39, -1e-39, 1.1754942e-38]        # denormals
    v += [np.inf, -np.inf]
    out = np.array(v, dtype=f32)
    nans = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff], dtype=np.uint32).view(f32)
    return np.concatenate([out, nans])


def bit_patterns():
    """All f32 bit patterns i << 16, i = 0 .. 65535: every sign, exponent and the top 7 mantissa bits."""
    return (np.arange(65536, dtype=np.uint32) << np.uint32(16)).view(f32)


def host_rgb8(spt, x):
    """spt.film_to_rgb8 on any number of values (it takes whole pixels: the input is padded to a multiple of 3)."""
    x = np.asarray(x, dtype=f32).reshape(-1)
    padded = np.concatenate([x, np.zeros((-x.size) % 3, dtype=f32)])
    return spt.film_to_rgb8(padded.reshape(-1, 1, 3)).reshape(-1)[:x.size]
