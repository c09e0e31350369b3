"""The 8-bit image on the host (CPU tests): spt.film_to_rgb8 pinned on hand-made values against the numpy statement of
color_to_rgb (tests/_rgb8_values.py), and the binding's own argument checks of ProgressiveFilm.read_rgb8."""
import ctypes as C

import numpy as np

import _rgb8_values as V
import _util

spt = _util.load_pkg()


def test_film_to_rgb8_on_hand_made_values():
    x = V.hand_values()
    got = V.host_rgb8(spt, x)
    want = V.rgb8_numpy(x)
    assert np.array_equal(got, want), [(float(a), int(b), int(c)) for a, b, c in zip(x, got, want) if b != c]
    # the statement itself, spelled out where it matters
    one = lambda v: int(V.host_rgb8(spt, np.array([v], dtype=np.float32))[0])
    assert one(0.0) == 0 and one(-0.0) == 0 and one(1.0) == 255 and one(2.0) == 255 and one(-1e-30) == 0
    assert one(np.inf) == 255 and one(-np.inf) == 0 and one(np.nan) == 0 and one(-np.nan) == 0
    assert one(np.float32(254.999) / np.float32(255)) == 254 and one(1e-45) == 0         # truncation, a denormal


def test_film_to_rgb8_on_all_exponents():
    x = V.bit_patterns()
    assert np.array_equal(V.host_rgb8(spt, x), V.rgb8_numpy(x))


def test_binding_argument_checks():
    """read_rgb8's own argument checks come before any device call."""
    film = spt.ProgressiveFilm.__new__(spt.ProgressiveFilm)
    film._h = C.c_void_p()                                   # a closed film: anything that reached the library would raise SptError
    for bad in (lambda: film.read_rgb8("median"), lambda: film.read_rgb8("mean", iterations=3), lambda: film.read_rgb8("mon", guide=film)):
        try:
            bad()
        except ValueError:
            continue
        raise AssertionError("accepted")
    try:
        film.read_rgb8("denoised", sigma=1.0)
    except TypeError:
        pass
    else:
        raise AssertionError("accepted")
    assert spt.READ_SOURCES == {"mean": 0, "mon": 1, "gmon": 2, "denoised": 3}
    # write_image takes the u8 image as it is
    img = np.arange(4 * 5 * 3, dtype=np.uint8).reshape(4, 5, 3)
    assert np.array_equal(spt._as_rgb8(img), img)
