"""The numpy restatement of the weighted read-out (tests/_filter_ref.py) against facts that do not depend on it.  This checks the
reference, not the library: it runs no code of the film and needs no GPU (exp goes through the CPU oracle)."""
import math

import numpy as np
import pytest

import _filter_ref as ref
import _util

f32 = np.float32
FILTERS = [("tent", 1.0, {}), ("tent", 0.5, {}), ("gaussian", 1.5, {"alpha": 2.0}), ("mitchell", 2.0, {"b": 1.0 / 3.0, "c": 1.0 / 3.0})]


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    _util.ensure_cpu_build()


def _ulps(a, b):
    return abs(float(a) - float(b)) / float(np.spacing(f32(abs(b))))


def test_radius_int():
    assert [ref.radius_int(r) for r in (0.2, 0.5, 0.51, 1.0, 1.5, 1.51, 2.0, 2.5)] == [0, 0, 1, 1, 1, 2, 2, 2]


def test_mitchell_one_third():
    f = ref.filter_fn("mitchell", 2.0)
    # t = a at radius 2.  f(0) = q0 = (6 - 2B) / 6 = 8/9: one rounding of B, one of the coefficient
    assert _ulps(f(f32(0.0)), 8.0 / 9.0) <= 4
    # Both pieces at t = 1 are B / 6 + C = 1/18 in exact arithmetic, and the outer piece at t = 2 is 0.  The Horner steps round
    # at the size of their intermediates, which stay below 4 (|c1| = 10/3): a few ulp means a few spacings of f32 in [2, 4)
    tol = 4 * float(np.spacing(f32(2.0)))
    c3, c2, c1, c0, q3, q2, q0 = ref.mitchell_coefficients(1.0 / 3.0, 1.0 / 3.0)
    one = f32(1.0)
    outer_1 = ((c3 * one + c2) * one + c1) * one + c0
    inner_1 = ((q3 * one + q2) * one) * one + q0
    assert abs(float(outer_1) - float(inner_1)) <= tol and abs(float(inner_1) - 1.0 / 18.0) <= tol
    assert float(f(f32(1.0))) == float(inner_1)                  # t == 1 takes the inner piece
    assert abs(float(f(f32(2.0)))) <= tol
    assert float(f(f32(1.5))) < 0.0                              # the negative lobe is kept


def test_mitchell_coefficients_in_double():
    got = ref.mitchell_coefficients(1.0 / 3.0, 1.0 / 3.0)
    want = (-7.0 / 18.0, 2.0, -10.0 / 3.0, 16.0 / 9.0, 7.0 / 6.0, -2.0, 8.0 / 9.0)
    for g, w in zip(got, want):
        assert g.dtype == np.float32 and _ulps(g, w) <= 2


def test_gaussian_is_zero_at_the_radius():
    for r, alpha in ((1.5, 2.0), (1.0, 0.5), (2.5, 3.0)):
        f = ref.filter_fn("gaussian", r, alpha=alpha)
        assert float(f(f32(r))) == 0.0
        assert float(f(f32(0.0))) > 0.0
        a = np.linspace(0, r, 50, dtype=f32)
        assert (f(a) >= 0).all() and (np.diff(f(a)) <= 0).all()


def test_tent_is_symmetric():
    # an impulse in the middle, every offset at the pixel centre or mirrored about it in eighths (exact in f32): the filtered
    # image is its own mirror image
    H, W, n = 7, 9, 4
    samples = np.zeros((n, H, W, 3), dtype=f32)
    samples[:, 3, 4] = 1.0
    off = np.full((n, H, W, 2), 0.5, dtype=f32)
    off[0, ..., 0], off[1, ..., 0] = 0.125, 0.875
    off[2, ..., 1], off[3, ..., 1] = 0.25, 0.75
    color, wsum, mean = ref.filter_film(samples, off, "tent", 1.5)
    assert color.max() > 0
    assert np.array_equal(color, color[::-1]) and np.array_equal(color, color[:, ::-1])
    assert np.array_equal(wsum, wsum[::-1]) and np.array_equal(wsum, wsum[:, ::-1])
    f = ref.filter_fn("tent", 1.5)
    assert float(f(f32(0.375))) == 1.125


@pytest.mark.parametrize("kind,radius,params", FILTERS)
def test_a_constant_image_stays_constant(kind, radius, params):
    # Constants that are powers of two: w * c is exact, so the colour chain is the wsum chain scaled by c, rounding for rounding,
    # and what is left is 1 / wsum and one product: at most 1.5 ulp.  The bound of 4 ulp holds with room.
    rng = np.random.default_rng(3)
    n, H, W = 5, 6, 8
    const = np.array([0.5, 2.0, 0.25], dtype=f32)
    samples = np.broadcast_to(const, (n, H, W, 3)).copy()
    off = rng.random((n, H, W, 2), dtype=f32)
    color, wsum, mean = ref.filter_film(samples, off, kind, radius, **params)
    assert (wsum > 0).all()
    err = np.abs(mean.astype(np.float64) - const) / np.spacing(const).astype(np.float64)
    assert err.max() <= 4, err.max()


@pytest.mark.parametrize("kind,radius,params", [("tent", 0.5, {}), ("gaussian", 0.5, {"alpha": 2.0})])
def test_a_constant_that_is_no_power_of_two(kind, radius, params):
    # One sample per pixel and Rf = 0: color = fl(w * c), wsum = w, mean = fl(color * fl(1 / w)) - three roundings, each at most
    # 2^-24 relative, and 2^-24 |x| is below one ulp of x: under 4 ulp for any constant.  (With n contributing samples the chains
    # add 2 (n - 1) roundings, which no bound of 4 ulp covers for an arbitrary constant: those cases use powers of two, above.)
    rng = np.random.default_rng(5)
    H, W = 6, 8
    const = np.array([0.3, 1.7, 0.05], dtype=f32)
    samples = np.broadcast_to(const, (1, H, W, 3)).copy()
    off = (0.25 + 0.5 * rng.random((1, H, W, 2))).astype(f32)       # inside the support of radius 0.5, away from its edge
    color, wsum, mean = ref.filter_film(samples, off, kind, radius, **params)
    assert (wsum > 0).all() and len(np.unique(wsum)) > 3
    err = np.abs(mean.astype(np.float64) - const) / np.spacing(const).astype(np.float64)
    assert err.max() <= 4, err.max()


def _f64(kind, r, alpha=2.0, b=1.0 / 3.0, c=1.0 / 3.0):
    if kind == "tent":
        return lambda a: r - a
    if kind == "gaussian":
        return lambda a: max(math.exp(-alpha * a * a) - math.exp(-alpha * r * r), 0.0)

    def mitchell(a):
        t = 2.0 * a / r
        if t > 1:
            return ((-b - 6 * c) * t ** 3 + (6 * b + 30 * c) * t ** 2 + (-12 * b - 48 * c) * t + (8 * b + 24 * c)) / 6
        return ((12 - 9 * b - 6 * c) * t ** 3 + (-18 + 12 * b + 6 * c) * t ** 2 + (6 - 2 * b)) / 6
    return mitchell


@pytest.mark.parametrize("kind,radius,params", FILTERS)
def test_against_float64(kind, radius, params):
    rng = np.random.default_rng(11)
    n, H, W = 5, 6, 8
    samples = (0.1 + rng.random((n, H, W, 3))).astype(f32)
    off = rng.random((n, H, W, 2), dtype=f32)
    color, wsum, mean = ref.filter_film(samples, off, kind, radius, **params)
    f = _f64(kind, radius, **params)
    R = max(math.ceil(radius - 0.5), 0)
    want = np.zeros((H, W, 3))
    for y in range(H):
        for x in range(W):
            acc, ws = np.zeros(3), 0.0
            for dj in range(-R, R + 1):
                for di in range(-R, R + 1):
                    if not (0 <= y + dj < H and 0 <= x + di < W):
                        continue
                    for s in range(n):
                        ax = abs(di + float(off[s, y + dj, x + di, 0]) - 0.5)
                        ay = abs(dj + float(off[s, y + dj, x + di, 1]) - 0.5)
                        if ax <= radius and ay <= radius:
                            w = f(ax) * f(ay)
                            acc += w * samples[s, y + dj, x + di].astype(np.float64)
                            ws += w
            want[y, x] = acc / ws
    assert np.abs(mean - want).max() <= 1e-5 * np.abs(want).max()
    assert np.allclose(mean, want, rtol=1e-5, atol=0)
