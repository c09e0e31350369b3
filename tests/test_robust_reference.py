"""The float32 restatement of bucketed films (tests/_robust_ref.py): hand-checkable properties, and its two read-outs on the
single samples of the CPU oracle.

On t_materials (camera main, 96x72, max_depth 5, random sampler) the 2048 samples of seed 77 hold two pixels with one sample each
that is not finite: the plain mean is not finite there, the median of the bucket means (MON) and the Gini-adaptive trimmed mean
(GMON) are finite everywhere.  Against that mean, over the pixels finite in both, 64 samples of seed 5 in 9 buckets have the RMSE
0.366 (plain mean), 0.345 (MON) and 0.303 (GMON); the test asserts the order of the first and the last only.
"""
import os

import numpy as np
import pytest

import _robust_ref as R
import _util

spt = _util.load_pkg()
f32 = np.float32


def _pixels(means):
    """Bucket sums (k, 1, n, 3) of n pixels whose buckets hold one sample each: the sums are the means."""
    b = np.asarray(means, dtype=np.float32).T          # (k, n)
    return np.repeat(b[:, None, :, None], 3, axis=3)


def test_hand_checks():
    b = _pixels([[0, 0, 0, 0, 10], [1, 1, 1, 1, 1]])
    s = b.sum(axis=0)
    a = R.sorted_keys(b, 0, 5)
    assert R.trim(a)[0, :, 0].tolist() == [1, 0]
    # G of the first pixel: 2 * (5 * 10) / (5 * 10) - 6 / 5 = 0.8, t = (uint32_t)(0.8 * 2) = 1: the three middle keys, all 0
    gmon, mon = R.robust(b, s, 0, 5, R.GMON), R.robust(b, s, 0, 5, R.MON)
    assert gmon[0, 0].tolist() == [0, 0, 0] and mon[0, 0].tolist() == [0, 0, 0]
    assert (s[0, 0] * f32(0.2)).tolist() == [2, 2, 2]                    # the plain mean
    assert gmon[0, 1].tolist() == [1, 1, 1] and mon[0, 1].tolist() == [1, 1, 1]


def test_permuting_the_buckets_changes_no_bit():
    rng = np.random.default_rng(3)
    k = 9
    b = rng.gamma(0.3, 2.0, size=(k, 6, 7, 3)).astype(np.float32)
    b[4, 2, 3] = f32(500.0)                                               # a firefly
    s = b.sum(axis=0, dtype=np.float32)
    n = 3 * k                                                             # every bucket holds 3 samples, whatever the order
    for est in (R.MON, R.GMON):
        ref = R.robust(b, s, 0, n, est)
        for _ in range(4):
            got = R.robust(b[rng.permutation(k)], s, 0, n, est)
            assert _util.same_words(got, ref)
    assert R.trim(R.sorted_keys(b, 0, n))[2, 3, 0] >= 1


def test_a_bucket_that_is_not_finite_is_trimmed():
    for bad in (np.nan, np.inf):
        b = _pixels([[1, 2, 3, 4, 5, 6, 7, 8, bad]])[[8, 0, 1, 2, 3, 4, 5, 6, 7]]
        s = b.sum(axis=0)
        a = R.sorted_keys(b, 0, 9)
        assert np.isposinf(a[8]).all() and (R.trim(a) == 4).all()
        for est in (R.MON, R.GMON):
            assert R.robust(b, s, 0, 9, est)[0, 0].tolist() == [5, 5, 5]   # a_4 of (1 .. 8, +inf)
        assert not np.isfinite(s).any()


def test_all_zero_buckets_give_zero():
    b = np.zeros((5, 2, 3, 3), dtype=np.float32)
    for est in (R.MON, R.GMON):
        out = R.robust(b, b[0], 0, 10, est)
        assert not out.any() and not np.signbit(out).any()


def test_fewer_samples_than_buckets_give_the_plain_mean():
    rng = np.random.default_rng(5)
    xs = [rng.random((2, 4, 3), dtype=np.float32) for _ in range(4)]
    b = R.bucket_sums(xs, 3, 5)
    s = np.zeros_like(xs[0])
    for x in xs:
        s = s + x
    counts = np.array([[1, 2, 3, 4], [4, 4, 4, 4]])                      # (as if every pixel had stopped there: all below K)
    for est in (R.MON, R.GMON):
        assert _util.same_words(R.robust(b, s, 3, 4, est), s * f32(0.25))
        got = R.robust(b, s, 3, counts, est)
        assert _util.same_words(got, (s * (f32(1) / counts.astype(np.float32))[..., None]).astype(np.float32))


def test_counts():
    assert R.bucket_counts(7, 20, 5).tolist() == [4, 4, 4, 4, 4]
    assert R.bucket_counts(3, 7, 5).tolist() == [1, 1, 1, 2, 2]
    per_pixel = R.bucket_counts(3, np.array([[7, 0], [1, 12]]), 5)
    assert per_pixel.shape == (5, 2, 2)
    assert per_pixel[:, 0, 0].tolist() == [1, 1, 1, 2, 2] and per_pixel[:, 0, 1].tolist() == [0] * 5
    assert per_pixel[:, 1, 0].tolist() == [0, 0, 0, 1, 0] and per_pixel[:, 1, 1].tolist() == [2, 2, 2, 3, 3]
    for first, n, k in ((0, 1, 3), (11, 64, 9), (5, 29, 15)):
        brute = [sum(1 for s in range(first, first + n) if s % k == j) for j in range(k)]
        assert R.bucket_counts(first, n, k).tolist() == brute


def test_bucket_sums_follow_the_plan_index():
    xs = [np.full((1, 1, 3), f32(10 ** i)) for i in range(7)]
    b = R.bucket_sums(xs, 3, 5)                                           # plan indices 3 .. 9: buckets 3 4 0 1 2 3 4
    assert b[:, 0, 0, 0].tolist() == [100.0, 1000.0, 10000.0, 100001.0, 1000010.0]


# ---- on the oracle's single samples ---------------------------------------------------------------------------------------------

W, H, DEPTH, K = 96, 72, 5, 9


def _oracle_film(sc, spp, seed):
    """S and the K bucket sums of the whole plan, from the oracle's single samples (a chunk at a time)."""
    r = spt.PathTracer(max_depth=DEPTH, sampler=spt.SAMPLER_RANDOM, spp=spp, seed=seed)
    s = np.zeros((H, W, 3), dtype=np.float32)
    b = np.zeros((K, H, W, 3), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for first in range(0, spp, 128):
            xs = _util.oracle_render_samples(sc, r, W, H, first, min(128, spp - first), camera="main", flags=_util.ORACLE_DEVICE)
            for i, x in enumerate(xs):
                s = s + x
                b[(first + i) % K] = b[(first + i) % K] + x
    return s, b


@pytest.fixture(scope="module")
def materials():
    _util.ensure_cpu_build()
    sc = spt.load_scene(os.path.join(_util.SCENES, "t_materials.json"))
    long_film = _oracle_film(sc, 2048, 77)
    short_film = _oracle_film(sc, 64, 5)
    sc.close()
    return long_film, short_film


def test_one_bad_sample_spoils_a_bucket_not_the_pixel(materials):
    (s, b), _ = materials
    mean = s * (f32(1) / f32(2048))
    bad = ~np.isfinite(mean).all(axis=-1)
    print("pixels whose plain mean is not finite: %d" % bad.sum())
    assert bad.sum() >= 1
    for est in (R.MON, R.GMON):
        out = R.robust(b, s, 0, 2048, est)
        print("estimator %d: pixels that are not finite: %d" % (est, (~np.isfinite(out).all(axis=-1)).sum()))
        assert np.isfinite(out).all()


def test_gmon_is_closer_to_the_reference_than_the_mean(materials):
    (s_ref, _), (s, b) = materials
    ref = s_ref * (f32(1) / f32(2048))
    mean = s * (f32(1) / f32(64))
    gmon, mon = R.robust(b, s, 0, 64, R.GMON), R.robust(b, s, 0, 64, R.MON)
    ok = np.isfinite(ref).all(axis=-1) & np.isfinite(mean).all(axis=-1) & np.isfinite(gmon).all(axis=-1) & np.isfinite(mon).all(axis=-1)

    def rmse(img):
        return float(np.sqrt(np.mean((img[ok].astype(np.float64) - ref[ok].astype(np.float64)) ** 2)))
    print("RMSE against 2048 samples: plain mean %.4f, MON %.4f, GMON %.4f (%d pixels left out)" % (rmse(mean), rmse(mon), rmse(gmon), (~ok).sum()))
    assert rmse(gmon) < rmse(mean)
