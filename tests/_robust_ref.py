"""Bucketed films (spt_film_buckets, spt_film_read_buckets, spt_film_read_robust) in float32 numpy, one rounded operation at a
time and in the order of spt_abi.h (numpy does not contract), so the device's bucket sums and both read-outs can be compared bit
for bit.  Sample s of the plan goes to bucket s % K; the read-outs are the median of the K bucket means (MON) and their
Gini-adaptive trimmed mean (GMON).
"""
import numpy as np

f32 = np.float32
MON, GMON = 0, 1


def bucket_sums(samples, first_sample, k):
    """B_j, (k,) + sample shape: the single samples of the plan indices first_sample, first_sample + 1, ... added in that
    order, each into bucket (plan index) % k, from +0."""
    b = np.zeros((k,) + tuple(samples[0].shape), dtype=np.float32)
    for i, x in enumerate(samples):
        j = (first_sample + i) % k
        b[j] = b[j] + x
    return b


def bucket_counts(first_sample, n, k):
    """n_j = #{ s in [first_sample, first_sample + n) : s % k == j }, integers, shape (k,) + n.shape; n: a number or one count
    per pixel."""
    n = np.asarray(n, dtype=np.int64)
    j = np.arange(k, dtype=np.int64).reshape((k,) + (1,) * n.ndim)

    def below(x):   # the s in [0, x) with s % k == j
        return x // k + (x % k > j)
    return below(first_sample + n) - below(np.int64(first_sample))


def _reciprocal(count):
    """r(c) = 1.0f / (float)c as the host rounds it (r(0) is never used: 0 stands in)."""
    c = np.asarray(count).astype(np.float32)
    return np.where(c > 0, f32(1) / np.where(c > 0, c, f32(1)), f32(0)).astype(np.float32)


def sorted_keys(b, first_sample, n):
    """a_0 <= ... <= a_{k-1}, the shape of b = (k, rows, width, 3): the bucket means, one that is not finite replaced by +inf.
    n: the samples the pixels cover (a number or (rows, width)); a bucket without samples has the key 0 * B."""
    k = b.shape[0]
    n_px = np.broadcast_to(np.asarray(n, dtype=np.int64), b.shape[1:-1])
    r = _reciprocal(bucket_counts(first_sample, n_px, k))[..., None]
    with np.errstate(invalid="ignore", over="ignore"):
        mu = (b * r).astype(np.float32)
        key = np.where(np.isfinite(mu), mu + f32(0), f32(np.inf)).astype(np.float32)
    return np.sort(key, axis=0)


def trim(a):
    """GMON's t per pixel and channel from the sorted keys a (k, ...): how many keys are dropped at either end."""
    k = a.shape[0]
    h = (k - 1) // 2
    num = np.zeros(a.shape[1:], dtype=np.float32)
    den = np.zeros(a.shape[1:], dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for i in range(k):
            num = num + f32(i + 1) * a[i]
            den = den + a[i]
        g = (f32(2) * num) / (f32(k) * den) - (f32(k + 1) / f32(k))
        gh = g * f32(h)
        positive = g > 0
        full = positive & (gh >= f32(h))
        t = np.where(positive & ~full, gh, f32(0)).astype(np.uint32).astype(np.int64)   # (uint32_t)(G * (float)h), below h
    t = np.where(full, h, t)
    t = np.where(den > 0, t, 0)
    return np.where(a[k - 1] == f32(np.inf), h, t)


def robust(b, s, first_sample, n, estimator):
    """spt_film_read_robust from the bucket sums b (k, rows, width, 3), the film's sum s (rows, width, 3) and the samples the
    pixels cover, n: a number, or (rows, width) counts of an adaptive film."""
    k = b.shape[0]
    h = (k - 1) // 2
    n_px = np.broadcast_to(np.asarray(n, dtype=np.int64), s.shape[:-1])
    a = sorted_keys(b, first_sample, n_px)
    if estimator == MON:
        res = a[h]
    else:
        t = trim(a)
        res = np.zeros(s.shape, dtype=np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            for tv in range(h + 1):
                acc = np.zeros(s.shape, dtype=np.float32)
                for i in range(tv, k - tv):
                    acc = acc + a[i]
                res = np.where(t == tv, acc * (f32(1) / f32(k - 2 * tv)), res)
    with np.errstate(invalid="ignore", over="ignore"):
        plain = (s * _reciprocal(n_px)[..., None]).astype(np.float32)
    return np.where((n_px < k)[..., None], plain, res).astype(np.float32)
