"""The 8-bit image from the device (spt_film_read_rgb8, k_pack_rgb8), byte for byte against spt.film_to_rgb8 - color_to_rgb of
the reference (src/core/film.rs:94-99) on the host - of the film's own float read-out."""
import os
import subprocess

import numpy as np
import pytest

import _rgb8_values as V
import _util

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 4


@pytest.fixture(scope="module")
def spt():
    pkg = _util.load_pkg()
    _util.ensure_cpu_build()
    return pkg


def _scene(spt, name):
    return spt.load_scene(os.path.join(_util.SCENES, name))


# ---- the seam: k_pack_rgb8 alone -------------------------------------------------------------------------------------------

def test_seam_all_values(spt):
    hand, patterns = V.hand_values(), V.bit_patterns()
    full = np.concatenate([hand, patterns])
    for x in (hand, patterns, full):
        got = spt.debug_pack_rgb8(x)
        want = V.host_rgb8(spt, x)
        assert got.dtype == np.uint8 and np.array_equal(got, want), [(hex(int(b)), int(g), int(w)) for b, g, w in
                                                                     zip(x.view(np.uint32), got, want) if g != w][:8]
    assert np.array_equal(V.host_rgb8(spt, full), V.rgb8_numpy(full))     # (the host reference is the stated expression)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 255, 256, 257, 65536])
def test_seam_lengths(spt, n):
    """One float, the tail lane alone (1 .. 3), one whole lane, a lane and a tail, around a lane-group and a block boundary."""
    full = np.concatenate([V.hand_values(), V.bit_patterns()])
    # windows that start on the hand-made values, just before the infinities / NaNs of the bit patterns, and at the sign change
    for start in (0, V.hand_values().size - 3, V.hand_values().size + 0x7f7e, V.hand_values().size + 0x7fff):
        x = np.resize(full[start:], n) if start + n > full.size else full[start:start + n]
        got = spt.debug_pack_rgb8(x)
        assert got.shape == (n,) and np.array_equal(got, V.host_rgb8(spt, x)), (n, start)
    assert spt.debug_pack_rgb8(np.zeros(0, np.float32)).size == 0


# ---- films -----------------------------------------------------------------------------------------------------------------

def _float_reads(film, guide):
    return dict(mean=film.mean(), mon=film.robust_mean("mon"), gmon=film.robust_mean("gmon"), denoised=film.denoise(guide))


def _state(film):
    return [film.sum(), film.sum_sq(), film.bucket_sums()]


def _same(a, b):
    return all(_util.same_words(x, y) for x, y in zip(a, b))


def _check_reads(spt, film, guide):
    """read_rgb8 of the four sources = film_to_rgb8 of the four float reads; the film is the bits it was."""
    before, floats = _state(film), _float_reads(film, guide)
    for source, want in floats.items():
        got = film.read_rgb8(source, guide) if source == "denoised" else film.read_rgb8(source)
        assert got.dtype == np.uint8 and got.shape == want.shape
        assert np.array_equal(got, spt.film_to_rgb8(want)), (source, film.samples)
    again = _float_reads(film, guide)
    assert all(_util.same_words(floats[k], again[k]) for k in floats) and _same(_state(film), before)
    return floats


def test_film_read_outs(spt):
    sc = _scene(spt, "t_materials.json")
    r = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RANDOM, spp=24, seed=5)
    cfg = spt.OutputConfig(64, 48, None, "main")
    with r.progressive(sc, cfg, moments=True, buckets=9) as film, r.guide_film(sc, cfg) as guide:
        guide.render(8)
        seen = []
        for n in (7, 9, 8):
            film.render(n)
            seen.append(_check_reads(spt, film, guide))
        assert film.samples == 24
        assert not np.array_equal(spt.film_to_rgb8(seen[0]["mean"]), spt.film_to_rgb8(seen[2]["mean"]))
        assert not np.array_equal(spt.film_to_rgb8(seen[2]["mean"]), spt.film_to_rgb8(seen[2]["denoised"]))
        # the denoiser's parameters and a missing guide go through
        kw = dict(iterations=3, k_color=0.75)
        assert np.array_equal(film.read_rgb8("denoised", guide, **kw), spt.film_to_rgb8(film.denoise(guide, **kw)))
        assert np.array_equal(film.read_rgb8("denoised"), spt.film_to_rgb8(film.denoise()))
    sc.close()


def test_film_read_outs_of_an_adaptive_film(spt):
    sc = _scene(spt, "t_materials.json")
    r = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RANDOM, spp=24, seed=5)
    cfg = spt.OutputConfig(64, 48, None, "main")
    with r.progressive(sc, cfg, moments=True, buckets=9) as film, r.guide_film(sc, cfg) as guide:
        guide.render(8)
        for n in (7, 9):
            film.render(n)
            done = film.samples                             # a tolerance that retires about 40 % of the noisy active pixels
            m, sd = film.mean().astype(np.float64), np.sqrt(film.variance_of_mean().astype(np.float64))
            with np.errstate(divide="ignore", invalid="ignore"):
                need = np.max(sd / np.abs(m), axis=-1)
            need = need[(film.sample_counts() == done) & np.isfinite(need) & (need > 0)]
            film.adapt(float(np.quantile(need, 0.4)) if need.size else 0.0, 0.0, 4)
            _check_reads(spt, film, guide)
        film.render(8)
        counts = film.sample_counts()
        assert counts.min() < 24 and counts.max() == 24 and len(np.unique(counts)) > 2, np.unique(counts)   # some retired, not all
        _check_reads(spt, film, guide)
        assert np.array_equal(film.sample_counts(), counts)
    sc.close()


def test_film_read_outs_other_layouts(spt):
    """A box radius other than 0.5 (k_finish_box with wsum), a shard's packed rows, a film of libspt_hip_bez.so (the forwarder,
    both inner handles), a film without rows."""
    sc, bez = _scene(spt, "cfg2_cube.json"), _scene(spt, "t_bezier.json")
    r = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RANDOM, spp=8, seed=5)
    with spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RANDOM, spp=8, seed=5, filter_radius=0.3).progressive(sc, spt.OutputConfig(45, 31)) as box:
        box.render(5)
        assert np.array_equal(box.read_rgb8(), spt.film_to_rgb8(box.mean()))
    with r.progressive(sc, spt.OutputConfig(45, 31), shard_index=1, shard_count=3, strip_rows=4, buckets=3) as shard:
        shard.render(8)
        for source in ("mean", "mon", "gmon"):
            want = shard.mean() if source == "mean" else shard.robust_mean(source)
            assert np.array_equal(shard.read_rgb8(source), spt.film_to_rgb8(want)), source
    with r.progressive(sc, spt.OutputConfig(45, 8), shard_index=2, shard_count=3, strip_rows=4) as empty:
        assert empty.rows == 0
        empty.render(2)
        assert empty.read_rgb8().shape == (0, 45, 3)
    cfg_b = spt.OutputConfig(48, 32, None, "main")
    with r.progressive(bez, cfg_b, moments=True, buckets=3) as film, r.guide_film(bez, cfg_b) as guide:
        film.render(8)
        guide.render(4)
        _check_reads(spt, film, guide)
    sc.close()
    bez.close()


def _refused(spt, status, call):
    with pytest.raises(spt.SptError) as e:
        call()
    assert e.value.status == status, (e.value.status, str(e.value))
    return e.value.status


def test_film_refusals(spt):
    sc, bez = _scene(spt, "t_materials.json"), _scene(spt, "t_bezier.json")
    r = spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RANDOM, spp=24, seed=5)
    cfg = spt.OutputConfig(64, 48, None, "main")
    lib = spt.hip_lib()
    out8 = np.zeros((48, 64, 3), np.uint8)
    with r.progressive(sc, cfg, moments=True, buckets=9) as film, r.progressive(sc, cfg, moments=True, buckets=9) as alone, \
            r.guide_film(sc, cfg) as guide:
        guide.render(8)
        # a robust source at done == 0, the mean too: the float call's status
        for source, float_call in (("mon", lambda: film.robust_mean("mon")), ("gmon", lambda: film.robust_mean("gmon")), ("mean", film.mean)):
            assert _refused(spt, INVALID, lambda: film.read_rgb8(source)) == _refused(spt, INVALID, float_call)
        film.render(1)
        alone.render(1)
        # denoised with fewer than 2 samples (on the film, on the guide)
        assert _refused(spt, INVALID, lambda: film.read_rgb8("denoised", guide)) == _refused(spt, INVALID, lambda: film.denoise(guide))
        with r.guide_film(sc, cfg) as young_guide:
            young_guide.render(1)
            film.render(6)
            alone.render(6)
            assert _refused(spt, INVALID, lambda: film.read_rgb8("denoised", young_guide)) == _refused(spt, INVALID, lambda: film.denoise(young_guide))
        _refused(spt, INVALID, lambda: film.read_rgb8("denoised", film))
        _refused(spt, INVALID, lambda: film.read_rgb8("denoised", guide, iterations=9))
        # a robust source without buckets; the denoiser without moments
        with r.progressive(sc, cfg) as plain:
            plain.render(4)
            for source in ("mon", "gmon"):
                assert _refused(spt, INVALID, lambda: plain.read_rgb8(source)) == _refused(spt, INVALID, lambda: plain.robust_mean(source))
            assert _refused(spt, INVALID, lambda: plain.read_rgb8("denoised")) == _refused(spt, INVALID, plain.denoise)
            assert np.array_equal(plain.read_rgb8(), spt.film_to_rgb8(plain.mean()))
        # a box radius other than 0.5 and a shard of several: the denoiser's SPT_ERR_UNSUPPORTED
        with spt.PathTracer(max_depth=5, sampler=spt.SAMPLER_RANDOM, spp=24, seed=5, filter_radius=0.3).progressive(sc, cfg, moments=True) as box:
            box.render(4)
            assert _refused(spt, UNSUPPORTED, lambda: box.read_rgb8("denoised")) == _refused(spt, UNSUPPORTED, box.denoise)
        # an unknown source, null arguments
        assert lib.spt_film_read_rgb8(film._handle(), 4, None, None, out8.ctypes.data) == INVALID
        assert lib.spt_film_read_rgb8(film._handle(), 0xffffffff, None, None, out8.ctypes.data) == INVALID
        assert lib.spt_film_read_rgb8(film._handle(), 0, None, None, None) == INVALID
        assert lib.spt_film_read_rgb8(None, 0, None, None, out8.ctypes.data) == INVALID
        # a guide of the other library
        cfg_b = spt.OutputConfig(64, 48, None, "main")
        with r.guide_film(bez, cfg_b) as fwd_guide:
            fwd_guide.render(4)
            assert _refused(spt, INVALID, lambda: film.read_rgb8("denoised", fwd_guide)) == _refused(spt, INVALID, lambda: film.denoise(fwd_guide))
        # after all of that the film continues to the bits of an undisturbed one
        assert _same(_state(film), _state(alone))
        film.render(9)
        alone.render(9)
        assert _same(_state(film), _state(alone))
        assert np.array_equal(film.read_rgb8("gmon"), alone.read_rgb8("gmon")) and np.array_equal(film.read_rgb8("denoised", guide), alone.read_rgb8("denoised", guide))
        _check_reads(spt, film, guide)
    sc.close()
    bez.close()


# ---- the command line ---------------------------------------------------------------------------------------------------------

def test_cli_files_equal_the_binding_s(spt, tmp_path):
    scene, renderer = os.path.join(_util.SCENES, "cfg2_cube.json"), os.path.join(_util.SCENES, "pt.json")
    w, h, spp = 64, 64, 16
    base = ["-s", scene, "-r", renderer, "-w", str(w), "-h", str(h), "--spp", str(spp), "--seed", "3"]
    plain, dn, noisy = tmp_path / "plain.png", tmp_path / "dn.png", tmp_path / "noisy.png"
    exe = os.path.join(spt.LIB_DIR, "spt")
    res = subprocess.run([exe] + base + ["-o", str(plain)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    res = subprocess.run([exe] + base + ["-o", str(dn), "--preview-every", "6", "--denoise", "--noisy-out", str(noisy)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    sc = spt.load_scene(scene)
    ren = spt.load_renderer(renderer, seed=3)
    ren.spp = spp
    cfg = spt.OutputConfig(w, h)
    want = tmp_path / "want.png"
    spt.write_png(str(want), ren.render_shard(sc, cfg))
    assert plain.read_bytes() == want.read_bytes()
    with ren.progressive(sc, cfg, moments=True) as film, ren.guide_film(sc, cfg) as guide:
        guide.render(16)                                    # the CLI's default --guide-samples, before the first increment
        for n in (6, 6, 4):
            film.render(n)
        spt.write_png(str(want), film.denoise(guide))
        assert dn.read_bytes() == want.read_bytes()
        spt.write_png(str(want), film.mean())
        assert noisy.read_bytes() == want.read_bytes()
        assert dn.read_bytes() != noisy.read_bytes()
    sc.close()
