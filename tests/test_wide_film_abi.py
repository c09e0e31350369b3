"""Films that keep their samples: the header and the binding agree, and the numpy restatement of the read-out
(tests/_wide_film_ref.py) is checked against the CPU oracle's general film at 1 spp, where the kept samples are the
radius-0.5 film itself.  The second part checks the reference, not the library: it runs no code of the film and needs no GPU."""
import os
import re

import numpy as np
import pytest

import _util
import _wide_film_ref as ref

spt = _util.load_pkg()
SCENE = os.path.join(_util.SCENES, "cfg2_cube.json")
W, H = 24, 18


def _header():
    return open(os.path.join(_util.ROOT, "include", "spt_abi.h")).read()


def test_header_and_binding_constants_agree():
    text = _header()
    m = re.search(r"enum\s*\{\s*SPT_FILM_MOMENTS\s*=\s*1u\s*,\s*SPT_FILM_KEEP_SAMPLES\s*=\s*2u\s*\}", text)
    assert m, "include/spt_abi.h: enum { SPT_FILM_MOMENTS = 1u, SPT_FILM_KEEP_SAMPLES = 2u }"
    assert spt.FILM_MOMENTS == 1 and spt.FILM_KEEP_SAMPLES == 2
    proto = re.search(r"spt_status\s+spt_film_read_samples\(\s*spt_film\*\s*film,\s*uint32_t\s+first,\s*uint32_t\s+count,\s*float\*\s*out\s*\);", text)
    assert proto, "include/spt_abi.h: the prototype of spt_film_read_samples"
    assert re.search(r"#define\s+SPT_ABI_VERSION\s+14\b", text) and spt.SPT_ABI_VERSION == 14      # additive: the version stays


def test_binding_has_the_keyword_and_the_read_out():
    import inspect
    assert "keep_samples" in inspect.signature(spt.PathTracer.progressive).parameters
    assert "keep_samples" in inspect.signature(spt.MultiDevice.progressive).parameters
    assert inspect.signature(spt.PathTracer.progressive).parameters["keep_samples"].default is False
    assert list(inspect.signature(spt.ProgressiveFilm.kept).parameters) == ["self", "first", "count"]


@pytest.fixture(scope="module")
def one_sample():
    """The 1-spp radius-0.5 oracle film (= the samples themselves) and the samples' offsets, once for every radius."""
    assert spt.FILM_KEEP_SAMPLES == 2          # the reference below restates what that flag's read-out computes
    _util.ensure_cpu_build()
    sc = spt.load_scene(SCENE)
    base, _ = _util.oracle_render(sc, spt.PathTracer(max_depth=4, sampler=spt.SAMPLER_RANDOM, spp=1, seed=3), W, H)
    off = ref.offsets(spt, 3, W, H, 1, spt.SAMPLER_RANDOM, 0, 1)
    return sc, base, off


@pytest.mark.parametrize("radius", [0.3, 0.8, 1.0, 1.5, 2.2])
def test_restatement_equals_the_oracle_at_one_sample(one_sample, radius):
    sc, base, off = one_sample
    want, _ = _util.oracle_render(sc, spt.PathTracer(max_depth=4, sampler=spt.SAMPLER_RANDOM, spp=1, seed=3, filter_radius=radius), W, H)
    color, wsum, mean = ref.filter_film(base[None], off, radius)
    assert np.array_equal(np.isnan(want), np.isnan(mean))           # 0 * (1 / 0) where no sample lies inside the box
    assert _util.same_words(mean, want)
    R = ref.radius_int(radius)
    assert R == {0.3: 0, 0.8: 1, 1.0: 1, 1.5: 1, 2.2: 2}[radius]
    assert wsum.max() <= (2 * R + 1) ** 2 and base.max() > 0.1
    if radius == 0.3:
        assert np.isnan(mean).any() or np.isinf(mean).any()         # some pixel's only sample lies outside a box of radius 0.3
