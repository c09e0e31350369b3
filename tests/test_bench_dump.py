"""bench.py --dump-outputs: what the timed path computed in its last step, written as .npy files, so that two builds of the
project can be compared output for output; and a plain bench run (no --full) carries only the headline figures."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _util


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(_util.ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_the_whole_film(tmp_path):
    bench = _bench()
    film = np.random.default_rng(3).uniform(0, 2, size=(48, 64, 3)).astype(np.float32)
    film[5, 7, 1] = np.nan
    bench.dump_outputs(str(tmp_path / "out"), film)
    assert sorted(os.listdir(tmp_path / "out")) == ["film.npy"]
    got = np.load(tmp_path / "out" / "film.npy")
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), film.view(np.uint32))


def test_dump_outputs_samples_a_film_over_the_limit(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096)
    monkeypatch.setattr(bench, "DUMP_SAMPLE_PIXELS", 100)
    film = np.random.default_rng(4).uniform(0, 2, size=(40, 30, 3)).astype(np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), film)
    assert sorted(os.listdir(tmp_path / "a")) == ["film_sample.npy", "film_sample_pixels.npy"]
    vals, idx = np.load(tmp_path / "a" / "film_sample.npy"), np.load(tmp_path / "a" / "film_sample_pixels.npy")
    assert vals.dtype == np.float32 and vals.shape == (100, 3) and idx.dtype == np.float64 and idx.shape == (100,)
    assert len(np.unique(idx)) == 100 and np.array_equal(vals, film.reshape(-1, 3)[idx.astype(np.int64)])
    # the same pixels every time: two runs of the same arguments compare sample for sample
    assert np.array_equal(idx, np.load(tmp_path / "b" / "film_sample_pixels.npy"))
    assert np.array_equal(vals, np.load(tmp_path / "b" / "film_sample.npy"))


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_film_of_its_last_timed_step(tmp_path):
    w, h, spp, steps = 128, 96, 8, 3
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(_util.ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--width", str(w), "--height", str(h), "--spp", str(spp), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["unit"] == "Msamples/s" and line["higher_is_better"] is True
    assert abs(line["value"] - w * h * spp / (line["ms_per_step"] * 1e3)) <= 0.01 * line["value"] + 0.01
    for extra in ("roofline", "secondary", "cpu_baseline", "parity", "other_configs"):   # --full only
        assert extra not in line
    film = np.load(out / "film.npy")
    assert film.dtype == np.float32 and film.shape == (h, w, 3)
    # the same render, synchronous, in this process: the dumped film is the timed path's answer bit for bit
    spt = _util.load_pkg()
    scene = spt.load_scene(os.path.join(_util.SCENES, "cfg2_cube.json"))
    r = spt.load_renderer(os.path.join(_util.SCENES, "pt.json"), seed=1)
    r.spp = spp
    ref = r.render_shard(scene, spt.OutputConfig(w, h), device=0)
    scene.close()
    assert film.max() > 0.1 and np.array_equal(film.view(np.uint32), ref.view(np.uint32))
