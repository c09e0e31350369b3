"""What a film over several devices (spt_host_multi_film_*, MultiDevice.progressive) costs next to the single-device film, on one MI355X.

One box has one device, so the multi films here run on [0] (one worker: the fan-out's own overhead) and on [0, 0] (two workers
that SHARE the device: a rehearsal of the plumbing - two scene replicas, two streams, two shard films - not a speed-up; a scaling
curve needs a multi-GPU node).  The comparison basis is the single-device ProgressiveFilm of the same tree in the same process;
the variants alternate, REPEATS rounds after one warm-up round, median per variant, host clocks around the synchronous calls.

  render     cfg2_cube 1024x1024 @ 256 spp in 8 increments of 32 samples (moments, 5 buckets): the whole loop
  read-outs  per read-out (mean, variance of the mean, counts after an adapt, gmon, rgb8 of the mean): the single film's read
             against the shard reads plus the scatter into the full image
  denoise    MultiFilm.denoise_job with a normal guide (gather of four images + upload + filter) against
             ProgressiveFilm.denoise_job on one device, f32 and rgb8, 5 iterations

  python tools/multi_film_cost.py [--json profiles/multi_film_cost.json] [--repeats 5]
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
spt = importlib.import_module("simple-path-tracer_amd")

import numpy as np

W = H = 1024
SPP, INCREMENTS, REPEATS, BUCKETS = 256, 8, 5, 5
LAYOUTS = {"multi_[0]": [0], "multi_[0,0]": [0, 0]}


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def alternate(variants, repeats):
    """variants: {name: fn returning ms}.  One warm-up round, then `repeats` rounds that run every variant once, in order."""
    for fn in variants.values():
        fn()
    ms = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            ms[k].append(fn())
    return {k: {"median_ms": round(float(np.median(v)), 3), "samples_ms": [round(x, 3) for x in v]} for k, v in ms.items()}


def same(a, b):
    if a.dtype != np.float32:
        return bool(np.array_equal(a, b))
    nan = np.isnan(b)
    return bool(np.array_equal(nan, np.isnan(a)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--repeats", type=int, default=REPEATS)
    args = ap.parse_args()
    sc = spt.load_scene(os.path.join(ROOT, "scenes_amd", "cfg2_cube.json"))
    r = spt.load_renderer(os.path.join(ROOT, "scenes_amd", "pt.json"), seed=1)
    r.sampler, r.spp = 0, SPP
    cfg = spt.OutputConfig(W, H)
    multis = {name: spt.MultiDevice(sc, devs) for name, devs in LAYOUTS.items()}
    make = {"single": lambda **kw: r.progressive(sc, cfg, **kw)}
    for name, md in multis.items():
        make[name] = (lambda md: lambda **kw: md.progressive(r, cfg, **kw))(md)
    out = {"workload": "cfg2_cube %dx%d, random sampler, %d spp in %d increments of %d, moments, %d buckets" % (W, H, SPP, INCREMENTS, SPP // INCREMENTS, BUCKETS),
           "note": "multi_[0,0] is two workers time-sharing ONE device: a rehearsal of the plumbing, not a speed-up"}

    # 1. the render loop
    def loop(mk):
        def run():
            with mk(moments=True, buckets=BUCKETS) as film:
                return clock(lambda: [film.render(SPP // INCREMENTS) for _ in range(INCREMENTS)])
        return run
    out["render_loop_ms"] = alternate({k: loop(mk) for k, mk in make.items()}, args.repeats)

    # 2. and 3.: films that stay open, half way through the plan, one adapt behind them
    films = {k: mk(moments=True, buckets=BUCKETS) for k, mk in make.items()}
    guides = {k: mk(moments=True, flags=spt.RENDER_DEBUG_NORMAL) for k, mk in make.items()}
    for k in films:
        films[k].render(SPP // 2)
        films[k].adapt(0.02, 0.0, 16)
        guides[k].render(16)
    reads = {"mean": lambda f: f.mean(), "variance_of_mean": lambda f: f.variance_of_mean(), "sample_counts": lambda f: f.sample_counts(),
             "robust_gmon": lambda f: f.robust_mean("gmon"), "rgb8_mean": lambda f: f.read_rgb8("mean")}
    out["read_out_ms"], identical = {}, True
    for name, fn in reads.items():
        want = fn(films["single"])
        identical = identical and all(same(fn(films[k]), want) for k in multis)
        out["read_out_ms"][name] = alternate({k: (lambda f: lambda: clock(lambda: fn(f)))(films[k]) for k in films}, args.repeats)
    out["denoise_ms"] = {}
    for name, kw in (("f32", {}), ("rgb8", dict(rgb8=True))):
        want = films["single"].denoise_job(guide=guides["single"], **kw)
        identical = identical and all(same(films[k].denoise_job(guide=guides[k], **kw), want) for k in multis)
        out["denoise_ms"][name] = alternate({k: (lambda k: lambda: clock(lambda: films[k].denoise_job(guide=guides[k], **kw)))(k) for k in films}, args.repeats)
    # the parts of the multi denoise: the gather alone (four full-image reads) and spt_denoise_image alone on gathered arrays
    f, g = films["multi_[0,0]"], guides["multi_[0,0]"]
    arrays = [f.mean(), f.variance_of_mean(), g.mean(), g.variance_of_mean()]
    out["denoise_parts_ms"] = alternate({
        "gather_four_images_[0,0]": lambda: clock(lambda: (f.mean(), f.variance_of_mean(), g.mean(), g.variance_of_mean())),
        "denoise_image_alone": lambda: clock(lambda: spt.denoise_image(sc, arrays[0], arrays[1], guide=(arrays[2], arrays[3])))}, args.repeats)
    out["every_multi_result_identical_to_single"] = identical
    for d in (films, guides):
        for film in d.values():
            film.close()
    for md in multis.values():
        md.close()
    sc.close()
    print(json.dumps(out, indent=1))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
    if not identical:
        sys.exit("a multi film's result differs from the single film's")


if __name__ == "__main__":
    main()
