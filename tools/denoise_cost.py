"""What the film denoiser (spt_film_denoise) costs, on one MI355X.

For each workload: a moments film takes 16 samples, its guide (the same plan with debug_normal) 16; then a 5-iteration denoise
with and without the guide is timed next to a further 16-sample spt_film_render increment of the same film, in the same process.
Host clocks around the synchronous calls (the copy of the image to the host included), median of 5 after one warm-up call.

  python tools/denoise_cost.py [--json profiles/denoise_cost.json]
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/denoise_cost.py --trace
      the same calls once each after one warm-up call each, for the kernel times
  python tools/denoise_cost.py --pair-trace DIR/..._kernel_trace.csv [--json profiles/denoise_cost.json]
      per workload and per iteration: the kernel's time and the fraction of 6.3 TB/s that its algorithmic bytes (48 per pixel
      with a guide: two 16-byte records read, one written; 32 without; the last iteration writes 12) come to; merged into the
      JSON of the first form when it exists
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

WORKLOADS = [
    # name, scene, camera, width, height
    ("cfg2_cube", "cfg2_cube.json", None, 1024, 1024),
    ("t_materials", "t_materials.json", "main", 512, 512),
]
SPP, INCREMENT, ITERATIONS, REPEATS = 64, 16, 5, 5
HBM_BYTES_PER_S = 6.3e12


def timed(fn, repeats, warm):
    if warm:
        fn()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ms)), 4), [round(x, 4) for x in ms]


def run(only=None, repeats=REPEATS, warm=True):
    out = []
    for name, scene_name, camera, w, h in WORKLOADS:
        if only and only != name:
            continue
        sc = spt.load_scene(os.path.join(ROOT, "scenes_amd", scene_name))
        r = spt.load_renderer(os.path.join(ROOT, "scenes_amd", "pt.json"), seed=1)
        r.sampler, r.spp = 0, SPP
        cfg = spt.OutputConfig(w, h, None, camera)
        with r.progressive(sc, cfg, moments=True) as film, r.guide_film(sc, cfg) as guide:
            film.render(INCREMENT)
            guide.render(INCREMENT)
            # the order a trace is paired by: with guide, without guide, the mean, then the increments
            guided = timed(lambda: film.denoise(guide, iterations=ITERATIONS), repeats, warm)
            plain = timed(lambda: film.denoise(iterations=ITERATIONS), repeats, warm)
            mean = timed(film.mean, repeats, warm)
            inc = timed(lambda: film.render(INCREMENT), min(repeats, (SPP - INCREMENT) // INCREMENT), False)
        sc.close()
        wl = {"workload": "%s %dx%d, random sampler, %d-sample increments, %d iterations" % (name, w, h, INCREMENT, ITERATIONS),
              "name": name, "pixels": w * h,
              "denoise_with_guide_ms": guided[0], "denoise_without_guide_ms": plain[0], "film_mean_ms": mean[0], "increment_ms": inc[0],
              "denoise_with_guide_over_increment": round(guided[0] / inc[0], 4), "denoise_without_guide_over_increment": round(plain[0] / inc[0], 4),
              "samples_ms": {"with_guide": guided[1], "without_guide": plain[1], "film_mean": mean[1], "increment": inc[1]}}
        print("%s: denoise %.3f ms with guide, %.3f without; film read %.3f ms; %d-sample increment %.3f ms (ratio %.3f / %.3f)" % (
            wl["workload"], guided[0], plain[0], mean[0], INCREMENT, inc[0], wl["denoise_with_guide_over_increment"],
            wl["denoise_without_guide_over_increment"]))
        out.append(wl)
    return out


def pair_trace(csv_path):
    """The trace of `--trace`: per workload two guided calls (pack<true>, 5 atrous<true, .>) then two plain ones (pack<false>, ...);
    the first of each pair is the warm-up, the second is reported."""
    import csv
    rows = sorted(csv.DictReader(open(csv_path)), key=lambda d: int(d["Start_Timestamp"]))
    us = lambda d: (int(d["End_Timestamp"]) - int(d["Start_Timestamp"])) * 1e-3
    dn = [(d["Kernel_Name"], us(d)) for d in rows if "k_denoise" in d["Kernel_Name"]]
    per_call = 1 + ITERATIONS
    assert len(dn) == 4 * per_call * len(WORKLOADS), len(dn)
    out = []
    for k, (name, _, _, w, h) in enumerate(WORKLOADS):
        res = {"name": name}
        for j, key in enumerate(("with_guide", "without_guide")):
            first = (4 * k + 2 * j + 1) * per_call
            call = dn[first:first + per_call]
            assert "k_denoise_pack" in call[0][0] and all("k_denoise_atrous" in c[0] for c in call[1:]), [c[0] for c in call]
            assert ("<true" in call[1][0]) == (key == "with_guide"), call[1][0]
            read = 32 if key == "with_guide" else 16
            its = []
            for i, (kernel, t) in enumerate(call[1:]):
                nbytes = (read + (12 if i == ITERATIONS - 1 else 16)) * w * h
                its.append({"step": 1 << i, "kernel": "k_denoise_atrous_lds" if "_lds" in kernel else "k_denoise_atrous", "us": round(t, 2), "bytes_per_pixel": nbytes // (w * h),
                            "fraction_of_6.3_TB_per_s": round(nbytes / (t * 1e-6) / HBM_BYTES_PER_S, 4)})
            res[key] = {"pack_us": round(call[0][1], 2), "iterations": its, "kernels_us": round(sum(c[1] for c in call), 2)}
        res["note"] = "kernel times of one call each, after one warm-up call"
        out.append(res)
    print(json.dumps(out, indent=1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write (or, with --pair-trace, merge into) this file")
    ap.add_argument("--only", default=None, help="one workload by name")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--pair-trace", default=None, metavar="KERNEL_TRACE_CSV")
    args = ap.parse_args()
    if args.trace:
        run(repeats=1, warm=True)
        return
    doc = {"command": "python tools/denoise_cost.py", "workloads": []}
    if args.json and os.path.exists(args.json):
        doc = json.load(open(args.json))
    if args.pair_trace:
        doc["kernel_trace"] = pair_trace(args.pair_trace)
    else:
        doc["workloads"] = run(args.only)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
