"""What the 8-bit read-out of a film (spt_film_read_rgb8) costs and buys, on one MI355X.

Each read-out runs as f32 and as RGB8 alternately in one process: REPEATS rounds of (f32, RGB8) after one warm-up round, the
median per variant, host clocks around the synchronous calls.

  previews     a moments film of cfg2_cube 1024x1024 after 16 samples, its guide after 16: spt_film_read MEAN against
               spt_film_read_rgb8 MEAN, spt_film_denoise against spt_film_read_rgb8 DENOISED (5 iterations, with the guide), each
               into pageable and into page-locked memory, next to one further 16-sample increment of the film
  pack kernel  from a kernel trace of its own (below)

  python tools/rgb8_cost.py [--json profiles/rgb8_cost.json] [--label NAME]
      with SPT_LIB_DIR naming a build without the entry point (the parent commit) only the f32 variants run: the same job
      alternates the two builds process by process, and --label keeps their results apart in the JSON ("runs": a list)
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/rgb8_cost.py --trace
      the read-outs twice each, for the kernel times
  python tools/rgb8_cost.py --pair-trace DIR/..._kernel_trace.csv [--json profiles/rgb8_cost.json]
      k_pack_rgb8 alone: its launches, their median time and the fraction of 6.3 TB/s that its 15 bytes per pixel (12 read, 3
      written) come to; the blit kernels of the runtime's copy-out next to it
"""
import argparse
import ctypes as C
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
INCREMENT, ITERATIONS, REPEATS = 16, 5, 5
HBM_BYTES_PER_S = 6.3e12


def has_rgb8():
    return hasattr(spt.hip_lib(), "spt_film_read_rgb8")


def alternate(variants, repeats=REPEATS, warm=True):
    """variants: {name: fn returning ms}.  One warm-up round, then `repeats` rounds that run every variant once, in order."""
    if warm:
        for fn in variants.values():
            fn()
    ms = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            ms[k].append(fn())
    return {k: {"median_ms": round(float(np.median(v)), 4), "samples_ms": [round(x, 4) for x in v]} for k, v in ms.items()}


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def previews(repeats=REPEATS):
    sc = spt.load_scene(os.path.join(ROOT, "scenes_amd", "cfg2_cube.json"))
    r = spt.load_renderer(os.path.join(ROOT, "scenes_amd", "pt.json"), seed=1)
    r.sampler, r.spp = 0, INCREMENT * (repeats + 3)
    cfg = spt.OutputConfig(W, H)
    lib = spt.hip_lib()
    ds = sc.device_scene(0)
    out = {}
    with r.progressive(sc, cfg, moments=True) as film, r.guide_film(sc, cfg) as guide:
        film.render(INCREMENT)
        guide.render(INCREMENT)
        dn = spt.DenoiseParams(C.sizeof(spt.DenoiseParams), ITERATIONS, 2.0, 1.0, 1e-8, 1e-2)
        pinned = ds.film_buffer(H, W)                        # page-locked, (H, W, 3) f32: its first quarter holds the bytes
        targets = {"pageable": (np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.uint8)),
                   "pinned": (pinned, pinned.reshape(-1).view(np.uint8)[:H * W * 3])}
        for memory, (f32, u8) in targets.items():
            fh, gh = film._handle(), guide._handle()
            ok = lambda status: spt._check_hip(status)
            mean = {"f32": lambda: clock(lambda: ok(lib.spt_film_read(fh, spt.FILM_MEAN, f32.ctypes.data)))}
            den = {"f32": lambda: clock(lambda: ok(lib.spt_film_denoise(fh, gh, C.byref(dn), f32.ctypes.data)))}
            if has_rgb8():
                mean["rgb8"] = lambda: clock(lambda: ok(lib.spt_film_read_rgb8(fh, 0, None, None, u8.ctypes.data)))
                den["rgb8"] = lambda: clock(lambda: ok(lib.spt_film_read_rgb8(fh, 3, gh, C.byref(dn), u8.ctypes.data)))
            out[memory] = {"film_mean_ms": alternate(mean, repeats), "denoise_with_guide_ms": alternate(den, repeats)}
        out["increment_ms"] = alternate({"f32": lambda: clock(lambda: film.render(INCREMENT))}, repeats, warm=True)["f32"]
    sc.close()
    out["workload"] = "cfg2_cube %dx%d film with moments, random sampler, %d-sample increments, %d denoise iterations" % (W, H, INCREMENT, ITERATIONS)
    return out


def trace_run():
    """What `--trace` runs under the profiler: the two RGB8 read-outs and the float mean, twice each."""
    sc = spt.load_scene(os.path.join(ROOT, "scenes_amd", "cfg2_cube.json"))
    r = spt.load_renderer(os.path.join(ROOT, "scenes_amd", "pt.json"), seed=1)
    r.sampler, r.spp = 0, 2 * INCREMENT
    cfg = spt.OutputConfig(W, H)
    with r.progressive(sc, cfg, moments=True) as film, r.guide_film(sc, cfg) as guide:
        film.render(INCREMENT)
        guide.render(INCREMENT)
        for _ in range(2):
            film.read_rgb8("mean")
            film.read_rgb8("denoised", guide)
            film.mean()
    sc.close()


def pair_trace(csv_path):
    import csv
    rows = list(csv.DictReader(open(csv_path)))
    us = lambda d: (int(d["End_Timestamp"]) - int(d["Start_Timestamp"])) * 1e-3
    pack = [us(d) for d in rows if "k_pack_rgb8" in d["Kernel_Name"]]
    read = [us(d) for d in rows if d["Kernel_Name"].startswith("k_film_read")]
    blit = [us(d) for d in rows if "copyBuffer" in d["Kernel_Name"] or "__amd_rocclr" in d["Kernel_Name"]]
    nbytes = 15 * W * H
    res = {"k_pack_rgb8": {"launches": len(pack), "median_us": round(float(np.median(pack)), 2) if pack else None, "all_us": [round(x, 2) for x in pack],
                           "bytes": nbytes,
                           "fraction_of_6.3_TB_per_s": round(nbytes / (float(np.median(pack)) * 1e-6) / HBM_BYTES_PER_S, 4) if pack else None},
           "k_film_read": {"launches": len(read), "median_us": round(float(np.median(read)), 2) if read else None},
           "runtime_copy_kernels": {"launches": len(blit), "all_us": [round(x, 2) for x in blit]},
           "note": "every image is %dx%d; the first launch of each kernel includes its code's first use" % (W, H)}
    print(json.dumps(res, indent=1))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write (append a run to, or with --pair-trace merge into) this file")
    ap.add_argument("--label", default=None, help="name of this run in the JSON (default: the library directory)")
    ap.add_argument("--repeats", type=int, default=REPEATS)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--pair-trace", default=None, metavar="KERNEL_TRACE_CSV")
    args = ap.parse_args()
    if args.trace:
        trace_run()
        return
    doc = {"command": "python tools/rgb8_cost.py", "runs": []}
    if args.json and os.path.exists(args.json):
        doc = json.load(open(args.json))
    if args.pair_trace:
        doc["kernel_trace"] = pair_trace(args.pair_trace)
    else:
        run = {"label": args.label or os.path.relpath(spt.LIB_DIR, ROOT), "has_rgb8": has_rgb8()}
        run["previews"] = previews(args.repeats)
        print(json.dumps(run, indent=1))
        doc.setdefault("runs", []).append(run)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
