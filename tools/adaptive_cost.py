"""What adaptive sampling (spt_film_adapt) costs and buys, on one MI355X.

For each workload: an adaptive moments film takes increments of spp / 16 samples with an adapt after each, until no pixel is
active or spp is reached; the time of every increment and every adapt and the active fractions (pixels, and 16x16 tiles with any
active pixel) after each are recorded.  A uniform film of the same plan takes the same increments without adapting.  Both are
compared with a high-spp render of ANOTHER seed (the reference): the per-pixel error of the adaptive film against that of the
uniform film at EQUAL TIME (the uniform film's error curve interpolated linearly in time at the adaptive film's total time).
Host clocks around synchronous calls, after a warm-up run of each schedule; one repetition per tolerance.  Both the plan's
sampler of pt.json (the R2 recurrence) and the independent random sampler are run.  Pixels that are not finite in the reference
or in a film are left out of the errors and counted.

  python tools/adaptive_cost.py [--json profiles/adaptive_cost.json]
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/adaptive_cost.py --trace steps.json
      one adaptive and one uniform film of cfg2 (random sampler, rel 0.03), no warm-up: the i-th masked k_primary launch of the
      trace is the i-th increment of steps.json (one pass per increment at this size)
  python tools/adaptive_cost.py --pair-trace DIR/..._kernel_trace.csv steps.json
      pairs them: k_primary time per increment against the active pixel and tile fractions of the adapt before it
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
    # name, scene, camera, width, height, spp, reference spp, tolerances (rel_error)
    ("cfg2_cube", "cfg2_cube.json", None, 1024, 1024, 256, 4096, (0.1, 0.03, 0.01)),
    ("t_materials", "t_materials.json", "main", 512, 512, 256, 4096, (0.1, 0.03, 0.01)),
]
SAMPLERS = (("recurrence", 2), ("random", 0))
ABS_FLOOR = 1e-4
MIN_SAMPLES = 16


def errors(img, ref):
    ok = np.isfinite(img).all(axis=-1) & np.isfinite(ref).all(axis=-1)
    d = img[ok].astype(np.float64) - ref[ok]
    return {"l1": float(np.abs(d).mean()), "rmse": float(np.sqrt((d * d).mean())), "nonfinite_pixels": int((~ok).sum())}


def tile_fraction(counts, done):
    rows, w = counts.shape
    ty, tx = (rows + 15) // 16, (w + 15) // 16
    pad = np.zeros((ty * 16, tx * 16), bool)
    pad[:rows, :w] = counts == done
    return float(pad.reshape(ty, 16, tx, 16).any(axis=(1, 3)).mean())


def uniform_run(r, sc, cfg, inc, spp, ref):
    steps, t = [], 0.0
    with r.progressive(sc, cfg, moments=True) as f:
        while f.samples < spp:
            t0 = time.perf_counter()
            f.render(inc)
            t += time.perf_counter() - t0
            steps.append(dict(samples=f.samples, ms=round(t * 1e3, 3), **errors(f.mean(), ref)))
    return steps


def adaptive_run(r, sc, cfg, inc, spp, ref, rel):
    steps, t_inc, t_adapt = [], 0.0, 0.0
    with r.progressive(sc, cfg, moments=True) as f:
        n_pix = f.rows * f.width
        while f.samples < spp:
            t0 = time.perf_counter()
            f.render(inc)
            t1 = time.perf_counter()
            if steps:   # the pixels the last adapt left active are those that took this increment (a pixel retired by an adapt
                        # also has n_p == done right after it, so the fraction is read one increment late)
                steps[-1]["active_tiles"] = round(tile_fraction(f.sample_counts(), f.samples), 4)
            t1b = time.perf_counter()
            active = f.adapt(rel, ABS_FLOOR, MIN_SAMPLES)
            t2 = time.perf_counter()
            t_inc += t1 - t0
            t_adapt += t2 - t1b
            steps.append({"samples": f.samples, "increment_ms": round((t1 - t0) * 1e3, 3), "adapt_ms": round((t2 - t1b) * 1e3, 3),
                          "active_pixels": round(active / n_pix, 4), "active_tiles": None if active else 0.0})
            if active == 0:
                break
        counts = f.sample_counts()
        res = {"rel_error": rel, "abs_floor": ABS_FLOOR, "min_samples": MIN_SAMPLES, "ms": round((t_inc + t_adapt) * 1e3, 3),
               "increments_ms": round(t_inc * 1e3, 3), "adapts_ms": round(t_adapt * 1e3, 3),
               "mean_samples_per_pixel": round(float(counts.mean()), 2), **errors(f.mean(), ref), "steps": steps}
    return res


def at_time(curve, ms, key):
    """The uniform film's error at `ms`, linear in time between its increments (None before the first / past the last)."""
    for a, b in zip(curve, curve[1:]):
        if a["ms"] <= ms <= b["ms"]:
            w = (ms - a["ms"]) / max(b["ms"] - a["ms"], 1e-12)
            return a[key] + w * (b[key] - a[key])
    return None


def trace(path):
    sc = spt.load_scene(os.path.join(ROOT, "scenes_amd", "cfg2_cube.json"))
    r = spt.load_renderer(os.path.join(ROOT, "scenes_amd", "pt.json"), seed=1)
    r.sampler, r.spp = 0, 256
    cfg = spt.OutputConfig(1024, 1024)
    ref = np.zeros((1024, 1024, 3))
    a = adaptive_run(r, sc, cfg, 16, 256, ref, 0.03)
    uniform_run(r, sc, cfg, 16, 256, ref)
    with open(path, "w") as fh:
        json.dump(a["steps"], fh, indent=1)
    sc.close()


def pair_trace(csv_path, steps_path):
    import csv
    steps = json.load(open(steps_path))
    rows = sorted(csv.DictReader(open(csv_path)), key=lambda d: int(d["Start_Timestamp"]))
    dur = lambda d: (int(d["End_Timestamp"]) - int(d["Start_Timestamp"])) * 1e-6
    masked = [dur(d) for d in rows if "k_primary" in d["Kernel_Name"] and "FilmMask" in d["Kernel_Name"]]
    plain = [dur(d) for d in rows if "k_primary" in d["Kernel_Name"] and "FilmMask" not in d["Kernel_Name"]]
    adapt = [dur(d) for d in rows if "k_film_adapt" in d["Kernel_Name"]]
    # the adaptive film's first increment (before its first adapt) and the uniform film's 16 run the plain chunked instance
    assert len(plain) == 17 and len(masked) == len(steps) - 1, (len(plain), len(masked), len(steps))
    base = float(np.median(plain[1:]))
    out = {"k_primary_ms_uniform_median": round(base, 4), "k_film_adapt_ms_median": round(float(np.median(adapt)), 4), "increments": []}
    for k, ms in enumerate(masked):   # increment k + 1 follows the adapt of step k
        out["increments"].append({"samples": steps[k + 1]["samples"], "k_primary_ms": round(ms, 4), "vs_uniform": round(ms / base, 4),
                                  "active_pixels": steps[k]["active_pixels"], "active_tiles": steps[k]["active_tiles"]})
    print(json.dumps(out, indent=1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the result here")
    ap.add_argument("--only", default=None, help="one workload by name")
    ap.add_argument("--trace", default=None, metavar="STEPS_JSON")
    ap.add_argument("--pair-trace", nargs=2, default=None, metavar=("KERNEL_TRACE_CSV", "STEPS_JSON"))
    args = ap.parse_args()
    if args.trace:
        return trace(args.trace)
    if args.pair_trace:
        res = pair_trace(*args.pair_trace)
        if args.json:
            with open(args.json, "w") as fh:
                json.dump(res, fh, indent=1)
        return
    out = {"command": "python tools/adaptive_cost.py", "workloads": []}
    for (name, scene_name, camera, w, h, spp, ref_spp, rels), (sampler_name, sampler) in [(wl, s) for wl in WORKLOADS for s in SAMPLERS]:
        if args.only and args.only != name:
            continue
        sc = spt.load_scene(os.path.join(ROOT, "scenes_amd", scene_name))
        r = spt.load_renderer(os.path.join(ROOT, "scenes_amd", "pt.json"), seed=1)
        r.sampler = sampler
        cfg = spt.OutputConfig(w, h, None, camera)
        r_ref = spt.load_renderer(os.path.join(ROOT, "scenes_amd", "pt.json"), seed=977)
        r_ref.spp = ref_spp
        ref = r_ref.render_shard(sc, cfg).astype(np.float64)
        r.spp = spp
        inc = max(1, spp // 16)
        uniform_run(r, sc, cfg, inc, spp, ref)            # warm-up
        uni = uniform_run(r, sc, cfg, inc, spp, ref)
        wl = {"workload": "%s %dx%d @ %d spp, %s sampler, increments of %d" % (name, w, h, spp, sampler_name, inc),
              "reference": "recurrence sampler, seed 977, %d spp" % ref_spp, "uniform": uni, "adaptive": []}
        print("%s: uniform %d spp in %.2f ms, l1 %.4g rmse %.4g" % (wl["workload"], spp, uni[-1]["ms"], uni[-1]["l1"], uni[-1]["rmse"]))
        for rel in rels:
            adaptive_run(r, sc, cfg, inc, spp, ref, rel)  # warm-up
            a = adaptive_run(r, sc, cfg, inc, spp, ref, rel)
            for key in ("l1", "rmse"):
                u = at_time(uni, a["ms"], key)
                a["uniform_%s_at_equal_time" % key] = None if u is None else round(u, 6)
                a["%s_ratio_at_equal_time" % key] = None if u is None else round(a[key] / u, 4)
            a["adapt_share_of_time"] = round(a["adapts_ms"] / a["ms"], 4)
            wl["adaptive"].append(a)
            print("  rel %.3g: %.2f ms (adapts %.2f ms), %.1f spp mean, l1 %.4g rmse %.4g, equal-time ratio l1 %s rmse %s" % (
                rel, a["ms"], a["adapts_ms"], a["mean_samples_per_pixel"], a["l1"], a["rmse"], a["l1_ratio_at_equal_time"],
                a["rmse_ratio_at_equal_time"]))
        out["workloads"].append(wl)
        sc.close()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
