"""What bucketed films (spt_film_buckets, spt_film_read_robust) cost on one MI355X, and what their read-outs gain.

Cost: per workload a plan of 256 samples is rendered in 16 increments of 16 into a film with K = 9 buckets and into the same film
without buckets, alternating, five rounds after one warm-up round; then spt_film_read_robust (both estimators) is timed next to
spt_film_read MEAN on the finished bucketed film.  Host clocks around the synchronous calls, medians.

  python tools/robust_cost.py [--json profiles/robust_cost.json]
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/robust_cost.py --trace
      one bucketed film per workload (16 increments, then one read of each kind), for the kernel times
  python tools/robust_cost.py --pair-trace DIR/..._kernel_trace.csv [--json profiles/robust_cost.json]
      per workload: the summed time of k_resolve_buckets, of the plain resolve and of every other kernel of the 16 increments, and
      the read kernels; merged into the JSON of the first form when it exists
  python tools/robust_cost.py --quality [--cpu] [--json profiles/robust_cost.json]
      RMSE of the plain mean, MON and GMON (64 samples of seed 5, K = 9, 96x72, random sampler, max_depth 5) against 2048 samples
      of seed 77 over the pixels finite in all four images, on five scenes; --cpu: from the CPU oracle's single samples and the
      float32 restatement (tests/_robust_ref.py) instead of the device
  hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S -o /dev/null simple-path-tracer_amd/csrc/hip/spt_hip.hip \
        -Rpass-analysis=kernel-resource-usage 2> LOG;  python tools/robust_cost.py --resources LOG [--json profiles/robust_cost.json]
      VGPRs, SGPRs, scratch, LDS and occupancy of the new kernels from the compiler's remarks (no GPU needed)
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
SPP, INCREMENT, K, REPEATS = 256, 16, 9, 5
QUALITY = dict(width=96, height=72, spp=64, seed=5, max_depth=5, ref_spp=2048, ref_seed=77)
QUALITY_SCENES = [("cfg2_cube.json", None), ("t_materials.json", "main"), ("t_textured.json", None), ("t_plastic.json", None),
                  ("t_medium.json", None)]


def median(ms):
    return round(float(np.median(ms)), 4)


def render_all(film):
    """The plan in increments; the host time of each."""
    ms = []
    for _ in range(SPP // INCREMENT):
        t0 = time.perf_counter()
        film.render(INCREMENT)
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def timed(fn, repeats):
    fn()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return median(ms), [round(x, 4) for x in ms]


def run(only=None, trace=False):
    out = []
    for name, scene_name, camera, w, h in WORKLOADS:
        if only and only != name:
            continue
        sc = spt.load_scene(os.path.join(ROOT, "scenes_amd", scene_name))
        r = spt.load_renderer(os.path.join(ROOT, "scenes_amd", "pt.json"), seed=1)
        r.sampler, r.spp = 0, SPP
        cfg = spt.OutputConfig(w, h, None, camera)
        if trace:
            with r.progressive(sc, cfg, buckets=K) as film:
                render_all(film)
                film.mean()
                film.robust_mean("mon")
                film.robust_mean("gmon")
            sc.close()
            continue
        plain_ms, bucket_ms = [], []
        for rnd in range(REPEATS + 1):           # round 0 warms up
            for buckets, acc in ((0, plain_ms), (K, bucket_ms)):
                with r.progressive(sc, cfg, buckets=buckets) as film:
                    ms = render_all(film)
                    if rnd:
                        acc.append(median(ms))   # the median increment of this film
                    if rnd == REPEATS and buckets:
                        mean = timed(film.mean, REPEATS)
                        mon = timed(lambda: film.robust_mean("mon"), REPEATS)
                        gmon = timed(lambda: film.robust_mean("gmon"), REPEATS)
        sc.close()
        wl = {"workload": "%s %dx%d, random sampler, %d samples in %d-sample increments, K = %d" % (name, w, h, SPP, INCREMENT, K),
              "name": name, "pixels": w * h,
              "increment_ms": median(plain_ms), "increment_buckets_ms": median(bucket_ms),
              "buckets_over_plain": round(median(bucket_ms) / median(plain_ms), 4),
              "film_mean_ms": mean[0], "read_robust_mon_ms": mon[0], "read_robust_gmon_ms": gmon[0],
              "samples_ms": {"increment": plain_ms, "increment_buckets": bucket_ms, "film_mean": mean[1], "mon": mon[1], "gmon": gmon[1]}}
        print("%s: increment %.4f ms, with buckets %.4f ms (ratio %.4f); read MEAN %.4f ms, MON %.4f ms, GMON %.4f ms" % (
            wl["workload"], wl["increment_ms"], wl["increment_buckets_ms"], wl["buckets_over_plain"], mean[0], mon[0], gmon[0]))
        out.append(wl)
    return out


def pair_trace(csv_path):
    """The trace of `--trace`: a workload's kernels end with its second k_film_read_robust (MON, then GMON)."""
    import csv
    rows = sorted(csv.DictReader(open(csv_path)), key=lambda d: int(d["Start_Timestamp"]))
    us = lambda d: (int(d["End_Timestamp"]) - int(d["Start_Timestamp"])) * 1e-3
    reads = [i for i, d in enumerate(rows) if "k_film_read_robust" in d["Kernel_Name"]]
    assert len(reads) == 2 * len(WORKLOADS), len(reads)
    out, begin = [], 0
    for k, (name, _, _, w, h) in enumerate(WORKLOADS):
        end = reads[2 * k + 1] + 1
        part = rows[begin:end]
        begin = end
        buckets = [us(d) for d in part if "k_resolve_buckets" in d["Kernel_Name"]]
        resolve = [us(d) for d in part if "k_resolve" in d["Kernel_Name"] and "k_resolve_buckets" not in d["Kernel_Name"]]
        robust = [us(d) for d in part if "k_film_read_robust" in d["Kernel_Name"]]
        mean = [us(d) for d in part if "k_film_read" in d["Kernel_Name"] and "robust" not in d["Kernel_Name"]]
        other = sum(us(d) for d in part if "k_resolve" not in d["Kernel_Name"] and "k_film_read" not in d["Kernel_Name"])
        passes = len(buckets)
        # per pass and pixel: 12 B per sample re-read, K * 12 B read and K * 12 B written
        nbytes = (INCREMENT * 12 + 2 * K * 12) * w * h
        res = {"name": name, "passes": passes, "k_resolve_buckets_us_per_pass": round(float(np.median(buckets)), 2),
               "k_resolve_us_per_pass": round(float(np.median(resolve)), 2), "resolve_passes": len(resolve),
               "k_resolve_buckets_us_total": round(sum(buckets), 2), "k_resolve_us_total": round(sum(resolve), 2),
               "other_kernels_us_total": round(other, 2),
               "k_resolve_buckets_bytes_per_pixel_and_pass": nbytes // (w * h),
               "k_resolve_buckets_fraction_of_6.3_TB_per_s": round(nbytes / (float(np.median(buckets)) * 1e-6) / 6.3e12, 4),
               "k_film_read_us": round(mean[-1], 2), "k_film_read_robust_mon_us": round(robust[0], 2), "k_film_read_robust_gmon_us": round(robust[1], 2),
               "note": "one bucketed film, %d increments of %d samples, kernel times from rocprofv3 --kernel-trace" % (SPP // INCREMENT, INCREMENT)}
        out.append(res)
    print(json.dumps(out, indent=1))
    return out


def rmse_table(images, ref):
    keep = np.isfinite(ref).all(axis=-1)
    for img in images.values():
        keep &= np.isfinite(img).all(axis=-1)
    r64 = ref[keep].astype(np.float64)
    res = {k: round(float(np.sqrt(((img[keep].astype(np.float64) - r64) ** 2).mean())), 4) for k, img in images.items()}
    res["pixels_left_out"] = int((~keep).sum())
    return res


def quality(cpu):
    q = QUALITY
    out = []
    if cpu:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import _robust_ref as R
        import _util
        _util.ensure_cpu_build()
        pkg = _util.load_pkg()      # the oracle's bindings take the structures of the package as the tests load it
    else:
        pkg = spt
    for scene_name, camera in QUALITY_SCENES:
        sc = pkg.load_scene(os.path.join(ROOT, "scenes_amd", scene_name))
        plan = pkg.PathTracer(max_depth=q["max_depth"], sampler=pkg.SAMPLER_RANDOM, spp=q["spp"], seed=q["seed"])
        long_plan = pkg.PathTracer(max_depth=q["max_depth"], sampler=pkg.SAMPLER_RANDOM, spp=q["ref_spp"], seed=q["ref_seed"])
        w, h = q["width"], q["height"]
        if cpu:
            ref, _ = _util.oracle_render(sc, long_plan, w, h, camera=camera, flags=_util.ORACLE_DEVICE)
            xs = _util.oracle_render_samples(sc, plan, w, h, 0, q["spp"], camera=camera, flags=_util.ORACLE_DEVICE)
            s = np.zeros_like(xs[0])
            with np.errstate(all="ignore"):
                for x in xs:
                    s = s + x
                b = R.bucket_sums(xs, 0, K)
                images = {"mean": s * (np.float32(1) / np.float32(q["spp"])), "mon": R.robust(b, s, 0, q["spp"], R.MON),
                          "gmon": R.robust(b, s, 0, q["spp"], R.GMON)}
        else:
            cfg = pkg.OutputConfig(w, h, None, camera)
            ref = long_plan.render_shard(sc, cfg).copy()
            with plan.progressive(sc, cfg, buckets=K) as film:
                film.render(q["spp"])
                images = {"mean": film.mean(), "mon": film.robust_mean("mon"), "gmon": film.robust_mean("gmon")}
        sc.close()
        res = {"scene": scene_name[:-5]}
        res.update(rmse_table(images, ref))
        res["gmon_over_mean"] = round(res["gmon"] / res["mean"], 4)
        print("%-12s RMSE mean %.4f  MON %.4f  GMON %.4f  (GMON / mean %.3f, %d pixels left out)" % (
            res["scene"], res["mean"], res["mon"], res["gmon"], res["gmon_over_mean"], res["pixels_left_out"]))
        out.append(res)
    return out


def resources(log_path):
    """The compiler's kernel-resource-usage remarks of k_resolve_buckets<.> and k_film_read_robust<.>."""
    import re
    keys = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch_bytes", "LDS Size [bytes/block]": "lds_bytes",
            "Occupancy [waves/SIMD]": "waves_per_simd", "VGPRs Spill": "vgpr_spills", "SGPRs Spill": "sgpr_spills"}
    out, cur = {}, None
    for line in open(log_path):
        m = re.search(r"remark:\s+(Function Name|[A-Za-z][A-Za-z \[\]/]*):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            k = re.match(r"_Z\d+(k_resolve_buckets|k_film_read_robust)ILb([01])E", m.group(2))
            cur = "%s<%s>" % (k.group(1), "true" if k.group(2) == "1" else "false") if k else None
            if cur:
                out[cur] = {}
        elif cur and m.group(1).strip() in keys:
            out[cur][keys[m.group(1).strip()]] = int(m.group(2))
    assert len(out) == 4, sorted(out)
    out["source"] = "hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage with the build's flags"
    print(json.dumps(out, indent=1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write (or merge into) this file")
    ap.add_argument("--only", default=None, help="one workload by name")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--pair-trace", default=None, metavar="KERNEL_TRACE_CSV")
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--resources", default=None, metavar="COMPILE_LOG")
    args = ap.parse_args()
    if args.trace:
        run(trace=True)
        return
    doc = {"command": "python tools/robust_cost.py", "workloads": []}
    if args.json and os.path.exists(args.json):
        doc = json.load(open(args.json))
    if args.resources:
        doc["kernel_resources"] = resources(args.resources)
    elif args.pair_trace:
        doc["kernel_trace"] = pair_trace(args.pair_trace)
    elif args.quality:
        doc["quality_cpu_oracle" if args.cpu else "quality_device"] = {
            "plan": "%(width)dx%(height)d, random sampler, max_depth %(max_depth)d, %(spp)d samples of seed %(seed)d against %(ref_spp)d of seed %(ref_seed)d" % QUALITY + ", K = %d" % K,
            "rmse": quality(args.cpu)}
    else:
        doc["workloads"] = run(args.only)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
