"""What the read-out of a sample-keeping film costs under each reconstruction filter: cfg2_cube at 1024x1024 with 16 and 64 kept samples,
the plan's radius equal to the filter's.

Timed is the device time of the read-out kernels of one spt_film_read(MEAN), between the scene's two events
(spt_debug_render_info, what 2): five reads after one warm-up read, the median and the spread (min, max) of each.  The box rows use
only calls that exist without spt_film_filter, so the same tool measures the box on a library built before the weighted filters;
the weighted rows are left out there.  --parent-json takes that run's --json file (made in the same job, on the same machine)
and records the condition on the box: this tree's box median is no more than the parent's plus the larger of the two five-run
spreads (`parent_box`, `box_condition`).

  python tools/filter_cost.py [--reps 5] [--json profiles/filter_cost.json] [--parent-json parent_filter_cost.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
spt = importlib.import_module("simple-path-tracer_amd")

CASES = [("box r=1.0", "box", 1.0, {}), ("box r=2.0", "box", 2.0, {}), ("tent r=1.0", "tent", 1.0, {}),
         ("gaussian r=1.5", "gaussian", 1.5, {"alpha": 2.0}), ("mitchell r=2.0", "mitchell", 2.0, {"b": 1.0 / 3.0, "c": 1.0 / 3.0})]


def stat(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "spread": round(max(xs) - min(xs), 4)}


def with_parent(result, parent):
    """`result` with the parent commit's box rows and the condition on the box, row by row."""
    rows = {}
    for spp, mine in result["samples"].items():
        for name, a in mine.items():
            b = parent["samples"].get(spp, {}).get(name)
            if not name.startswith("box") or b is None:
                continue
            margin = max(a["spread"], b["spread"])
            rows["%s spp, %s" % (spp, name)] = {"this_tree": a["median"], "parent": b["median"], "margin": round(margin, 4),
                                               "not_slower": a["median"] <= b["median"] + margin}
    out = dict(result)
    out["parent_box"] = {spp: {n: v for n, v in r.items() if n.startswith("box")} for spp, r in parent["samples"].items()}
    out["box_condition"] = {"rule": "this tree's box median <= the parent's + the larger of the two five-run spreads", "rows": rows,
                            "met": all(r["not_slower"] for r in rows.values())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--spp", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--json", default=None, help="also write the result here")
    ap.add_argument("--parent-json", default=None, help="the --json file of this tool run on the parent commit: adds parent_box and box_condition")
    args = ap.parse_args()
    assert spt.device_count() >= 1, "needs an MI355X"
    weighted = hasattr(spt.ProgressiveFilm, "set_filter")
    scene = spt.load_scene(os.path.join(ROOT, "scenes_amd", "cfg2_cube.json"))
    ds = scene.device_scene(0)
    cfg = spt.OutputConfig(args.width, args.height)
    result = {"workload": "cfg2_cube %dx%d, spt_film_read(MEAN) of a sample-keeping film" % (args.width, args.height), "reps": args.reps,
              "unit": "ms on the device (spt_debug_render_info, what 2)", "weighted_filters": weighted, "samples": {}}
    for spp in args.spp:
        rows = {}
        for name, kind, radius, params in CASES:
            if kind != "box" and not weighted:
                continue
            r = spt.load_renderer(os.path.join(ROOT, "scenes_amd", "pt.json"), seed=1)
            r.spp = spp
            r.filter_radius = radius
            with r.progressive(scene, cfg, keep_samples=True) as film:
                for _ in range(spp // 16):
                    film.render(16)
                if spp % 16:
                    film.render(spp % 16)
                if kind != "box":
                    film.set_filter(kind, radius=radius, **params)
                ms = []
                for k in range(args.reps + 1):
                    mean = film.mean()
                    if k:                                  # (the first read warms up)
                        ms.append(ds.render_info(2) / 1e6)
                assert mean.max() > 0.1
            rows[name] = stat(ms)
            print("%3d spp  %-16s %s" % (spp, name, rows[name]), flush=True)
        for name in rows:
            if not name.startswith("box"):
                rows[name]["ratio_to_box_r1"] = round(rows[name]["median"] / rows["box r=1.0"]["median"], 3)
                rows[name]["ratio_to_box_r2"] = round(rows[name]["median"] / rows["box r=2.0"]["median"], 3)
        result["samples"][str(spp)] = rows
    scene.close()
    if args.parent_json:
        with open(args.parent_json) as f:
            result = with_parent(result, json.load(f))
    print(json.dumps(result))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
