#!/usr/bin/env python3
"""Per-step figures from a rocprofv3 --kernel-trace CSV of bench.py: between the first k_primary and the last bounce-0 shade kernel of a
frame, the time no kernel of {fill, k_block_candidates, k_primary, bounce-0 shade} runs, their sum, their overlap, the film queue's busy time.
usage: trace_idle.py <kernel_trace.csv> [skip_frames=8] [passes_per_frame=2]"""
import sys

import pandas as pd

df = pd.read_csv(sys.argv[1]).sort_values("Start_Timestamp").reset_index(drop=True)
skip = int(sys.argv[2]) if len(sys.argv) > 2 else 8
ppf = int(sys.argv[3]) if len(sys.argv) > 3 else 2
name = df["Kernel_Name"].astype(str)
is_prim = name.str.contains("k_primary")
is_shade0 = name.str.contains(r"k_shade<0, true")
prim = df[is_prim].reset_index(drop=True)
sh0 = df[is_shade0].reset_index(drop=True)
print("k_primary launches %d, bounce-0 shade launches %d" % (len(prim), len(sh0)))
print("queues: k_primary %s, shade0 %s" % (sorted(prim["Queue_Id"].unique()), sorted(sh0["Queue_Id"].unique())))
n_frames = min(len(prim), len(sh0)) // ppf
main_q = set(prim["Queue_Id"].unique()) | set(sh0["Queue_Id"].unique())
film_names = name.str.contains("k_resolve|k_finish|k_shade<0, false")
rows = []
for f in range(skip, n_frames - 1):
    t0 = prim["Start_Timestamp"].iloc[f * ppf]
    t1 = sh0["End_Timestamp"].iloc[f * ppf + ppf - 1]
    t_next = prim["Start_Timestamp"].iloc[(f + 1) * ppf]
    # kernels of the primary / shade queues that are not film-stage kernels, inside the frame's window
    w = df[(df["Start_Timestamp"] >= t0) & (df["End_Timestamp"] <= t1) & df["Queue_Id"].isin(main_q) & ~film_names]
    iv = sorted(zip(w["Start_Timestamp"], w["End_Timestamp"]))
    busy, cur_s, cur_e = 0, None, None
    for s, e in iv:
        if cur_e is None or s > cur_e:
            if cur_e is not None:
                busy += cur_e - cur_s
            cur_s, cur_e = s, e
        else:
            cur_e = max(cur_e, e)
    if cur_e is not None:
        busy += cur_e - cur_s
    ksum = int((w["End_Timestamp"] - w["Start_Timestamp"]).sum())
    fw = df[(df["Start_Timestamp"] >= t0) & (df["Start_Timestamp"] < t_next) & film_names]
    film_busy = int((fw["End_Timestamp"] - fw["Start_Timestamp"]).sum())
    rows.append((f, (t_next - t0) / 1e3, (t1 - t0) / 1e3, busy / 1e3, (t1 - t0 - busy) / 1e3, ksum / 1e3, (ksum - busy) / 1e3, film_busy / 1e3))
print("frame  step_us  window_us  union_busy_us  idle_us  kernel_sum_us  overlapped_us  film_busy_us")
for r in rows:
    print("%5d %8.1f %9.1f %13.1f %8.1f %13.1f %13.1f %12.1f" % r)
if rows:
    import statistics as st
    print("median %8.1f %9.1f %13.1f %8.1f %13.1f %13.1f %12.1f" % tuple(st.median(r[k] for r in rows) for k in range(1, 8)))
for label, sel in (("k_primary", is_prim), ("shade0", is_shade0), ("tail", name.str.contains("k_shade<0, false")), ("resolve", name.str.contains("k_resolve")),
                   ("finish", name.str.contains("k_finish")), ("block_cand", name.str.contains("k_block_candidates"))):
    d = df[sel]
    if len(d):
        dur = (d["End_Timestamp"] - d["Start_Timestamp"]) / 1e3
        print("%-10s n %4d  mean %8.1f us  median %8.1f us  min %8.1f  max %8.1f" % (label, len(d), dur.mean(), dur.median(), dur.min(), dur.max()))
