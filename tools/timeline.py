#!/usr/bin/env python3
"""Dispatch timeline of the last render in a rocprofv3 --kernel-trace CSV: start offset, duration, gap to the previous
dispatch (negative: it started beside it), hardware queue.  With a --memory-copy-trace CSV as the third argument the copies
the runtime ran on a DMA engine are printed between the kernels, in start order (a copy that ran as a blit kernel is a
dispatch and in the kernel trace already).
usage: python3 tools/timeline.py <..._kernel_trace.csv> [n_last=20] [<..._memory_copy_trace.csv>]"""
import sys

import pandas as pd

df = pd.read_csv(sys.argv[1])
n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
df = df[["Start_Timestamp", "End_Timestamp", "Kernel_Name"] + (["Queue_Id"] if "Queue_Id" in df else [])]
if len(sys.argv) > 3:
    mc = pd.read_csv(sys.argv[3])
    mc["Kernel_Name"] = "[copy engine] " + mc["Direction"].astype(str) + " " + mc["Source_Agent_Id"].astype(str) + " -> " + mc["Destination_Agent_Id"].astype(str)
    mc["Queue_Id"] = "-"
    df = pd.concat([df, mc[[c for c in df.columns]]], ignore_index=True)
df = df.sort_values("Start_Timestamp").tail(n)
t0 = df["Start_Timestamp"].iloc[0]
prev_end = None
for _, r in df.iterrows():
    gap = 0.0 if prev_end is None else (r["Start_Timestamp"] - prev_end) / 1e3
    print("%9.1f us  dur %8.1f us  gap %7.1f us  q %s  %s" % ((r["Start_Timestamp"] - t0) / 1e3, (r["End_Timestamp"] - r["Start_Timestamp"]) / 1e3, gap,
                                                             r.get("Queue_Id", "?"), r["Kernel_Name"][:80]))
    prev_end = max(prev_end or 0, r["End_Timestamp"])
