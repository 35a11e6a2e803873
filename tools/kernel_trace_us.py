#!/usr/bin/env python3
"""Kernel time of one kernel from a `rocprofv3 --kernel-trace --output-format csv` directory: every dispatch whose name contains NAME
and that ran longer than --min-us (the launches that tracked blocks, not the empty launch that ends run()), with the mean duration
divided by --blocks (us per 1 ms block per launch) and by --blocks * --channels (us per block per channel).  Prints one JSON line.
usage: tools/kernel_trace_us.py DIR NAME --blocks B --channels K [--min-us 100]"""
import argparse
import csv
import glob
import json
import os


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("name")
    ap.add_argument("--blocks", type=float, required=True)
    ap.add_argument("--channels", type=int, required=True)
    ap.add_argument("--min-us", type=float, default=100.0)
    a = ap.parse_args()
    durs = []
    for path in glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                if a.name in row["Kernel_Name"]:
                    us = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
                    if us >= a.min_us:
                        durs.append(us)
    mean = sum(durs) / len(durs) if durs else float("nan")
    print(json.dumps(dict(kernel=a.name, K=a.channels, dispatches=len(durs), kernel_us=durs, kernel_us_per_block=mean / a.blocks,
                          kernel_us_per_block_per_channel=mean / (a.blocks * a.channels))))


if __name__ == "__main__":
    main()
