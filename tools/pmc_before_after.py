"""Before / after summary of tools/pmc_passes.sh runs of tools/prof_run.py (one rocprofv3 --pmc
pass per counter group): per run directory the frame kernel's name, its DRAM bytes per frame
(FETCH_SIZE x2 + WRITE_SIZE, as tools/traffic_json.py), the L1 hit rate
(1 - TCP_TCC_READ_REQ / TCP_TOTAL_CACHE_ACCESSES) and the share of the data-return path's busy
cycles spent waiting on L1 misses (TD_TC_STALL / TD_TD_BUSY), each the mean over the frame
kernel's dispatches (the counting kernel prof_run.py launches once is left out).
Usage: python tools/pmc_before_after.py out.json name=dir [name=dir ...]
"""
import collections
import csv
import glob
import json
import os
import sys

from traffic_json import frame_kernel


def summarise(d):
    acc, kernels = collections.defaultdict(list), collections.Counter()
    for f in glob.glob(os.path.join(d, "p*", "**", "run_counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if frame_kernel(r["Kernel_Name"]):
                acc[r["Counter_Name"]].append(float(r["Counter_Value"]))
                kernels[r["Kernel_Name"]] += 1
    m = {k: sum(v) / len(v) for k, v in acc.items()}
    out = dict(kernel=kernels.most_common(1)[0][0] if kernels else None,
               dispatches={k: len(v) for k, v in acc.items()}, counters=m)
    for log in sorted(glob.glob(os.path.join(d, "p*.log")))[:1]:
        for line in open(log, errors="replace"):
            if line.startswith("{"):
                out["kernel_ms_under_profiler"] = json.loads(line)["kernel_ms"]
    if "FETCH_SIZE" in m:
        out["dram_read_gb"] = 2 * m["FETCH_SIZE"] * 1024 / 1e9
    if "WRITE_SIZE" in m:
        out["dram_write_gb"] = m["WRITE_SIZE"] * 1024 / 1e9
    if m.get("TCP_TOTAL_CACHE_ACCESSES_sum"):
        out["l1_hit_rate"] = 1 - m["TCP_TCC_READ_REQ_sum"] / m["TCP_TOTAL_CACHE_ACCESSES_sum"]
    if m.get("TD_TD_BUSY_sum"):
        out["td_tc_stall_over_td_busy"] = m["TD_TC_STALL_sum"] / m["TD_TD_BUSY_sum"]
    # address translation and the L1's read-request latency (tools/pmc_sets_tlb.txt)
    if "TCP_UTCL1_TRANSLATION_MISS_sum" in m:
        out["utcl1_translation_miss"] = m["TCP_UTCL1_TRANSLATION_MISS_sum"]
        if m.get("TCP_UTCL1_REQUEST_sum"):
            out["utcl1_miss_per_request"] = (m["TCP_UTCL1_TRANSLATION_MISS_sum"] /
                                             m["TCP_UTCL1_REQUEST_sum"])
    if "TCP_TCC_READ_REQ_LATENCY_sum" in m and m.get("TCP_TCC_READ_REQ_sum"):
        out["tcc_read_latency_cycles_per_request"] = (m["TCP_TCC_READ_REQ_LATENCY_sum"] /
                                                      m["TCP_TCC_READ_REQ_sum"])
    return out


def main():
    res = {}
    for arg in sys.argv[2:]:
        name, d = arg.split("=", 1)
        res[name] = summarise(d)
    json.dump(res, open(sys.argv[1], "w"), indent=1)
    for name, r in res.items():
        print(name, {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()
                     if k not in ("counters", "dispatches")})


if __name__ == "__main__":
    main()
