#!/usr/bin/env python3
"""timeline_lag.py <rocprofv3 --kernel-trace output dir>: for every scan and shade dispatch of a kernel trace -- wait behind its predecessor on the same queue, and when the other queues' traversal that ran
during that wait ended relative to the dispatch's start."""
import csv, glob, os, sys, statistics as st
d = sys.argv[1]
f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
rows = []
for r in csv.DictReader(open(f)):
    n = r["Kernel_Name"].replace("void ", "").split("(")[0].split("<")[0]
    if not n.startswith(("kPt", "kScan")): continue
    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Queue_Id"], n, int(r["Grid_Size_X"] if "Grid_Size_X" in r else r["Grid_Size"])))
rows.sort()
rows = rows[len(rows) // 2:]  # the second half: timed steps, past warm-up
byq = {}
for r in rows: byq.setdefault(r[2], []).append(r)
print("queues:", {q: len(v) for q, v in byq.items()})
out = {}
for q, v in byq.items():
    for k in range(1, len(v)):
        s, e, _, n, g = v[k]
        if not (n.startswith("kScan") or n.startswith("kPtShade")): continue
        pe = v[k - 1][1]
        lag = (s - pe) / 1e3  # us
        # traversal dispatches of other queues that were running at pe (predecessor's end)
        oth = [o for qq, vv in byq.items() if qq != q for o in vv if o[3].startswith("kPtTraceStream") and o[0] <= pe < o[1]]
        big = [o for o in oth if o[4] >= 64 * 1000]
        rel = min(((s - o[1]) / 1e3 for o in big), default=None)  # start minus the other traversal's end: > 0 = started after it ended, < 0 = started while it ran
        relend = min(((e - o[1]) / 1e3 for o in big), default=None)  # end minus the sibling traversal's end
        out.setdefault(n, []).append((lag, rel, (e - s) / 1e3, len(big), relend))
for n, v in sorted(out.items()):
    lags = [x[0] for x in v]
    withO = [x for x in v if x[3] > 0]
    noO = [x for x in v if x[3] == 0]
    dur = [x[2] for x in v]
    print("%-18s n=%4d  wait behind predecessor us: median %8.1f p90 %8.1f max %8.1f sum %9.1f | duration us median %8.1f sum %10.1f" % (
        n, len(v), st.median(lags), sorted(lags)[int(len(lags) * 0.9)], max(lags), sum(lags), st.median(dur), sum(dur)))
    if withO:
        l = [x[0] for x in withO]; r = [x[1] for x in withO]
        print("    sibling traversal (full grid) running at predecessor's end: n=%4d wait median %8.1f sum %9.1f | start - sibling's end us: median %8.1f  (>= -50: %d of %d)" % (
            len(withO), st.median(l), sum(l), st.median(r), sum(1 for x in r if x >= -50), len(r)))
        d2 = [x[2] for x in withO]; re = [x[4] for x in withO]
        print("    ... their duration us: median %8.1f sum %10.1f | end - sibling traversal's end us: median %8.1f min %8.1f max %8.1f (ended before it: %d of %d)" % (
            st.median(d2), sum(d2), st.median(re), min(re), max(re), sum(1 for x in re if x < 0), len(re)))
        d3 = [x[2] for x in noO]
        if d3: print("    ... duration us without a sibling traversal: median %8.1f sum %10.1f" % (st.median(d3), sum(d3)))
    if noO:
        l = [x[0] for x in noO]
        print("    no sibling traversal running:                              n=%4d wait median %8.1f sum %9.1f" % (len(noO), st.median(l), sum(l)))
span = (rows[-1][1] - rows[0][0]) / 1e6
print("span of analysed half: %.2f ms, dispatches %d" % (span, len(rows)))
