import collections, csv, glob, json, os, sys
O = sys.argv[1]
out = {}
for lib in ("parent", "new"):
    st = {}
    for f in glob.glob(os.path.join(O, "trace_" + lib, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            st[r["Name"][:90]] = {k: r[k] for k in ("Calls", "TotalDurationNs", "AverageNs", "Percentage") if k in r}
    top = dict(sorted(st.items(), key=lambda kv: -float(kv[1].get("TotalDurationNs", 0)))[:8])
    agg = collections.defaultdict(lambda: collections.defaultdict(float)); disp = collections.defaultdict(set)
    for f in glob.glob(os.path.join(O, "pmc_" + lib, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            k = r["Kernel_Name"].split("(")[0][:90]
            if "tb_kernel" not in k: continue
            agg[k][r["Counter_Name"]] += float(r["Counter_Value"]); disp[k].add(r["Dispatch_Id"])
    out[lib] = {"kernel_stats_top": top, "counters": {k: dict(v, dispatches=len(disp[k])) for k, v in agg.items()}}
print(json.dumps(out, indent=1))
