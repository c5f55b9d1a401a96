"""Per-step sum, spread and launch count of the kernels that serve the fine cross correlation, from a
rocprofv3 kernel trace of bench.py (steps delimited by the rasterizer's render_kernel as in prof_steps.py):
the table route's flip, two splits, K = 3C library GEMM and table gather, or the fused route's pack and
fused kernels. usage: uv_cross_per_step.py run_kernel_trace.csv"""
import csv, sys
rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
ends = [int(r["End_Timestamp"]) for r in rows if "render_kernel" in r["Kernel_Name"]]
spans = list(zip(ends[4:-2], ends[5:-1]))
def serves(r):
    n = r["Kernel_Name"]
    if "uv_cross" in n or "split3" in n: return True
    if "Cijk" in n and "BSS_BH" in n and "MT256x256x32" in n: return True
    if "flip" in n: return True
    return False
import statistics
per = []; names = {}
for lo, hi in spans:
    t = 0; c = 0
    for r in rows:
        e = int(r["End_Timestamp"])
        if lo < e <= hi and serves(r):
            d = e - int(r["Start_Timestamp"]); t += d; c += 1
            k = r["Kernel_Name"][:60]; a = names.setdefault(k, [0, 0]); a[0] += d; a[1] += 1
    per.append((t / 1e3, c))
ts = [p[0] for p in per]
print(f"steps {len(per)}: correlation kernels per step mean {statistics.mean(ts):.1f} us, min {min(ts):.1f}, max {max(ts):.1f}, "
      f"stdev {statistics.pstdev(ts):.2f}; launches per step {sorted(set(p[1] for p in per))}")
walls = [(hi - lo) / 1e3 for lo, hi in spans]
print(f"wall per step mean {statistics.mean(walls):.1f} us, min {min(walls):.1f}, max {max(walls):.1f}")
for k, (t, c) in sorted(names.items(), key=lambda kv: -kv[1][0]):
    print(f"  {t / len(per) / 1e3:7.1f} us/step  {c / len(per):4.1f} calls/step  avg {t / c / 1e3:6.1f} us  {k}")
