"""kernel trace csv -> per (kernel, grid) launch means, medians and launch-to-launch standard deviations in us;
usage: trace_by_grid.py DIR OUT.csv"""
import csv, glob, statistics, sys, collections
d, out = sys.argv[1], sys.argv[2]
f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
acc = collections.defaultdict(list)
for r in csv.DictReader(open(f)):
    name = r["Kernel_Name"].split("(")[0]
    grid = (r.get("Grid_Size_X") or r.get("Grid_Size"), r.get("Grid_Size_Y"))
    acc[(name, grid)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
rows = sorted(acc.items(), key=lambda kv: -sum(kv[1]))
with open(out, "w") as o:
    o.write("kernel,grid_x,grid_y,calls,mean_us,median_us,total_us,std_us\n")
    for (name, grid), v in rows:
        v = sorted(v)
        o.write(f"\"{name}\",{grid[0]},{grid[1]},{len(v)},{sum(v)/len(v):.2f},{v[len(v)//2]:.2f},{sum(v):.1f},{statistics.pstdev(v):.2f}\n")
for (name, grid), v in rows[:14]:
    v = sorted(v)
    print(f"{name[:70]:70s} grid {grid} n {len(v):4d} mean {sum(v)/len(v):8.1f} med {v[len(v)//2]:8.1f} std {statistics.pstdev(v):6.1f}")
