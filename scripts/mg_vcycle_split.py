"""Split of a multigrid V-cycle's kernel time by level, from a `rocprofv3 --kernel-trace --stats --output-format csv` run of
`python scripts/sweep_mg_tail.py --worker n steps`.

    python scripts/mg_vcycle_split.py <..._kernel_trace.csv> [out.json] [device levels above the tail = 5]

A cycle is found around every k_mg_tail launch: the 3 launches per device level before it (scale, pre-sweep, residual +
restriction; on level 0 both pre-sweeps in one SpMV launch, the residual in another, the restriction of that vector) and the 3 per level after it (prolongation + correction, two post-sweeps); level 0's sweeps are the SpMV's mode 8
(k_spmv_s<8>).  Cycles queued past convergence (the tail returned at the done flag, < 5 us) are left out.  Kernel durations
only: the gaps between launches are not in them."""
import collections
import csv
import json
import re
import statistics
import sys

path = sys.argv[1]
out = sys.argv[2] if len(sys.argv) > 2 else "profiles/mg_vcycle_split.json"
NL = int(sys.argv[3]) if len(sys.argv) > 3 else 5
rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))


def short(name):
    m = re.search(r"(k_[a-z_0-9]+)(<\d+)?", name)
    return (m.group(1) + (m.group(2) + ">" if m.group(2) else "")) if m else name[:30]


ev = [(short(r["Kernel_Name"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for r in rows]
DOWN, UP = ("k_mg_scale", "k_mg_jacobi", "k_mg_restrict", "k_mg_restrict_vec", "k_spmv_s<8>"), ("k_mg_prolong", "k_mg_jacobi", "k_spmv_s<8>")
per, cycles = collections.defaultdict(list), 0
for t in [i for i, e in enumerate(ev) if e[0] == "k_mg_tail"]:
    back, i = [], t - 1
    while len(back) < 3 * NL and i >= 0:
        if ev[i][0] in DOWN:
            back.append(ev[i])
        i -= 1
    fwd, i = [], t + 1
    while len(fwd) < 3 * NL and i < len(ev):
        if ev[i][0] in UP:
            fwd.append(ev[i])
        i += 1
    if len(back) < 3 * NL or len(fwd) < 3 * NL or ev[t][1] < 5000:
        continue
    back.reverse()
    cycles += 1
    for l in range(NL):
        names = ("scale", "pre-sweep", "residual + restriction")
        if back[3 * l + 2][0] == "k_mg_restrict_vec":      # level 0 through the SpMV: three launches of another kind
            names = ("both pre-sweeps (one Horner launch)", "residual (Horner launch)", "restriction of the residual vector")
        for k, e in zip(names, back[3 * l:3 * l + 3]):
            per[(l, k)].append(e[1])
        for k, e in zip(("prolongation + correction", "post-sweep 1", "post-sweep 2"), fwd[3 * (NL - 1 - l):3 * (NL - l)]):
            per[(l, k)].append(e[1])
    per[("tail", "k_mg_tail")].append(ev[t][1])
kern = {f"level {k[0]}: {k[1]}": round(statistics.mean(v) / 1e3, 2) for k, v in sorted(per.items(), key=str)}
lev = collections.defaultdict(float)
for k, v in per.items():
    lev[str(k[0])] += statistics.mean(v) / 1e3
res = dict(what="mean kernel time per V-cycle, microseconds", trace=path, cycles=cycles, per_kernel_us=kern,
           per_level_us={k: round(v, 1) for k, v in lev.items()}, cycle_us=round(sum(lev.values()), 1))
print(json.dumps(res, indent=1))
with open(out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
