"""Reduce a rocprofv3 kernel_trace.csv to what is needed: per-kernel stats of selected kernels and the timeline of two consecutive late steps.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python3 bench.py --steps 50 --warmup 10 --no-cpu-baseline --no-standin
    python tools/trace_summary.py DIR/NAME_kernel_trace.csv step      (or: ... alone, for a trace of tools/bench_kernels.py --sort)

The csv of a bench run is ~100 MB: reduce it where it was written and keep the summary."""
import collections
import csv
import re
import sys

path, mode = sys.argv[1], sys.argv[2]
rows = []
with open(path) as f:
    for x in csv.DictReader(f):
        rows.append((int(x["Start_Timestamp"]), int(x["End_Timestamp"]), x["Kernel_Name"], x.get("Queue_Id", "")))
rows.sort()


def short(n):
    n = re.sub(r"^void ", "", n)
    n = n.replace("snerf::", "")
    return n[:90]


sel = re.compile(r"sort_|scan_|mlp_bwd|scatter_halfwave|field_fwd|ray_train|adam_planes|density_bwd")
d = collections.defaultdict(list)
late = rows[len(rows) // 2:] if mode == "step" else rows
for s, e, n, q in late:
    if sel.search(n):
        d[short(n)].append((e - s) / 1e3)
print(f"# {path}: {len(rows)} kernel records; stats over the {'second half of the run' if mode == 'step' else 'whole run'} (us)")
for k, v in sorted(d.items()):
    v = sorted(v)
    print(f"{k:92s} n={len(v):5d} median {v[len(v) // 2]:8.1f} mean {sum(v) / len(v):8.1f} min {v[0]:8.1f} max {v[-1]:8.1f}")
if mode == "step":
    ff = [i for i, r in enumerate(rows) if "field_fwd" in r[2]]
    if len(ff) < 4:
        sys.exit(f"{path}: {len(ff)} field_fwd records, need at least 4 (two complete late steps) for the timeline")
    i0, i1 = ff[-4], ff[-2]
    t0 = rows[i0][0]
    print("# two consecutive steps, offsets in us from the first field forward's start: start end duration queue kernel")
    for s, e, n, q in rows[i0:i1 + 1]:
        print(f"{(s - t0) / 1e3:9.1f} {(e - t0) / 1e3:9.1f} {(e - s) / 1e3:8.1f} q{q:>3s} {short(n)}")
else:
    srt = [r for r in rows if "sort_" in r[2]]
    for grp in (srt[len(srt) // 2 - 4: len(srt) // 2], srt[-4:]):
        t0 = grp[0][0]
        print("# one sort, offsets in us")
        for s, e, n, q in grp:
            print(f"{(s - t0) / 1e3:9.1f} {(e - t0) / 1e3:9.1f} {(e - s) / 1e3:8.1f} {short(n)}")
