"""Per-kernel times inside the replayed step from a rocprofv3 kernel trace: for every (kernel name with its template arguments,
grid) whose name contains one of the given substrings, the median / minimum / maximum duration over its LAST n launches (the
timed steps of bench.py: the warm-ups, the capture and the capacity pre-pass come first).
usage: python tools/kernel_in_step.py <dir with *kernel_trace.csv> [n = 20] [substring ...]"""
import collections
import csv
import glob
import statistics
import sys

d = sys.argv[1]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
subs = sys.argv[3:] or ['k_agg_bwd_dst<', 'k_mlp2_bwd_first3<']
f = (glob.glob(d + '/**/*kernel_trace.csv', recursive=True) + glob.glob(d + '/*kernel_trace.csv'))[0]
rows = list(csv.DictReader(open(f)))
rows.sort(key=lambda r: int(r['Start_Timestamp']))
by = collections.defaultdict(list)
for r in rows:
    name = r['Kernel_Name'].replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0]
    if any(s in name for s in subs):
        by[(name, r.get('Grid_Size_X', r.get('Grid_Size', '?')))].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
for (name, grid), v in sorted(by.items()):
    last = v[-n:]
    print('%-44s grid %-9s launches %4d  last %2d: median %7.2f  min %7.2f  max %7.2f us' % (
        name[:44], grid, len(v), len(last), statistics.median(last), min(last), max(last)))
