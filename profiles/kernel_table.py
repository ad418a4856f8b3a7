#!/usr/bin/env python3
"""Per (kernel, grid) table out of a rocprofv3 --kernel-trace CSV: calls, total and mean microseconds.  The --stats summary
adds up every launch of a kernel name; a kernel that runs at several shapes (resize2x_bwd_kernel, the fills) needs the grid to
tell the head-shape launch from the others.  usage: kernel_table.py p_kernel_trace.csv [name substring ...] > table.csv"""
import collections
import csv
import re
import sys


def short(name):
    name = re.sub(r'^_ZN12_GLOBAL__N_1\d+', '', name)
    f = re.search(r'FillFunctor<([^>]*)>', name)
    if f:
        return 'aten_fill<%s>' % f.group(1)
    m = re.search(r'(\w+_kernel|\w+Functor<[^>]*>|__amd_\w+)', name)
    return m.group(1) if m else name[:60]


def main():
    want = sys.argv[2:]
    rows = collections.OrderedDict()
    with open(sys.argv[1], newline='') as f:
        for r in csv.DictReader(f):
            name = short(r['Kernel_Name'])
            if want and not any(w in name for w in want):
                continue
            key = (name, int(r['Grid_Size_X']), int(r['Grid_Size_Y']), int(r['Workgroup_Size_X']))
            d = rows.setdefault(key, [0, 0])
            d[0] += 1
            d[1] += int(r['End_Timestamp']) - int(r['Start_Timestamp'])
    out = csv.writer(sys.stdout)
    out.writerow(['kernel', 'grid_x', 'grid_y', 'workgroup', 'calls', 'total_us', 'mean_us'])
    for (name, gx, gy, wg), (n, ns) in sorted(rows.items(), key=lambda kv: -kv[1][1]):
        out.writerow([name, gx, gy, wg, n, '%.1f' % (ns / 1e3), '%.1f' % (ns / 1e3 / n)])


if __name__ == '__main__':
    main()
