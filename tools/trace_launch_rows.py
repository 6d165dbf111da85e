"""Rows of a rocprofv3 kernel trace by ordinal inside one replayed UNet step (the 256x160 f16 pipe-kernel launches between two step_kernel rows) or inside one
VAE decode (launches over 300 us between two to_u8_kernel rows) -- for library A/Bs of single launches (profiles/upsample_fold_ab.txt).
usage: trace_launch_rows.py step|decode <rocprofv3 output dir>"""
import csv, glob, sys
mode, d = sys.argv[1], sys.argv[2]
f = sorted(glob.glob(d + "/**/*kernel_trace.csv", recursive=True))[0]
rows = []
for r in csv.DictReader(open(f)):
    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0], r.get("Grid_Size_X", r.get("Grid_Size", ""))))
rows.sort()
if mode == "step":
    idx = [i for i, r in enumerate(rows) if r[2].split("<")[0].endswith("step_kernel")]
    for a, b in ((idx[-4], idx[-3]), (idx[-3], idx[-2])):
        seg = rows[a + 1:b + 1]
        print("step span %.3f ms, %d dispatches" % ((seg[-1][1] - rows[a][1]) / 1e6, len(seg)))
        for o, (s, e, n, g) in enumerate(seg):
            if "256, 160" in n or "Li256ELi160E" in n: print("   ordinal %3d  %8.1f us  grid %s  %s" % (o, (e - s) / 1e3, g, n[-70:]))
else:
    ends = [i for i, r in enumerate(rows) if "to_u8" in r[2]]
    for a, b in ((ends[-3], ends[-2]), (ends[-2], ends[-1])):
        seg = rows[a + 1:b + 1]
        print("decode span %.3f ms, %d dispatches, kernel time %.3f ms" % ((seg[-1][1] - rows[a][1]) / 1e6, len(seg), sum(e - s for s, e, _, _ in seg) / 1e6))
        for o, (s, e, n, g) in enumerate(seg):
            if e - s > 300e3: print("   ordinal %3d  %8.1f us  grid %s  %s" % (o, (e - s) / 1e3, g, n[-70:]))
