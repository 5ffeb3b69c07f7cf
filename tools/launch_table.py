"""Per-step launch table from rocprofv3 kernel traces: python tools/launch_table.py DIR [DIR ...]  (DIR holds *_kernel_trace.csv).
Every launch of a step in launch order with its median duration (us) over the last 8 complete steps; a step ends at the iSTFT."""
import csv
import glob
import re
import statistics
import sys


def load(d):
    """(kernel name, median us) per launch of a step, and how many steps the medians are taken over"""
    f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))]
    rows.sort()
    # the iSTFT kernel is the last launch of a step: cut after each one; what precedes the first cut (warm-up, weight
    # preparation) is dropped
    ends = [i for i, r in enumerate(rows) if "istft" in r[2]]
    steps = [rows[a + 1:b + 1] for a, b in zip(ends, ends[1:])]
    # a complete step has the usual number of launches; the last 8 of those
    L = statistics.mode(len(s) for s in steps)
    steps = [s for s in steps if len(s) == L][-8:]
    out = []
    for i in range(L):
        nm = steps[0][i][2]
        assert all(s[i][2] == nm for s in steps)
        out.append((nm, statistics.median((s[i][1] - s[i][0]) / 1e3 for s in steps)))
    return out, len(steps)


def short(n):
    n = re.sub(r"\(anonymous namespace\)::", "", n)
    return re.sub(r"\(.*", "", n)[:60]


if __name__ == "__main__":
    for d in sys.argv[1:]:
        o, n = load(d)
        print("==", d, "launches/step", len(o), "steps used", n, "sum us", round(sum(x[1] for x in o), 1))
        for i, (nm, us) in enumerate(o):
            print(i, short(nm), round(us, 1))
