"""How much of every k_front_fold and k_copy_result launch runs beside a heavy
kernel (k_front, k_count3c) of the other context, from a rocprofv3
--kernel-trace CSV.

usage: python tools/trace_overlap.py DIR_OR_CSV [--json OUT]

A stream runs its kernels in order, so a k_front or k_count3c interval that
overlaps a fold or copy launch in time belongs to another stream; where the
trace has a queue or stream column, launches of the light kernel's own queue
are excluded as well.  Per light kernel: launches, median duration, the mean
share of a launch's duration covered by the other stream's k_front, by its
k_count3c and by either, the share of launches with no heavy kernel beside
them at all, and the mean time per launch spent with none beside it."""
import argparse
import bisect
import csv
import glob
import json
import os

LIGHT = ("k_front_fold", "k_copy_result")
HEAVY = ("k_front", "k_count3c")


def short(name):
    n = name.split("(")[0].replace("void ", "")
    n = n.split("<")[0]
    return n.split("::")[-1]


def load(path):
    files = [path] if path.endswith(".csv") else glob.glob(os.path.join(path, "**", "*kernel_trace.csv"),
                                                            recursive=True)
    rows = []
    for f in files:
        for r in csv.DictReader(open(f)):
            q = r.get("Queue_Id") or r.get("Stream_Id") or ""
            rows.append((short(r["Kernel_Name"]), int(r["Start_Timestamp"]), int(r["End_Timestamp"]), q))
    return rows


def union(iv):
    """The sorted disjoint union of intervals."""
    out = []
    for a, b in sorted(iv):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return out, [b for _, b in out]


def covered(s, e, iv, ends):
    """ns of [s, e) covered by the disjoint intervals iv."""
    tot = 0
    for a, b in iv[bisect.bisect_right(ends, s):]:
        if a >= e:
            break
        tot += min(b, e) - max(a, s)
    return tot


def report(rows):
    out = {}
    per_queue = len({q for _, _, _, q in rows}) > 1
    cache = {}

    def beside(names, q):
        """The union of the launches of `names` that are not on queue q."""
        key = (names, q if per_queue else "")
        if key not in cache:
            cache[key] = union((a, b) for n, a, b, hq in rows if n in names and not (per_queue and hq == q))
        return cache[key]

    for light in LIGHT:
        ls = [r for r in rows if r[0] == light]
        if not ls:
            continue
        rec = {"launches": len(ls), "median_us": sorted((e - s) / 1e3 for _, s, e, _ in ls)[len(ls) // 2]}
        shares = {h: [] for h in HEAVY + ("either",)}
        alone_us = []
        for _, s, e, q in ls:
            for h in shares:
                c = covered(s, e, *beside(HEAVY if h == "either" else (h,), q))
                shares[h].append(c / max(1, e - s))
                if h == "either":
                    alone_us.append((e - s - c) / 1e3)
        for h, v in shares.items():
            rec[f"mean_share_beside_{h}"] = sum(v) / len(v)
        rec["share_of_launches_alone"] = sum(1 for v in shares["either"] if v == 0) / len(ls)
        rec["mean_alone_us"] = sum(alone_us) / len(alone_us)
        out[light] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("path")
    ap.add_argument("--json")
    a = ap.parse_args()
    rows = load(a.path)
    if not rows:
        raise SystemExit(f"no *kernel_trace.csv under {a.path}")
    out = report(rows)
    for k, rec in out.items():
        print(k, {x: (round(v, 4) if isinstance(v, float) else v) for x, v in rec.items()})
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
