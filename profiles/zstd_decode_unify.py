"""Merges runs of profiles/zstd_decode_lab.py made with two commits' packages into one record and
applies the project's rule to the decode kernels: the new median GiB/s must not be below the
parent's by more than the larger min-max spread of the two.

    python profiles/zstd_decode_lab.py --layouts sharded --gib 0.25 --tree <parent checkout> \
        --out parent_1.json        (and new_1.json with this checkout, parent_2.json, new_2.json:
                                    the two packages in turn on one device)
    python profiles/zstd_decode_unify.py --parent parent_1.json parent_2.json \
        --new new_1.json new_2.json [--out profiles/zstd_decode/unify_lab.json]"""
import argparse
import json
import os
import statistics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--parent", nargs="+", required=True)
ap.add_argument("--new", nargs="+", required=True)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zstd_decode", "unify_lab.json"))
a = ap.parse_args()
out = {"lab": "profiles/zstd_decode_lab.py --layouts sharded --gib 0.25 --repeats 5, the parent "
              "commit's package (--tree) and this one's in turn, %d and %d processes, one MI355X" % (len(a.parent), len(a.new)),
       "rule": "the new median of the decode kernels' GiB/s must not be below the parent's by more "
               "than the larger min-max spread of the two",
       "arrays": {}}
runs = {w: [json.load(open(p)) for p in paths]
        for w, paths in (("parent", a.parent), ("new", a.new))}
ok = True
for key in runs["new"][0]["arrays"]:
    row = {}
    for w in ("parent", "new"):
        gib = runs[w][0]["arrays"][key]["decoded_bytes"] / (1 << 30)
        ms = [m for r in runs[w] for m in r["arrays"][key]["kernel"]["ms"]]
        rate = [gib / (m / 1e3) for m in ms]
        row[w] = {"kernel_ms": ms, "median_GiB_per_s": round(statistics.median(rate), 2),
                  "spread_GiB_per_s": round(max(rate) - min(rate), 2),
                  "host_route_median_ms": [r["arrays"][key]["host_route"]["median_ms"] for r in runs[w]],
                  "device_route_median_ms": [r["arrays"][key]["device_route"]["median_ms"]
                                             for r in runs[w]]}
    margin = max(row["parent"]["spread_GiB_per_s"], row["new"]["spread_GiB_per_s"])
    row["margin_GiB_per_s"] = margin
    row["holds"] = row["new"]["median_GiB_per_s"] >= row["parent"]["median_GiB_per_s"] - margin
    ok = ok and row["holds"]
    out["arrays"][key] = row
    print(key, row["parent"]["median_GiB_per_s"], row["parent"]["spread_GiB_per_s"],
          row["new"]["median_GiB_per_s"], row["new"]["spread_GiB_per_s"], row["holds"])
out["holds"] = ok
with open(a.out, "w") as fh:
    json.dump(out, fh, indent=1)
