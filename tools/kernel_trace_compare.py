"""python tools/kernel_trace_compare.py DIR_A DIR_B  --  compares two `rocprofv3 --kernel-trace --output-format csv` output directories by the library's
kernels: the multiset of (kernel name, number of launches), names containing "brmi".  Prints one JSON line; `equal` is the verdict, `only_a` / `only_b` list
the names whose counts differ."""
import collections
import csv
import glob
import json
import sys


def names(directory):
    c = collections.Counter()
    for f in glob.glob(directory + "/**/*kernel_trace.csv", recursive=True):
        for row in csv.DictReader(open(f)):
            n = row.get("Kernel_Name") or row.get("kernel_name")
            if n and "brmi" in n:
                c[n] += 1
    return c


def main():
    a, b = names(sys.argv[1]), names(sys.argv[2])
    print(json.dumps({"launches_a": sum(a.values()), "launches_b": sum(b.values()), "distinct_a": len(a), "distinct_b": len(b), "equal": a == b and len(a) > 0,
                      "only_a": {k: v for k, v in a.items() if b.get(k) != v}, "only_b": {k: v for k, v in b.items() if a.get(k) != v}}))


if __name__ == "__main__":
    main()
