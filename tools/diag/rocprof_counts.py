"""Sums up the csv traces of one rocprofv3 run (--kernel-trace --memory-copy-trace --output-format csv -d DIR): launches per kernel and copies per direction."""
import collections
import csv
import glob
import os
import re
import sys


def rows(d, suffix):
    for f in sorted(glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True)):
        with open(f, newline="") as fh:
            yield from csv.DictReader(fh)


def main(d):
    k = collections.Counter(re.sub(r"\s*\[clone.*$", "", r.get("Kernel_Name", "?")) for r in rows(d, "kernel_trace.csv"))
    print("kernel launches: %d" % sum(k.values()))
    for name in sorted(k):
        print("  %5d  %s" % (k[name], name[:140]))
    c = collections.Counter(r.get("Direction", "?") for r in rows(d, "memory_copy_trace.csv"))
    print("memory copies: %d" % sum(c.values()))
    for name in sorted(c):
        print("  %5d  %s" % (c[name], name))


if __name__ == "__main__":
    main(sys.argv[1])
