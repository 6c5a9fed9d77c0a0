#!/usr/bin/env python3
"""Wall time of `taxor profile` on a seeded synthetic search TSV: N reads over 2000 references, 70 % with one
match, 20 % with 2-6 matches, 10 % without a hit.  Prints the command's own timing line (parse / device / write) and the TSV's size.
Run:  python profiles/profile_cli.py [reads, default 1000000] > profiles/r08/profile_cli.txt"""
import os
import random
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "#QUERY_NAME\tACCESSION\tREFERENCE_NAME\tTAXID\tREF_LEN\tQUERY_LEN\tQHASH_COUNT\tQHASH_MATCH\tTAX_STR\tTAX_ID_STR\n"


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
    rng = random.Random(1)
    F = 2000
    weight = [1.0 / (1 + i) ** 0.7 for i in range(F)]
    sp = [(f"GCF_{100000 + i}.1", f"{5000 + i}", 2000000 + 1000 * (i % 3000),
           f"k__Bacteria;p__P{i % 7};c__C{i % 19};o__O{i % 53};f__F{i % 131};g__G{i % 400};s__Species {i}",
           f"2;{10 + i % 7};{100 + i % 19};{1000 + i % 53};{2000 + i % 131};{3000 + i % 400};{5000 + i}") for i in range(F)]
    with tempfile.TemporaryDirectory() as d:
        tsv = os.path.join(d, "search.tsv")
        with open(tsv, "w") as f:
            f.write(HEADER)
            out = []
            for r in range(n):
                u = rng.random()
                q = rng.randrange(1000, 20000)
                c = q // 11
                name = f"read_{r} runid=abc ch={r % 512}"
                if u < 0.1:
                    out.append(f"{name}\t-\t-\t-\t-\t{q}\n")
                else:
                    m = 1 if u < 0.8 else rng.randrange(2, 7)
                    first = rng.choices(range(F), weight)[0]
                    for j in range(m):
                        a = sp[(first + j * 400) % F]                 # relatives: the same genus index
                        out.append(f"{name}\t{a[0]}\tn\t{a[1]}\t{a[2]}\t{q}\t{c}\t{rng.randrange(c // 3, c) + 1}\t{a[3]}\t{a[4]}\n")
                if len(out) > 100000:
                    f.write("".join(out))
                    out = []
            f.write("".join(out))
        print(f"{n} reads, search TSV {os.path.getsize(tsv) / 1e6:.1f} MB")
        for rep in range(2):
            t0 = time.time()
            cp = subprocess.run([os.path.join(ROOT, "taxor_amd", "taxor"), "profile", "--search-file", tsv, "--cami-report-file",
                                 os.path.join(d, "cami"), "--seq-abundance-file", os.path.join(d, "seq"), "--binning-file", os.path.join(d, "bin"),
                                 "--sample-id", "bench"], capture_output=True, text=True)
            print(f"run {rep}: exit {cp.returncode}, {time.time() - t0:.3f} s wall;", cp.stdout.strip())
            print(cp.stderr.strip())
            if cp.returncode != 0:
                sys.exit(1)


if __name__ == "__main__":
    main()
