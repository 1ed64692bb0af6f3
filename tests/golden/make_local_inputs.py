#!/usr/bin/env python3
"""GENERATION-TIME ONLY: the inputs of tests/golden/local.tar.gz (make_local.sh runs the reference on them).

    make_local_inputs.py <outdir>

writes the hand-made pairs of tests/tools/local_cases.py — the edges of the mode 2 kernel: the lane's 16 residues, the step's 1024, ties of
the maximum and of the running minimum, both signs of the diagonal, the +-65536 wraps, the reverse strand, every gate on its threshold — as
small sequence DBs (nucl: dbtype 1, prot: dbtype 0) and HAND-WRITTEN prefilter DBs over them (pref_nucl7, pref_prot7: dbtype 7; pref_nucl14:
dbtype 14, a negative score is a reverse-strand hit), and NAMES (sequence DB, key, the case's label, length).  Everything is seeded."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import local_cases as cs  # noqa: E402


def main(out):
    dbs = cs.write_all(out)
    with open(os.path.join(out, "NAMES"), "w") as fd:
        for name in ("nucl", "prot"):
            for label, k in sorted(dbs[name].label.items(), key=lambda kv: kv[1]):
                fd.write("%s\t%d\t%s\t%d\n" % (name, k, label, len(dbs[name].seqs[k])))


if __name__ == "__main__":
    main(sys.argv[1])
