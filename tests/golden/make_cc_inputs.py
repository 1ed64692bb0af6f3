#!/usr/bin/env python3
"""GENERATION-TIME ONLY: the hand-written inputs of tests/golden/cc.tar.gz (make_cc.sh runs the reference on them).

    make_cc_inputs.py <outdir>

writes the hand-made graphs of tests/tools/cc_cases.py (hand_made: what each is there for is said beside it) as small nucleotide sequence DBs
<name> and result DBs <name>_res of dbtype 7, 14 and 5 over them, and RUNLIST: one line per `clust --cluster-mode 1` run — name, sequence DB,
result DB, the extra flags.  Everything is seeded."""
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import cc_cases  # noqa: E402


def main(out):
    os.makedirs(out, exist_ok=True)
    rnd = random.Random(20261020)
    with open(os.path.join(out, "RUNLIST"), "w") as runs:
        for name, seqs, lists, dbtype, flags, skip in cc_cases.hand_made(rnd):
            cc_cases.write_case(out, name, seqs, lists, dbtype, rnd, skip)
            runs.write("%s\tcc/%s\tcc/%s_res\t%s\n" % (name, name, name, ("--cluster-mode 1 " + flags).strip()))


if __name__ == "__main__":
    main(sys.argv[1])
