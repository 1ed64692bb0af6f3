#!/usr/bin/env python3
"""GENERATION-TIME ONLY: the inputs of tests/golden/subst.tar.gz (make_subst.sh runs the reference on them).

    make_subst_inputs.py <outdir>

writes under <outdir>/subst the hand-made pairs of tests/tools/subst_cases.py — the edges of the mode 1 kernel: the lane's 16 residues, the
group's step of 128, the wavefront's step of 1024, the hand-over between the tiers, scores that return to 0, a best score reached twice,
`*` and `X`, the reverse strand, every gate on its threshold — as sequence DBs (prot: dbtype 0, nuclx: dbtype 1) with HAND-WRITTEN prefilter
DBs over them (pref_prot7, pref_nuclx7: dbtype 7; pref_nuclx14: dbtype 14, a negative score is a reverse-strand hit), the protein DB of the
linclust run (fam) and NAMES (sequence DB, key, the case's label, length).  Everything is seeded."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import subst_cases as cs  # noqa: E402


def main(out):
    dbs = cs.write_all(out)
    cs.write_family(out)
    with open(os.path.join(out, "subst", "NAMES"), "w") as fd:
        for name in ("prot", "nuclx"):
            for label, k in sorted(dbs[name].label.items(), key=lambda kv: kv[1]):
                fd.write("%s\t%d\t%s\t%d\n" % (name, k, label, len(dbs[name].seqs[k])))
    with open(os.path.join(out, "subst", "RUNLIST"), "w") as fd:      # (read by make_subst.sh, not part of the tarball)
        for db, pref in cs.COMBOS:
            for name, flags in cs.RUNS:
                fd.write("%s_%s\t%s\t%s\t%s\n" % (os.path.basename(pref), name, db, pref, flags))
    open(os.path.join(out, "subst", "LINFLAGS"), "w").write(cs.LINCLUST + "\n")


if __name__ == "__main__":
    main(sys.argv[1])
