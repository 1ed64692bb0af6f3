"""Hand-made pairs at the edges of the mode 1 kernel (plass_amd/csrc/rescore_subst.hip): an eight-lane group walks a short pair in steps of
8 lanes x 16 residues, a wavefront a long one (min(qLen, tLen) > 1024) in steps of 64 x 16, so the cases sit at 1, 15, 16, 17, 127, 128, 129,
1023, 1024, 1025 and 2049 columns, on short overlaps of long pairs, on scores that fall to 0 and recover, on a best score reached twice, on
all-negative diagonals, on `*` and `X`, on the +-65536 wraps, on the reverse strand and on the thresholds of every gate.  The nucleotide
pairs of tests/tools/local_cases.py (local.tar.gz: local/nucl with pref_nucl14 and pref_nucl7) are run as they are; the DBs made here add
the protein pairs and the nucleotide lengths the mode 2 cases do not have.  Shared by tests/test_subst_host.py and tests/test_gpu_subst.py."""
import os
import random

import local_cases as lcs
import subst_check as sc

AA = "ACDEFGHIKLMNPQRSTVWY"
GROUP_MAX = 1024            # rescore_subst.hip, SB_GROUP_MAX: min(qLen, tLen) above it is the wavefront tier's

# (name, flags): the reference's flag names; --filter-hits 1 takes its threshold from the reference's table (RUNS of the fixture)
BASE = "--rescore-mode 1 --min-aln-len 0"
RUNS = [
    ("default", BASE + " -e 0.001 --min-seq-id 0.0 -c 0 --cov-mode 0 --filter-hits 0"),
    ("lax", BASE + " -e 10 --min-seq-id 0.0 -c 0 --cov-mode 0 --filter-hits 0"),
    ("alnlen1", "--rescore-mode 1 --min-aln-len 1 -e 10 --min-seq-id 0.0 -c 0 --cov-mode 0 --filter-hits 0"),
    ("cov", BASE + " -e 10 --min-seq-id 0.0 -c 0.5 --cov-mode 0 --filter-hits 0"),
    ("fh_target", BASE + " -e 0.001 --min-seq-id 0.99 -c 0.9 --cov-mode 1 --filter-hits 1"),
    ("fh_bidir", BASE + " -e 0.001 --min-seq-id 0.9 -c 0.8 --cov-mode 0 --filter-hits 1"),
    ("fh_lin", BASE + " -e 0.001 --min-seq-id 0.9 -c 0.8 --cov-mode 1 --filter-hits 1"),
    ("fh_norow", "--rescore-mode 1 --min-aln-len 200 -e 0.001 --min-seq-id 0.0 -c 0 --cov-mode 0 --filter-hits 1"),
]
# (sequence DB, prefilter DB) from the fixture's root; the local/ ones are local.tar.gz's
COMBOS = [("subst/prot", "subst/pref_prot7"), ("subst/nuclx", "subst/pref_nuclx14"), ("subst/nuclx", "subst/pref_nuclx7"),
          ("local/nucl", "local/pref_nucl14"), ("local/nucl", "local/pref_nucl7")]
# the protein linclust run (make_subst.sh); -k and --kmer-per-seq given: the automatic choice is the reference's alone
LINCLUST = ("--alignment-mode 4 --cluster-mode 2 --min-seq-id 0.9 -c 0.8 --cov-mode 1 -k 14 --kmer-per-seq 60 --kmer-per-seq-scale 0 --alph-size aa:13,nucl:5 "
            "--hash-shift 67 --ignore-multi-kmer 1 -e 0.001 --remove-tmp-files 0 --threads 1 -v 1")


def rnd_aa(r, n):
    return "".join(r.choice(AA) for _ in range(n))


def subst_aa(r, s, rate):
    x = list(s)
    for p in r.sample(range(len(s)), max(1, int(len(s) * rate)) if len(s) > 2 else 0):
        x[p] = r.choice(AA)
    return "".join(x)


def prot_cases():
    r = random.Random(20241020)
    c = lcs.Cases()
    # overlap lengths around the lane's 16 residues, the group's step of 128, the wavefront's step of 1024 and the hand-over between the tiers
    for n in (1, 15, 16, 17, 127, 128, 129, 300, 1023, 1024, 1025, 2049):
        q = rnd_aa(r, n)
        c.pair("len%d" % n, q, subst_aa(r, q, 0.08))
    # both signs of the diagonal on either tier; one sequence on either side of the hand-over
    for n in (200, 1500):
        q = rnd_aa(r, n)
        c.pair("neg%d" % n, q, rnd_aa(r, 5) + subst_aa(r, q, 0.05), diag=-5)
        c.pair("pos%d" % n, rnd_aa(r, 7) + q, subst_aa(r, q, 0.05), diag=7)
    q = rnd_aa(r, 1100)
    c.pair("mixed_tier", q, subst_aa(r, q[:900], 0.05))             # min(qLen, tLen) = 900: the group tier although the query is long
    # short overlaps of long pairs: the wavefront tier on 1, 17 and 129 columns
    for ov in (1, 17, 129):
        q = rnd_aa(r, 1100)
        c.pair("wave_ov%d" % ov, q, q[1100 - ov:] + rnd_aa(r, 1100 - ov), diag=1100 - ov)
    c.pair("miss", rnd_aa(r, 50), rnd_aa(r, 50), diag=50)           # the diagonal touches neither: no wrap scores
    # the best segment at position 0, at the last position, across a group step (128), a lane (16) and a wavefront step (1024)
    junk_q, junk_t = "W" * 1600, "P" * 1600                         # W against P: -4 a column
    s = rnd_aa(r, 40)
    c.pair("first", s + junk_q[:400], s + junk_t[:400])
    c.pair("last", junk_q[:400] + s, junk_t[:400] + s)
    c.pair("gstep", junk_q[:110] + s + junk_q[:50], junk_t[:110] + s + junk_t[:50])
    c.pair("lane", junk_q[:10] + s[:12] + junk_q[:30], junk_t[:10] + s[:12] + junk_t[:30])
    c.pair("wstep", junk_q[:1000] + s + junk_q[:500], junk_t[:1000] + s + junk_t[:500])
    # the best score reached twice (the same segment again behind a stretch that takes the running score to 0): on either tier
    c.pair("twice", s + junk_q[:100] + s, s + junk_t[:100] + s)
    c.pair("twice_wave", s + junk_q[:1200] + s, s + junk_t[:1200] + s)
    # nothing scores: the identity pair on a diagonal of W against P (kept whatever it scores: diagonal 0), an ordinary pair (never kept)
    k = c.add("allneg.self", "WP" * 40)
    c.lines[k].append((k, 5, 1))
    c.pair("allneg.pair", "W" * 33, "P" * 47)
    # identity pairs on their own diagonal, also listed twice, also with a diagonal that misses the sequence altogether
    k = c.add("self", rnd_aa(r, 300))
    c.lines[k] += [(k, 0, 0), (k, 9, 0), (k, 9, 301)]
    # `*` and `X`, lower case
    q = rnd_aa(r, 120)
    c.pair("xstar", q[:20] + "X" * 5 + q[25:60] + "*" + q[61:], q[:40] + "*" + q[41:58] + "XX" + q[60:100].lower() + q[100:])
    # canBeCovered (runs fh_target: -c 0.9 --cov-mode 1; fh_lin, fh_bidir: -c 0.8) met with equality and missed by one residue
    q = rnd_aa(r, 100)
    c.pair("cancover_eq", q[:90], q)
    c.pair("cancover_below", q[:89], q)
    c.pair("cancover8_eq", q[:80], q)
    c.pair("cancover8_below", q[:79], q)
    # coverage by the diagonal's length (run cov: -c 0.5 --cov-mode 0 with nothing else in the way): 50 and 49 of 100 columns
    c.pair("cov_eq", q, q[50:] + junk_t[:50], diag=50)
    c.pair("cov_below", q, q[51:] + junk_t[:51], diag=51)
    # a ladder of raw scores against one query length: -e 0.001 falls between two of its rungs
    q = rnd_aa(r, 60)
    for m in range(2, 24, 2):
        c.pair("evalue%d" % m, q, q[:m] + "".join("P" if a == "W" else "W" for a in q[m:]))
    return c


def nuclx_cases():
    """the nucleotide lengths local_cases does not have, and the tiers"""
    r = random.Random(77)
    c = lcs.Cases()
    for n in (127, 128, 129):
        q = lcs.rnd(r, n)
        c.pair("len%d" % n, q, lcs.mutate(q, [n // 3, n // 2]))
    # the reverse strand on either tier, the end of the overlap inside a lane
    for n in (333, 1301):
        q = lcs.rnd(r, n)
        c.pair("rev%d" % n, q, lcs.revcomp(lcs.mutate(q, [n // 4, n // 2])), diag=0, score=-9)
    q = lcs.rnd(r, 1200)
    c.pair("rev_shift", lcs.rnd(r, 40) + q, lcs.revcomp(q)[:1100], diag=0, score=-2)
    # +6 -6 repeated: the running score falls to exactly 0 and recovers, in a lane, across lanes, across group steps
    for label, reps in (("zeros_lane", 2), ("zeros_group", 20), ("zeros_steps", 60)):
        q = lcs.rnd(r, 5 * reps + 30)
        c.pair(label, q, lcs.mutate(q, [5 * i + j for i in range(reps) for j in (3, 4)] + list(range(5 * reps + 20, 5 * reps + 30))))
    # short overlap of a long pair
    q = lcs.rnd(r, 1500)
    c.pair("wave_ov20", q, q[1480:] + lcs.rnd(r, 1400), diag=1480)
    return c


def write_all(root):
    """the DBs made here under `root`/subst: prot (dbtype 0) with pref_prot7, nuclx (dbtype 1) with pref_nuclx14 and pref_nuclx7 -> {name: Cases}"""
    d = os.path.join(root, "subst")
    os.makedirs(d, exist_ok=True)
    p, n = prot_cases(), nuclx_cases()
    lcs.write_db(os.path.join(d, "prot"), [(k, p.seqs[k] + b"\n") for k in sorted(p.seqs)], 0)
    lcs.write_db(os.path.join(d, "pref_prot7"), p.pref(), 7)
    lcs.write_db(os.path.join(d, "nuclx"), [(k, n.seqs[k] + b"\n") for k in sorted(n.seqs)], 1)
    lcs.write_db(os.path.join(d, "pref_nuclx14"), n.pref(), 14)
    lcs.write_db(os.path.join(d, "pref_nuclx7"), n.pref(), 7)
    return {"prot": p, "nuclx": n}


def family_db():
    """a small protein DB for the linclust run: families of near copies (kept together by --min-seq-id 0.9), distant copies and fragments"""
    r = random.Random(5)
    seqs = []
    for _ in range(36):
        base = rnd_aa(r, r.randrange(150, 420))
        seqs.append(base)
        seqs.append(subst_aa(r, base, 0.02))
        seqs.append(subst_aa(r, base[r.randrange(0, 12):], 0.05))
        seqs.append(subst_aa(r, base, 0.2))
        seqs.append(subst_aa(r, base[:len(base) * 3 // 5], 0.01))
        # unrelated but for a block of 40 residues in place: a k-mer candidate of the base that only the diagonal filter can drop
        seqs.append(rnd_aa(r, 100) + base[100:140] + rnd_aa(r, len(base) - 140))
    r.shuffle(seqs)
    return [(3 * i + 1, s.encode() + b"\n") for i, s in enumerate(seqs)]


def write_family(root):
    lcs.write_db(os.path.join(root, "subst", "fam"), family_db(), 0)


def unpack_fixture(d):
    """tests/golden/subst.tar.gz (make_subst.sh: what the unmodified reference wrote) beside local.tar.gz under `d` -> runs =
    [(name, sequence DB, prefilter DB, flags, the threshold the reference took from its table or None)], paths from `d`"""
    import tarfile
    for name in ("subst", "local"):
        with tarfile.open(os.path.join(lcs.GOLDEN, name + ".tar.gz")) as t:
            t.extractall(d)
    runs = []
    for line in open(os.path.join(d, "subst", "RUNS")).read().splitlines():
        name, db, pref, flags, thr = line.split("\t")
        runs.append((name, db, pref, flags, None if thr == "-" else float(thr)))
    return runs


def expected(root, db, pref, flags, thr, db_residues=None):
    """the restatement on one combination -> ({key: entry bytes with the NUL}, records)"""
    seqs, dbtype = sc.read_seqdb(os.path.join(root, db))
    ent, pref_type = sc.read_db(os.path.join(root, pref))
    par = sc.parse_flags(flags)
    par["thr"] = thr
    out, recs = sc.rescore_subst(seqs, dbtype == 1, ent, pref_type, par, db_residues=db_residues)
    return {k: e + b"\0" for k, e in out}, recs
