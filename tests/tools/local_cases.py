"""Hand-made pairs at the edges of the mode 2 kernel (plass_amd/csrc/rescore_local.hip): one wavefront walks an overlap in steps of
64 lanes x 16 residues, so the cases sit at 1, 15, 16, 17, 1023, 1024 and 1025 columns, at the first and the last position, across a step
boundary, on ties of the maximum and of the running minimum, on both signs of the diagonal, on the +-65536 wraps, on the reverse strand and
on the thresholds of every gate.  Shared by tests/test_local_host.py (restatement against the CPU oracle) and tests/test_gpu_local.py."""
import os
import random

import local_check as lc

OTHER = {"A": "C", "C": "A", "G": "T", "T": "G"}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}

# (name, flags, --score-per-col-thr or None): the reference's flag names; the threshold is this project's own flag
RUNS = [
    ("default", "--rescore-mode 2 -e 0.001 --min-seq-id 0.0 -c 0 --cov-mode 0 --seq-id-mode 0 --min-aln-len 0 -a 0 --filter-hits 0", None),
    ("linclust", "--rescore-mode 2 -e 0.001 --min-seq-id 0.99 -c 0.9 --cov-mode 1 --seq-id-mode 0 --min-aln-len 90 -a 1 --filter-hits 0", None),
    ("lax", "--rescore-mode 2 -e 10 --min-seq-id 0.0 -c 0 --cov-mode 0 --seq-id-mode 1 --min-aln-len 0 -a 1 --filter-hits 0", None),
    ("long", "--rescore-mode 2 -e 0.001 --min-seq-id 0.5 -c 0.5 --cov-mode 0 --seq-id-mode 2 --min-aln-len 101 -a 0 --filter-hits 0", None),
    ("filter1", "--rescore-mode 2 -e 0.001 --min-seq-id 0.99 -c 0.9 --cov-mode 1 --seq-id-mode 0 --min-aln-len 90 -a 0 --filter-hits 1", 1.0),
    ("filter0", "--rescore-mode 2 -e 0.001 --min-seq-id 0.99 -c 0.9 --cov-mode 1 --seq-id-mode 0 --min-aln-len 90 -a 1 --filter-hits 1", 0.0),
]


def rnd(r, n):
    return "".join(r.choice("ACGT") for _ in range(n))


def mutate(s, positions):
    x = list(s)
    for p in positions:
        x[p] = OTHER[x[p].upper()]
    return "".join(x)


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


class Cases:
    def __init__(self):
        self.seqs, self.lines, self.label, self.next_key = {}, {}, {}, 3

    def add(self, label, s):
        k = self.next_key
        self.next_key += 1 + (k % 3)                    # keys with gaps
        self.seqs[k] = s.encode()
        self.label[label] = k
        self.lines.setdefault(k, [])
        return k

    def pair(self, label, q, t, diag=0, score=17):
        """query q lists target t on `diag` (score < 0: the reverse strand in a prefilter DB with strands)"""
        kq, kt = self.add(label + ".q", q), self.add(label + ".t", t)
        self.lines[kq].append((kt, score, diag))
        return kq, kt

    def pref(self):
        """[(key, entry bytes)] in key order; the diagonal as the signed short QueryMatcher writes"""
        out = []
        for k in sorted(self.seqs):
            out.append((k, b"".join(b"%d\t%d\t%d\n" % (t, s, ((d & 0xFFFF) ^ 0x8000) - 0x8000) for t, s, d in self.lines[k])))
        return out


def nucl_cases():
    """-> Cases (the E-value depends on the DB's residue count, which is only known when the DB is complete: the E-value gate is
    met by a ladder of raw scores 20, 22 .. 70 on one query length, between two of which -e 0.001 falls)"""
    r = random.Random(20240611)
    c = Cases()
    # overlap lengths around the lane's 16 residues and the step's 1024; a few substitutions inside, the ends equal
    for n in (1, 15, 16, 17, 1023, 1024, 1025, 2049):
        q = rnd(r, n)
        c.pair("len%d" % n, q, mutate(q, [p for p in (n // 3, n // 2) if 0 < p < n - 1]))
    # the best segment at position 0, at the last position, across the boundary between two steps (1024) and between two lanes (16)
    q = rnd(r, 1500)
    c.pair("first", q, q[:40] + mutate(q[40:], range(1460)))
    c.pair("last", q, mutate(q[:1460], range(1460)) + q[1460:])
    c.pair("step", q, mutate(q[:1000], range(1000)) + q[1000:1050] + mutate(q[1050:], range(450)))
    c.pair("lane", q, mutate(q[:10], range(10)) + q[10:22] + mutate(q[22:], range(1478)))
    # two equal maxima: the earlier end wins (in neighbouring lanes, in distant lanes, in two steps)
    for label, gap in (("tie_lane", 7), ("tie_wave", 100), ("tie_step", 1100)):
        q = rnd(r, gap + 40)
        t = mutate(q, list(range(0, 5)) + list(range(15, 15 + gap)) + list(range(25 + gap, 40 + gap)))
        c.pair(label, q, t)
    # prefixes that come back to zero: three matches, two substitutions (+6 -6), repeated — the LATER minimum position is the start
    for label, reps in (("zeros_lane", 2), ("zeros_wave", 30), ("zeros_step", 300)):
        q = rnd(r, 5 * reps + 30)
        t = mutate(q, [5 * i + j for i in range(reps) for j in (3, 4)] + list(range(5 * reps + 20, 5 * reps + 30)))
        c.pair(label, q, t)
    # the running minimum is reached again far below zero: X X M M M X X (the sum returns to the minimum only with score <= 0 rules)
    q = rnd(r, 64)
    c.pair("min_again", q, mutate(q, [0, 1, 5, 6, 40, 41, 42, 43]))
    # an all-negative diagonal: nothing scores, start = end = -1; as identity pair (kept whatever it scores) and as ordinary pair
    k = c.add("allneg.self", "AC" * 40)
    c.lines[k].append((k, 5, 1))
    c.pair("allneg.pair", "A" * 33, "C" * 47)
    # identity pairs on their own diagonal, also listed twice, also with a diagonal that misses the sequence altogether
    k = c.add("self", rnd(r, 300))
    c.lines[k] += [(k, 0, 0), (k, 9, 0), (k, 9, 301)]
    # both signs of the diagonal: the target sticks out on the left (negative) or the query does (positive)
    q = rnd(r, 200)
    c.pair("neg", q, rnd(r, 77) + mutate(q, [50]) + rnd(r, 10), diag=-77)
    c.pair("pos", rnd(r, 31) + q + rnd(r, 5), mutate(q, [120, 121]), diag=31)
    c.pair("miss", q[:50], q[:50], diag=50)              # the diagonal touches neither: no wrap scores
    # lower-case letters and N: the matrix decides, identities fold the case
    q = rnd(r, 120)
    t = q[:30].lower() + q[30:60] + "NNNN" + q[64:]
    c.pair("case", q[:80] + "N" * 6 + q[86:], t)
    # the reverse strand: the target is the reverse complement of the query's middle, positions come back flipped
    q = rnd(r, 400)
    c.pair("rev", q, revcomp(mutate(q[100:350], [77, 180])), diag=50, score=-17)
    c.pair("rev_lower", q.lower(), revcomp(q)[:390], diag=0, score=-3)
    c.pair("rev_long", rnd(r, 900) + q + rnd(r, 1000), rnd(r, 20) + revcomp(q) + rnd(r, 700), diag=980, score=-40)
    # entries beyond 65536 residues: diagonal 100 is also -65436 and 65636.  The same 50 columns are planted on -65436 and on 100:
    # the two wraps tie and the first one tried, the negative one, wins; a third, better segment on 65636 in the second pair
    q = rnd(r, 70000)
    t = list(rnd(r, 70000))
    t[65436 + 200:65436 + 250] = q[200:250]
    t[300:350] = q[400:450]
    for p in (65436 + 197, 65436 + 198, 65436 + 199, 65436 + 250, 65436 + 251, 65436 + 252):
        t[p] = OTHER[q[p - 65436]]
    for p in (297, 298, 299, 350, 351, 352):
        t[p] = OTHER[q[p + 100]]
    c.pair("wrap_tie", q, "".join(t), diag=100)
    t[1000:1080] = q[65636 + 1000:65636 + 1080]
    c.pair("wrap_third", q, "".join(t), diag=100)
    # the gates on their thresholds (run "linclust": --min-seq-id 0.99, -c 0.9 --cov-mode 1, --min-aln-len 90)
    q = rnd(r, 100)
    c.pair("seqid_eq", q, mutate(q, [60]))                              # 99 of 100 identical: 0.99 >= 0.99 - epsilon
    c.pair("seqid_below", q, mutate(q, [30, 60]))                       # 98 of 100
    c.pair("cov_eq", q[:90], q[:90] + OTHER[q[90]] * 10)        # target coverage 90 / 100 = 0.9
    c.pair("cov_below", q[:90], q[:89] + OTHER[q[89]] * 11)     # 89 / 100
    c.pair("alnlen_eq", q[:90], q[:90])                                 # alnLen 90 == --min-aln-len
    c.pair("alnlen_below", q[:89], q[:89])
    c.pair("cancover_eq", q[:90], q)                                    # canBeCovered: 90 / 100 >= 0.9, before any scoring
    c.pair("cancover_below", q[:89], q)
    # the score per column on the threshold 1.0 of run "filter1": 50 matches in an overlap of 100 columns, then 49 of 98 + a substitution
    q = rnd(r, 100)
    c.pair("percol_eq", q, q[:50] + mutate(q[50:], range(50)))
    c.pair("percol_below", q, q[:49] + mutate(q[49:], range(51)))
    # a ladder of raw scores 20, 22 .. 70 against one query length: -e 0.001 falls between two of them
    q = rnd(r, 60)
    for m in range(10, 36):
        c.pair("evalue%d" % m, q, q[:m] + mutate(q[m:], range(60 - m)))
    return c


def prot_cases():
    r = random.Random(7)
    aa = "ACDEFGHIKLMNPQRSTVWY"
    c = Cases()
    for n in (9, 40, 300, 1100):
        q = "".join(r.choice(aa) for _ in range(n))
        x = list(q)
        for p in r.sample(range(n), max(1, n // 12)):
            x[p] = r.choice(aa)
        c.pair("prot%d" % n, q, "".join(x))
        c.pair("prot_shift%d" % n, q, "".join(r.choice(aa) for _ in range(5)) + "".join(x), diag=-5)
    k = c.add("prot_self", "".join(r.choice(aa) for _ in range(50)))
    c.lines[k].append((k, 0, 0))
    return c


def write_db(path, entries, dbtype):
    """entries: [(key, bytes without the NUL)] in key order"""
    off = 0
    with open(path, "wb") as fd, open(path + ".index", "wb") as fi:
        for k, e in entries:
            fd.write(e + b"\0")
            fi.write(b"%d\t%d\t%d\n" % (k, off, len(e) + 1))
            off += len(e) + 1
    open(path + ".dbtype", "wb").write(int(dbtype).to_bytes(4, "little"))


def write_all(root):
    """the DBs of the hand-made cases under `root`: nucl, prot (sequence DBs), pref_nucl14, pref_nucl7, pref_prot7 -> {name: Cases}"""
    os.makedirs(root, exist_ok=True)
    n, p = nucl_cases(), prot_cases()
    write_db(os.path.join(root, "nucl"), [(k, n.seqs[k] + b"\n") for k in sorted(n.seqs)], 1)
    write_db(os.path.join(root, "prot"), [(k, p.seqs[k] + b"\n") for k in sorted(p.seqs)], 0)
    write_db(os.path.join(root, "pref_nucl14"), n.pref(), 14)
    write_db(os.path.join(root, "pref_nucl7"), n.pref(), 7)          # the same lines without strands: a negative score is a score
    write_db(os.path.join(root, "pref_prot7"), p.pref(), 7)
    return {"nucl": n, "prot": p}


COMBOS = [("nucl", "pref_nucl14"), ("nucl", "pref_nucl7"), ("prot", "pref_prot7")]
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")


def unpack_fixture(d):
    """tests/golden/local.tar.gz (make_local.sh: what the unmodified reference wrote on the DBs of write_all) with the two tarballs its
    mergeclusters runs take their inputs from, side by side under `d` -> (runs, merges): runs = [(name, sequence DB, prefilter DB, flags,
    the threshold the reference took from its table or None)], merges = [(name, sequence DB, first clustering, second clustering)], paths
    from `d`"""
    import tarfile
    for name in ("local", "hamming", "clust"):
        with tarfile.open(os.path.join(GOLDEN, name + ".tar.gz")) as t:
            t.extractall(d)
    runs = []
    for line in open(os.path.join(d, "local", "RUNS")).read().splitlines():
        name, db, pref, flags, thr = line.split("\t")
        runs.append((name, os.path.join("local", db), os.path.join("local", pref), flags, None if thr == "-" else float(thr)))
    merges = [tuple(line.split("\t")[:4]) for line in open(os.path.join(d, "local", "MERGES")).read().splitlines()]
    return runs, merges


def expected(root, db, pref, flags, thr):
    """the restatement on one combination -> ({key: entry bytes with the NUL}, records, counts)"""
    seqs, dbtype = lc.read_seqdb(os.path.join(root, db))
    ent, pref_type = lc.read_db(os.path.join(root, pref))
    par = lc.parse_flags(flags)
    par["thr"] = thr
    counts = {}
    out, recs = lc.rescore_local(seqs, dbtype == 1, ent, pref_type, par, counts=counts)
    return {k: e + b"\0" for k, e in out}, recs, counts
