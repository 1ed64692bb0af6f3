#!/usr/bin/env python3
"""GENERATION-TIME ONLY: the inputs of tests/golden/hamming.tar.gz (make_hamming.sh runs the reference on them).

    make_hamming_inputs.py <outdir>

writes small sequence DBs (nucl: dbtype 1, prot: dbtype 0) and HAND-WRITTEN prefilter DBs over them (pref_nucl7, pref_prot7: dbtype 7;
pref_nucl14: dbtype 14, lines with a negative score are reverse-strand hits), so that every diagonal the cases need is actually asked
for: kmermatcher would not produce them on demand.  Every key of a sequence DB has an entry in its prefilter DBs (possibly empty), as
kmermatcher leaves it.  Everything is seeded; NAMES lists which key is which sequence."""
import os
import random
import struct
import sys

LENS = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257)
R = random.Random(20261018)


def rnd(n, alphabet="ACGT"):
    return "".join(R.choice(alphabet) for _ in range(n))


def rot(x, s):
    """rot(x, s)[j] = x[(j + s) % len(x)]"""
    s %= max(len(x), 1)
    return x[s:] + x[:s]


def mutate(x, n, alphabet="ACGT"):
    x = list(x)
    for p in R.sample(range(len(x)), n):
        x[p] = alphabet[(alphabet.index(x[p].upper()) + 1 + R.randrange(len(alphabet) - 1)) % len(alphabet)] if x[p].upper() in alphabet else alphabet[0]
    return "".join(x)


def table_revcomp(x):
    """the reverse strand as the reference builds it: num2aa[reverseResidue(aa2num[c])], always upper case, X for everything unknown"""
    comp = {}
    for c in "A":
        comp[c] = "T"
    for c in "CMYH":
        comp[c] = "G"
    for c in "TUW":
        comp[c] = "A"
    for c in "GKBDVRS":
        comp[c] = "C"
    return "".join(comp.get(c.upper(), "X") for c in reversed(x))


def bio_revcomp(x):
    m = str.maketrans("ACGTacgtNn", "TGCAtgcaNn")
    return x.translate(m)[::-1]


class DB:
    def __init__(self):
        self.names, self.seqs, self.lines = [], [], {}

    def add(self, name, seq):
        assert name not in self.names
        self.names.append(name); self.seqs.append(seq); self.lines[name] = []
        return name

    def hit(self, query, target, score, diag):
        self.lines[query].append((target, score, diag % 65536))

    def key(self, name):
        return self.names.index(name)


def write_db(path, entries, dbtype):
    off = 0
    with open(path, "wb") as fd, open(path + ".index", "w") as fi:
        for key, data in entries:
            e = data + b"\0"
            fd.write(e); fi.write("%d\t%d\t%d\n" % (key, off, len(e))); off += len(e)
    with open(path + ".dbtype", "wb") as ft:
        ft.write(struct.pack("<i", dbtype))


def write_pref(path, db, dbtype, keep):
    ent = []
    for k, name in enumerate(db.names):
        txt = ""
        for (t, sc, dg) in db.lines[name]:
            if keep(sc):
                txt += "%d\t%d\t%d\n" % (db.key(t), sc, dg - 65536 if dg >= 32768 else dg)      # the diagonal is a signed short in the file
        ent.append((k, txt.encode()))
    write_db(path, ent, dbtype)


def nucl_db():
    d = DB()
    for n in LENS:
        s = n // 3
        a = d.add("a%d" % n, rnd(n))
        b = d.add("b%d" % n, rot(d.seqs[d.key(a)], s))                     # the same length: an exact rotation, the circular-contig case
        base = d.seqs[d.key(a)] + rnd(5 if n < 64 else 40)
        m, s2 = len(base), len(base) // 2
        cseq = rot(base, s2)
        if n >= 63:
            cseq = mutate(cseq, 1)
            p = (m - s2 + n // 2) % m                                      # a lower-case letter inside the match: the compare is case-sensitive
            cseq = cseq[:p] + cseq[p].lower() + cseq[p + 1:]
        c = d.add("c%d" % n, cseq)                                         # a longer query that holds the target across its end
        d.hit(a, a, 0, 0)
        d.hit(b, b, 0, 0)
        seen = []
        for dg in ((n - s) % n, 0, 1, n - 1, 65536 - 1, 65536 - s):
            if dg % 65536 not in seen:
                seen.append(dg % 65536); d.hit(b, a, 0, dg)
        d.hit(c, c, 0, 0)
        for dg in ((m - s2) % m, 0, 1, m - 1, 65535):
            d.hit(c, a, 0, dg)
        d.hit(c, b, 0, 0); d.hit(c, b, 0, (m - s2 + (n - s)) % m)
        if n in (15, 16, 17, 64, 65, 257):                                 # reverse-strand hits (pref_nucl14 only)
            rc = d.add("rc%d" % n, table_revcomp(d.seqs[d.key(a)]))
            for dg in ((m - n + s2) % m, 0, 65536 - 2):
                d.hit(c, rc, -1, dg)
            d.hit(rc, rc, 0, 0)
    d.hit("a16", "a17", 0, 0)                                              # a target one residue longer than the query: skipped by the wrapped mode
    d.lines["a17"] = [("a17", 0, 3)]                                       # an identity pair on a diagonal that fails every threshold
    d.add("empty", rnd(40))                                                # a query with an empty entry
    # lower case, N and IUPAC codes on the reverse strand
    rq = d.add("rq", rnd(97, "ACGTacgtNnRYKMSWBDHVUu"))
    rt = d.add("rt_table", table_revcomp(rot(d.seqs[d.key(rq)], 11)))
    rb = d.add("rt_bio", bio_revcomp(d.seqs[d.key(rq)]))
    d.hit(rq, rq, 0, 0)
    d.hit(rq, rt, -50, 97 - 11); d.hit(rq, rt, -50, 0); d.hit(rq, rb, -50, 0); d.hit(rq, rt, 50, 97 - 11); d.hit(rq, rb, 7, 0)
    d.hit(rt, rt, 0, 0); d.hit(rb, rb, 0, 0)
    # long contigs: the true offset on the second and third alias of the stored diagonal; both derived from one seeded sequence
    S = rnd(140000)
    P = rnd(300)
    q70 = list(mutate(rot(S[:70000], 12345), 40))
    for i in range(300):                                                   # the same 300 residues at two aliases of diagonal 65300: 65300 (second loop) and
        q70[(65300 + i) % 70000] = P[i]                                    # 70000 - 65536 + 65300 = 69764 (first loop, across the end): a tie, the first loop's alias wins
        q70[(69764 + i) % 70000] = P[i]
    q70 = "".join(q70)
    d.add("q140", S); d.add("q70", q70)
    d.add("t140", mutate(rot(S, 131072 + 500), 1400))                      # third alias of diagonal 500
    d.add("t140s", rot(S, 131072 + 700)[:1000])                            # third alias of diagonal 700, a short target
    d.add("t70", mutate(rot(q70, 65536 + 1000), 1400))                     # second alias of diagonal 1000
    d.add("t70rc", table_revcomp(mutate(rot(q70, 70000 - 66536), 700)))    # reverse strand: second alias of diagonal 1000
    d.add("ttie", P)
    d.hit("q140", "q140", 0, 0); d.hit("q140", "t140", 0, 500); d.hit("q140", "t140s", 0, 700); d.hit("q140", "t70", 0, 500)
    d.hit("q70", "q70", 0, 0); d.hit("q70", "t70", 0, 1000); d.hit("q70", "ttie", 0, 65300); d.hit("q70", "t70rc", -1, 1000); d.hit("q70", "t140", 0, 500)
    for t in ("t140", "t140s", "t70", "t70rc", "ttie"):
        d.hit(t, t, 0, 0)
    return d


def prot_db():
    aa = "ACDEFGHIKLMNPQRSTVWY"
    d = DB()
    for n in LENS:
        a = d.add("a%d" % n, rnd(n, aa))
        aseq = d.seqs[d.key(a)]
        bseq = mutate(aseq, n // 10, aa)
        if n >= 15:
            bseq = bseq[:7] + bseq[7].lower() + bseq[8:]
        b = d.add("b%d" % n, bseq)                                         # the same length, some residues changed, one in lower case
        k = 3 if n < 64 else 31
        c = d.add("c%d" % n, rnd(k, aa) + mutate(aseq, n // 20, aa) + rnd(9, aa))   # a longer query that holds the target at offset k
        d.hit(a, a, 0, 0); d.hit(a, c, 0, 65536 - k)
        d.hit(b, b, 0, 0); d.hit(b, a, 0, 0); d.hit(b, a, 0, 1); d.hit(b, a, 0, 65536 - 1)
        d.hit(c, c, 0, 0); d.hit(c, a, 0, k); d.hit(c, a, 0, 0); d.hit(c, a, 0, 65536 - 1); d.hit(c, b, 0, k)
    d.lines["a17"] = [("a17", 0, 3)]
    d.add("empty", rnd(40, aa))
    d.add("star", "*" + rnd(30, aa) + "*"); d.hit("star", "star", 0, 0); d.hit("star", "a15", 0, 2)
    return d


def main(out):
    os.makedirs(out, exist_ok=True)
    n, p = nucl_db(), prot_db()
    write_db(os.path.join(out, "nucl"), [(k, (s + "\n").encode()) for k, s in enumerate(n.seqs)], 1)
    write_db(os.path.join(out, "prot"), [(k, (s + "\n").encode()) for k, s in enumerate(p.seqs)], 0)
    write_pref(os.path.join(out, "pref_nucl7"), n, 7, lambda sc: sc >= 0)
    write_pref(os.path.join(out, "pref_nucl14"), n, 14, lambda sc: True)
    write_pref(os.path.join(out, "pref_prot7"), p, 7, lambda sc: True)
    with open(os.path.join(out, "NAMES"), "w") as fd:
        for db, name in ((n, "nucl"), (p, "prot")):
            for k, s in enumerate(db.names):
                fd.write("%s\t%d\t%s\t%d\n" % (name, k, s, len(db.seqs[k])))


if __name__ == "__main__":
    main(sys.argv[1])
