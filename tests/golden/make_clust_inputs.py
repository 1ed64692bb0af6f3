#!/usr/bin/env python3
"""GENERATION-TIME ONLY: the hand-written inputs of tests/golden/clust.tar.gz (make_clust.sh runs the reference on them).

    make_clust_inputs.py <outdir>

writes three small nucleotide sequence DBs and HAND-WRITTEN result DBs over them, so that every case the clustering can get wrong occurs:

  cases   keys with gaps, in a key order that is not the length order
          - the chain c -> b, b -> x, x -> y with strictly falling lengths: pass 1 leaves y with x, x with b, b with c; the correction pass
            promotes x (named by y) and b (named by x)
          - d -> e (twice: a duplicate line), e -> d (a target longer than its query), e -> m: m is left with e, e is with d and promoted;
            d is named by e and is its own representative already: the other outcome of the correction pass
          - lone: an empty entry, listed by nobody; selfonly: lists itself only; short: lists the longer d twice
          as cases7 (dbtype 7), cases14 (dbtype 14, some lines on the reverse strand) and cases5 (dbtype 5, alignment lines, one with a
          backtrace column)
  star    one query (the longest, not the first key) lists all others
  equal   all lengths equal: the ties fall to the position in key order

Everything is seeded; NAMES lists which key is which sequence."""
import os
import random
import struct
import sys

R = random.Random(20261019)


def rnd(n):
    return "".join(R.choice("ACGT") for _ in range(n))


def write_db(path, entries, dbtype):
    off = 0
    with open(path, "wb") as fd, open(path + ".index", "w") as fi:
        for key, data in entries:
            e = data + b"\0"
            fd.write(e); fi.write("%d\t%d\t%d\n" % (key, off, len(e))); off += len(e)
    with open(path + ".dbtype", "wb") as ft:
        ft.write(struct.pack("<i", dbtype))


class Graph:
    def __init__(self, name):
        self.name, self.seqs, self.edges = name, [], {}

    def add(self, label, key, length):
        self.seqs.append((key, label, length)); self.edges[label] = []

    def edge(self, q, *targets):
        self.edges[q] += targets

    def key(self, label):
        return next(k for k, l, _ in self.seqs if l == label)

    def write(self, out, names):
        seqs = sorted(self.seqs)
        write_db(os.path.join(out, self.name), [(k, (rnd(n) + "\n").encode()) for k, _, n in seqs], 1)
        for k, label, n in seqs:
            names.write("%s\t%d\t%s\t%d\n" % (self.name, k, label, n))

    def pref(self, out, suffix, dbtype, line):
        write_db(os.path.join(out, self.name + suffix), [(k, "".join(line(i, self.key(t), n) for i, t in enumerate(self.edges[label])).encode())
                                                        for k, label, n in sorted(self.seqs)], dbtype)


def aln_line(i, tkey, qlen):
    """an alignment line as Matcher::resultToBuffer writes it; every third one with a backtrace column"""
    s = "%d\t%d\t0.%03d\t1.000E-10\t0\t%d\t%d\t0\t%d\t%d" % (tkey, 50 + i, 970 + i, qlen - 1, qlen, qlen - 1, qlen)
    return s + ("\t%dM\n" % qlen if i % 3 == 2 else "\n")


def main(out):
    os.makedirs(out, exist_ok=True)
    g = Graph("cases")
    for label, key, n in (("c", 2, 400), ("y", 5, 100), ("x", 9, 200), ("b", 11, 300), ("d", 14, 350), ("e", 15, 120), ("lone", 23, 250),
                          ("selfonly", 30, 90), ("short", 31, 50), ("m", 44, 80)):
        g.add(label, key, n)
    g.edge("c", "c", "b"); g.edge("b", "b", "x"); g.edge("x", "x", "y"); g.edge("y", "y")
    g.edge("d", "d", "e", "e"); g.edge("e", "e", "d", "m"); g.edge("m", "m")
    g.edge("selfonly", "selfonly"); g.edge("short", "short", "d", "d")
    s = Graph("star")
    for i, n in enumerate((70, 95, 60, 300, 88, 61)):
        s.add("s%d" % i, 1 + i, n)
    for i in range(6):
        s.edge("s%d" % i, "s%d" % i)
    s.edge("s3", *["s%d" % i for i in (5, 0, 1, 2, 4)])
    q = Graph("equal")
    for i, key in enumerate((3, 8, 12, 20, 21)):
        q.add("q%d" % i, key, 60)
    q.edge("q0", "q0", "q1"); q.edge("q1", "q1", "q0"); q.edge("q3", "q3", "q2"); q.edge("q2", "q2"); q.edge("q4", "q3")
    with open(os.path.join(out, "NAMES"), "w") as names:
        for gr in (g, s, q):
            gr.write(out, names)
            gr.pref(out, "7", 7, lambda i, t, n: "%d\t%d\t%d\n" % (t, 97 + i, i))
    g.pref(out, "14", 14, lambda i, t, n: "%d\t%d\t%d\n" % (t, -(97 + i) if i % 2 else 97 + i, -i))
    g.pref(out, "5", 5, aln_line)


if __name__ == "__main__":
    main(sys.argv[1])
