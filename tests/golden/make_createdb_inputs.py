#!/usr/bin/env python3
"""The inputs of tests/golden/createdb.tar.gz (make_createdb.sh runs the unmodified reference's createdb on them): small read files that
cover the split boundaries of the shuffle (1, 31, 32, 33, 64, 65 reads), a count that runs across two files, FASTQ and FASTA of the same
reads, FASTA wrapped at 60, a 40 kb entry, lower case / N / IUPAC, headers with and without comments and tabs, a last line without '\\n',
'\\r\\n' line ends, a .gz, a protein FASTA and three broken FASTQ files.  Deterministic.
    python3 make_createdb_inputs.py <dir>   ->  <dir>/<name>, and <dir>/CASES: one line per case "case<TAB>expect<TAB>file [file ...]"
    (expect: ok = the reference's DB is the yardstick; 95 = refused as outside the GPU path; 1 = a broken file, refused with its record)"""
import gzip
import os
import random
import sys

out = sys.argv[1]
os.makedirs(out, exist_ok=True)
rng = random.Random(20261017)
ALPHA = "ACGT" * 12 + "acgt" * 2 + "N" * 2 + "n" + "RYKMSW"
PURE = "ACGT" * 12 + "acgt" * 2 + "N" * 2 + "n"      # the first ten entries decide the database type (createdb.cpp:171-200): no IUPAC codes there


def seq(n, alpha=ALPHA):
    return "".join(rng.choice(alpha) for _ in range(n))


def header(i):
    k = i % 6
    name = "r%d" % i if k != 5 else "gi|%d|ref|NC_%d.1|" % (1000 + i, i)
    return name + ["", " 1:N:0:ACGT", "\tlen=%d tab" % i, "  two  blanks ", " x", ""][k]


def reads(n, lo=1, hi=300, first=0):
    return [(header(first + i), seq(rng.randint(lo, hi), PURE if i < 10 else ALPHA)) for i in range(n)]


def fastq(rs, eol="\n", last_eol=True):
    t = "".join("@%s%s%s%s+%s%s%s" % (h, eol, s, eol, eol, "".join(rng.choice("FF:,#I") for _ in s), eol) for h, s in rs)
    return t if last_eol else t[:-len(eol)]


def fasta(rs, wrap=0, eol="\n", last_eol=True):
    t = ""
    for h, s in rs:
        lines = [s[k:k + wrap] for k in range(0, len(s), wrap)] if wrap else [s]
        t += ">%s%s%s%s" % (h, eol, eol.join(lines), eol)
    return t if last_eol else t[:-len(eol)]


cases = []


def put(name, text, gz=False):
    data = text.encode("latin-1") if isinstance(text, str) else text
    if gz:
        with open(os.path.join(out, name), "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as f:
            f.write(data)
    else:
        with open(os.path.join(out, name), "wb") as f:
            f.write(data)
    return name


for n in (1, 31, 32, 33, 64, 65):
    cases.append(("n%d" % n, "ok", [put("n%d.fastq" % n, fastq(reads(n, 20, 60)))]))
a, b = reads(351), reads(352, first=351)
cases.append(("mixed_fq", "ok", [put("mixed_a.fastq", fastq(a)), put("mixed_b.fastq", fastq(b))]))
cases.append(("mixed_fa", "ok", [put("mixed_a.fasta", fasta(a)), put("mixed_b.fasta", fasta(b))]))
cases.append(("wrapped", "ok", [put("wrapped.fasta", fasta(a, wrap=60))]))
cases.append(("fq_then_fa", "ok", ["mixed_b.fastq", "wrapped.fasta"]))
cases.append(("long40k", "ok", [put("long40k.fasta", fasta([("contig_1 one line", seq(40000))]) + fasta([("contig_2", seq(40001))], wrap=80))]))
c = reads(70, 1, 120)
cases.append(("nonl_fq", "ok", [put("nonl.fastq", fastq(c, last_eol=False))]))
cases.append(("nonl_fa", "ok", [put("nonl.fasta", fasta(c, wrap=60, last_eol=False))]))
cases.append(("crlf_fq", "ok", [put("crlf.fastq", fastq(c, eol="\r\n"))]))
cases.append(("crlf_fa", "ok", [put("crlf.fasta", fasta(c, wrap=60, eol="\r\n"))]))
cases.append(("gz", "ok", [put("mixed_a.fastq.gz", fastq(a), gz=True)]))
AA = "ACDEFGHIKLMNPQRSTVWY"
cases.append(("protein", "95", [put("protein.fasta", "".join(">p%d\n%s\n" % (i, "".join(rng.choice(AA) for _ in range(80))) for i in range(20)))]))
d = reads(40, 30, 80)
good = fastq(d).split("\n")                      # 4 lines per record (+ a last empty string)
noplus = list(good); del noplus[4 * 17 + 2]      # record 18 loses its '+' line
cases.append(("noplus", "1:18", [put("noplus.fastq", "\n".join(noplus))]))
qlen = list(good); qlen[4 * 22 + 3] = qlen[4 * 22 + 3][:-1] + "FF"        # record 23: one quality byte too many
cases.append(("qlen", "1:23", [put("qlen.fastq", "\n".join(qlen))]))
q200 = list(good); q200[4 * 8 + 3] = q200[4 * 8 + 3][:3] + chr(200) + q200[4 * 8 + 3][4:]       # record 9: a quality byte 200
cases.append(("q200", "1:9", [put("q200.fastq", "\n".join(q200))]))
with open(os.path.join(out, "CASES"), "w") as f:
    for name, expect, files in cases:
        f.write("%s\t%s\t%s\n" % (name, expect, " ".join(files)))
