#!/usr/bin/env python3
"""GENERATION-TIME ONLY: the hand-made input of tests/golden/gencode.tar.gz (make_gencode.sh runs the reference on it).

    make_gencode_inputs.py <outdir>

writes the nucleotide read DB <outdir>/in (+ in_h, the .index and .dbtype files) and <outdir>/RUNLIST: one line per run of the reference — name,
module, input DB, output DB, flags — for every genetic code the reference accepts, with --use-all-table-starts 0 and 1, and for four ids it does not
accept.  What each group of reads is there for is said beside it.  Everything is seeded."""
import os
import random
import struct
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gencode_ref as G  # noqa: E402

# the flags of the single runs, chosen so that what a run keeps depends on the table (a fixture of every ORF of every frame, fifty times, would be
# megabytes).  ORF: the ORFs that begin with a start codon (--orf-start-mode 0 --contig-start-mode 1), of 2 to 30 codons, at most one codon with a gap
# letter; TRANSLATED: the ORFs that end with a stop codon (any to stop, --contig-end-mode 1), from one codon on, translated by extractorfs itself
ORF = "--min-length 2 --max-length 30 --max-gaps 1 --orf-start-mode 0 --contig-start-mode 1"
TRANSLATED = "--min-length 1 --max-length 30 --max-gaps 1 --orf-start-mode 1 --contig-end-mode 1 --translate 1"
# data/assemble.sh:41-77 with the parameter strings of src/workflow/Assembler.cpp:116-130
START = "--min-length 20 --max-length 45 --max-gaps 0 --contig-start-mode 1 --contig-end-mode 0 --orf-start-mode 0 --forward-frames 1,2,3 --reverse-frames 1,2,3"
LONG = "--min-length 45 --max-length 32734 --max-gaps 0 --contig-start-mode 2 --contig-end-mode 2 --orf-start-mode 0 --forward-frames 1,2,3 --reverse-frames 1,2,3"
WORKFLOWS = (("wf11", 11, 1), ("wf4", 4, 0))

CODONS = [a + b + c for a in "TCAG" for b in "TCAG" for c in "TCAG"]
STARTS_1_4_11 = sorted({CODONS[i] for t in (1, 4, 11) for i in range(64) if G.TABLES[t][1][i] == "M"})
OPEN = "GCTGAACCTGGT"                      # four codons that no table reads as a start or a stop


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def reads(rnd):
    out = []
    # all 64 codons in each of the three frames and on both strands (the order shuffled once; the reverse complements put them on the other strand)
    order = CODONS[:]
    rnd.shuffle(order)
    for half in (order[:32], order[32:], order[16:48]):
        body = "".join(half)
        for shift in ("", "G", "GC"):
            out += [shift + body, revcomp(shift + body)]
    # every start codon of tables 1, 4 and 11 at position 0 and directly behind a stop (TAA is a stop wherever the code has stops at all)
    for c in STARTS_1_4_11:
        out += [c + OPEN + "TAA" + OPEN, OPEN + "TAA" + c + OPEN + "TAG" + c, "G" + c + OPEN + "TAA" + c + OPEN, revcomp(OPEN + "TAA" + c + OPEN)]
    # stops of tables 2 (AGA / AGG), 22 (TCA), 23 (TTA), and the codons tables 27, 28 and 31 list as stops but translate (TGA, TAA, TAG), inside open frames
    for c in ("AGA", "AGG", "TCA", "TTA", "TGA", "TAA", "TAG"):
        out += ["ATG" + OPEN + c + OPEN + OPEN, "C" + OPEN + OPEN + c + "ATG" + OPEN, revcomp("ATG" + OPEN + c + OPEN)]
    # lower case, U / u, and each IUPAC ambiguity letter in each codon position (TAR, YAA, TRA ...: around the stops and ATG)
    out += ["atg" + OPEN.lower() + "taa" + OPEN, "AtG" + OPEN + "tAa" + "aTG" + OPEN.lower(), "AUG" + OPEN + "UAA" + "aug" + OPEN + "uga" + OPEN, "UUG" + OPEN.replace("T", "U") + "UAG"]
    for amb in "RYSWKMBDHVN":
        for pos in range(3):
            c = [base[:pos] + amb + base[pos + 1:] for base in ("TAA", "ATG", "TGA")]
            out.append("ATG" + OPEN + c[0] + OPEN + c[1] + OPEN + c[2] + "TAA" + c[0].lower() + c[1].lower())
    # N runs around --max-gaps 1 (one codon with N, two, a run across a codon border), X and an illegal letter
    out += ["ATG" + OPEN + "NNN" + OPEN + "TAA", "ATG" + OPEN + "NGC" + "GCN" + OPEN + "TAA", "ATG" + "GCN" + "NGC" + OPEN, "ATG" + OPEN + "GNN" + "NNC" + "TAA",
            "ATG" + OPEN + "GCX" + OPEN, "ATG" + OPEN + "G-C" + OPEN + "TAA", "ATG" + OPEN + "G.C" + "G*C" + OPEN]
    # read lengths 0 .. 9, and 3n - 1, 3n, 3n + 1 around the 8-byte words a reader may load (15 .. 17, 23 .. 25)
    long_open = "ATG" + OPEN * 3
    out += [long_open[:n] for n in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 23, 24, 25)]
    out += [revcomp(long_open[:n]) for n in (3, 4, 5, 7, 8, 15, 16, 17, 23, 24, 25)]
    # ORFs exactly at --min-length and --max-length of the three flag sets (1, 2, 20, 30, 45 codons) and one codon off
    for n in (1, 2, 3, 4, 19, 20, 21, 29, 30, 31, 44, 45, 46):
        body = "".join(rnd.choice(["GCT", "GAA", "CCT", "GGT", "AAC", "CAG"]) for _ in range(n - 1))
        out += ["TAA" + "ATG" + body + "TAA" + "GC", "ATG" + body]
    # the rest: random reads, some with lower-case stretches, a U or an ambiguity letter
    while len(out) < 220:
        n = rnd.choice([12, 20, 31, 47, 64, 200])
        s = "".join(rnd.choice("ACGT") for _ in range(n))
        r = rnd.random()
        if r < 0.15:
            a = rnd.randrange(n)
            s = s[:a] + s[a:a + 9].lower() + s[a + 9:]
        elif r < 0.25:
            a = rnd.randrange(n)
            s = s[:a] + rnd.choice("UuRYKMSWBDHVNn") + s[a + 1:]
        out.append(s)
    assert all(len(s) <= 200 for s in out)
    return out


def write_db(path, entries, dbtype):
    data, index = G.db_files(entries)
    open(path, "wb").write(data)
    open(path + ".index", "wb").write(index)
    open(path + ".dbtype", "wb").write(struct.pack("<I", dbtype))


def main(out):
    os.makedirs(out, exist_ok=True)
    rnd = random.Random(20261020)
    seqs = reads(rnd)
    write_db(os.path.join(out, "in"), [(i, s.encode() + b"\n") for i, s in enumerate(seqs)], 1)
    write_db(os.path.join(out, "in_h"), [(i, b"read%d\n" % i) for i in range(len(seqs))], 12)
    with open(os.path.join(out, "RUNLIST"), "w") as runs:
        def run(name, module, src, dst, flags):
            runs.write("\t".join((name, module, src, dst, flags)) + "\n")
        for t in G.VALID + list(G.INVALID):
            for s in (0, 1):
                tag, tt = "t%d_s%d" % (t, s), "--translation-table %d" % t
                run(tag + "_orfs", "extractorfs", "in", tag + "_orfs", "%s %s --use-all-table-starts %d" % (ORF, tt, s))
                run(tag + "_tr", "extractorfs", "in", tag + "_tr", "%s %s --use-all-table-starts %d" % (TRANSLATED, tt, s))
            # translatenucs has no start flag: once per table, on the ORFs of its --use-all-table-starts 1 run (of table 1 for the ids that are refused)
            src = "t%d_s1_orfs" % (t if t in G.TABLES else 1)
            for stop in (0, 1):
                run("t%d_aa%d" % (t, stop), "translatenucs", src, "t%d_aa%d" % (t, stop), "--translation-table %d --add-orf-stop %d" % (t, stop))
        for name, t, s in WORKFLOWS:
            tt = "--translation-table %d" % t
            ex = "%s --translate 0 --use-all-table-starts %d --id-offset 0 --create-lookup 0" % (tt, s)
            run(name + "_nucl_6f_start", "extractorfs", "in", name + "_nucl_6f_start", "%s %s" % (START, ex))
            run(name + "_aa_6f_start", "translatenucs", name + "_nucl_6f_start", name + "_aa_6f_start", tt + " --add-orf-stop 1")
            run(name + "_nucl_6f_long", "extractorfs", "in", name + "_nucl_6f_long", "%s %s" % (LONG, ex))
            run(name + "_aa_6f_long", "translatenucs", name + "_nucl_6f_long", name + "_aa_6f_long", tt + " --add-orf-stop 1")
            run(name + "_aa_6f_start_long", "concatdbs", name + "_aa_6f_long " + name + "_aa_6f_start", name + "_aa_6f_start_long", "")
            run(name + "_aa_6f_start_long_h", "concatdbs", name + "_nucl_6f_long_h " + name + "_nucl_6f_start_h", name + "_aa_6f_start_long_h", "")


if __name__ == "__main__":
    main(sys.argv[1])
