#!/bin/bash
# GENERATION-TIME ONLY (build container): tests/golden/fasta_tail_*.tar.gz — the reference's workflow tail (data/assemble.sh:159-201,
# data/nuclassemble.sh:138-207: the `_only_assembled` selection, createsubdb, createhdb, convert2fasta) pinned on five cases.  The UNMODIFIED
# workflows run with --threads 1 (one data file in key order: the canonical layout the selection is defined on) and --remove-tmp-files 0;
# from each run the tarball keeps DATA only: the RESULT DB the tail selected from, SOURCE's index, the cycle index (PREV_CYCLE_ALL) where one
# exists, the FASTA the workflow wrote, and a MANIFEST (commands, thread count, awk version).  Reference binaries: an out-of-tree build of
# the reference (REF_BUILD, default /tmp/plass-build).
#
#   case1  plass assemble --filter-proteins 0
#   case2  plass assemble --filter-proteins 0 --keep-target 0            (keys are not 0..n-1: the rank-versus-key quirk of assemble.sh:176)
#   case3  penguin nuclassemble                                          (defaults: --contig-output-mode 1 --min-contig-len 1000; the
#          example yields no contig of 1000 nt, so this case reads the case-5 read set)
#   case4  penguin nuclassemble --contig-output-mode 0 --min-contig-len 200
#   case5  penguin nuclassemble on FASTQ pairs of the make_circular_chain.py model (mates split 75 / 75, they do not overlap)
#
# Cases 1-4 read the bundled example pairs (tests/golden/example_reads).  The script checks, on the reference's own output, that the
# fixture cannot pass vacuously (tests/tools/contigcheck.py restates the selection): every case selects something, case 1 or 2 has a key
# in S2 \ S1, case 5 has a "cycle:1" header, case 4 has an entry mode 1 would have dropped.
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd); REPO=$(cd "$HERE/../.." && pwd)
B=${REF_BUILD:-/tmp/plass-build}; PLASS=$B/src/plass; PENGUIN=$B/src/penguin
R1=$HERE/example_reads/reads_1.fastq.gz; R2=$HERE/example_reads/reads_2.fastq.gz
W=$(mktemp -d); OUT=$W/fasta_tail; mkdir -p $OUT; echo "work dir $W"
Q="--threads 1 --remove-tmp-files 0 -v 1"

# case 5's reads: the model of make_circular_chain.py (circular replicons whose reads wrap around the origin, a linear genome, 0.2 %
# substitutions, both strands) scaled down to four replicons so that the fixture stays small; every 150-nt read becomes a pair of
# 75-nt mates (mate 2 reverse-complemented) that do not overlap, so mergereads keeps both
python3 - "$W" <<'EOF'
import gzip, sys
import numpy as np
W, READ = sys.argv[1], 150
rng = np.random.default_rng(20261)
B = np.frombuffer(b"ACGT", dtype=np.uint8)
comp = np.zeros(256, dtype=np.uint8); comp[B] = B[::-1]
out = []
for L, circular, cov in [(int(rng.integers(2500, 4000)), True, 30.0) for _ in range(4)] + [(8000, False, 10.0)]:
    g = B[rng.integers(0, 4, L)]
    n = int(L * cov / READ)
    src = np.concatenate([g, g[:READ]]) if circular else g
    starts = rng.integers(0, L if circular else L - READ + 1, n)
    r = src[starts[:, None] + np.arange(READ)[None, :]].copy()
    err = rng.random(r.shape) < 0.002
    r[err] = B[(np.searchsorted(B, r[err]) + rng.integers(1, 4, int(err.sum()))) % 4]
    rev = rng.random(n) < 0.5
    r[rev] = comp[r[rev][:, ::-1]]
    out.append(r)
r = np.concatenate(out); r = r[rng.permutation(len(r))]
with gzip.GzipFile(W + "/circ_1.fastq.gz", "wb", mtime=0) as f1, gzip.GzipFile(W + "/circ_2.fastq.gz", "wb", mtime=0) as f2:
    for i, x in enumerate(r):
        a, b = x[:75].tobytes(), comp[x[75:][::-1]].tobytes()
        f1.write(b"@c%d/1\n%s\n+\n%s\n" % (i, a, b"I" * len(a)))
        f2.write(b"@c%d/2\n%s\n+\n%s\n" % (i, b, b"I" * len(b)))
EOF

run() {   # run <case> <tool> <module> <r1> <r2> [flags...]
    local c=$1 tool=$2 mod=$3 a=$4 b=$5; shift 5
    mkdir -p $W/$c
    echo "$(basename $tool) $mod <r1> <r2> $c.fasta tmp $Q $*" >> $OUT/MANIFEST
    $tool $mod $a $b $W/$c/out.fasta $W/$c/tmp $Q "$@" > $W/$c/log 2>&1
    local T=$W/$c/tmp/latest
    mkdir -p $OUT/$c
    cp $W/$c/out.fasta $OUT/$c/ref.fasta
    if [ "$tool" = "$PLASS" ]; then
        local last=$(ls $T | sed -n 's/^assembly_\([0-9]*\)$/\1/p' | sort -n | tail -n 1)
        local res=$T/assembly_$last; echo "protein" > $OUT/$c/mode
        cp $T/aa_6f_start_long.index $OUT/$c/source.index
    else
        local last=$(ls $T | sed -n 's/^assembly_\([0-9]*\)$/\1/p' | sort -n | tail -n 1)
        local res=$T/assembly_$last; echo "nucleotide" > $OUT/$c/mode
        [ -f $T/assembly_merged ] && res=$T/assembly_merged
        local cyc=$(ls $T | sed -n 's/^assembly_\([0-9]*\)_cycle_all\.index$/\1/p' | sort -n | tail -n 1)
        [ -n "$cyc" ] && cp $T/assembly_${cyc}_cycle_all.index $OUT/$c/cycle.index
        cp $T/nucl_reads.index $OUT/$c/source.index
    fi
    cp $res $OUT/$c/result; cp $res.index $OUT/$c/result.index; cp $res.dbtype $OUT/$c/result.dbtype
    echo "$*" > $OUT/$c/flags
}
echo "# reference workflows, --threads 1; $(awk -W version 2>&1 | head -n 1 || true)" > $OUT/MANIFEST
run case1 $PLASS assemble $R1 $R2 --filter-proteins 0
run case2 $PLASS assemble $R1 $R2 --filter-proteins 0 --keep-target 0
# (the bundled example yields no contig of 1000 nt: case 3 runs on the case-5 read set)
run case3 $PENGUIN nuclassemble $W/circ_1.fastq.gz $W/circ_2.fastq.gz
run case4 $PENGUIN nuclassemble $R1 $R2 --contig-output-mode 0 --min-contig-len 200
run case5 $PENGUIN nuclassemble $W/circ_1.fastq.gz $W/circ_2.fastq.gz
( cd $OUT && sha256sum */ref.fasta >> MANIFEST )
mkdir -p $OUT/reads; cp $W/circ_1.fastq.gz $W/circ_2.fastq.gz $OUT/reads/
# the non-vacuity conditions, asserted on the reference's own output with the numpy restatement
( cd "$REPO" && python3 tests/tools/contigcheck.py --assert-fixture $OUT )
# a FASTA over 1 MB is kept as "<sha256> <entries> <bytes>" (ref.fasta.sha256); one tarball per case (each under the 1 MiB limit), the
# case-5 read pairs and the MANIFEST in one of their own
for c in case1 case2 case3 case4 case5; do
    F=$OUT/$c/ref.fasta
    if [ $(stat -c %s $F) -gt 1000000 ]; then
        echo "$(sha256sum < $F | cut -c1-64) $(grep -c '^>' $F) $(stat -c %s $F)" > $F.sha256; rm $F
    fi
    tar -C $W -czf $HERE/fasta_tail_$c.tar.gz fasta_tail/$c
done
tar -C $W -czf $HERE/fasta_tail_reads.tar.gz fasta_tail/reads fasta_tail/MANIFEST
( cd "$REPO" && python3 tests/tools/contigcheck.py --assert-fixture $OUT )
ls -l $HERE/fasta_tail_*.tar.gz
rm -rf $W
