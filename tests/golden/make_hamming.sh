#!/bin/bash
# GENERATION-TIME ONLY (build container): tests/golden/hamming.tar.gz — the reference's `rescorediagonal --rescore-mode 0` (the Hamming score,
# lib/mmseqs/src/alignment/rescorediagonal.cpp with DistanceCalculator.h:57-175,276-295) pinned on small sequence DBs and hand-written
# prefilter DBs, with and without --wrapped-scoring 1.  The inputs come from make_hamming_inputs.py; the UNMODIFIED reference runs with
# linclust's flag set (lib/mmseqs/data/workflow/linclust.sh:30 as `penguin guided_nuclassemble` passes it) and with a second, loose one that
# makes the other outcome of every filter occur.  The tarball keeps DATA only: the input DBs, NAMES, RUNS (one line per run: name, sequence
# DB, prefilter DB, the flags) and per run the three files the reference wrote.  Reference binary: an out-of-tree build of the reference
# (REF_BUILD, default /tmp/plass-build).
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd)
B=${REF_BUILD:-/tmp/plass-build}; PENGUIN=$B/src/penguin
LINCLUST="--sub-mat nucl:nucleotide.out,aa:blosum62.out --rescore-mode 0 --filter-hits 0 -e 0.001 -c 0.99 -a 0 --cov-mode 1 --min-seq-id 0.97 --min-aln-len 0 --seq-id-mode 0 --add-self-matches 0 --sort-results 0 --db-load-mode 0 --threads 1 --compressed 0 -v 1"
LOOSE="--rescore-mode 0 -e 0.001 -c 0 --cov-mode 1 --min-seq-id 0.5 --seq-id-mode 1 --min-aln-len 20 --threads 1 -v 1"
W=$(mktemp -d); OUT=$W/hamming; mkdir -p $OUT/ref
python3 $HERE/make_hamming_inputs.py $OUT
: > $OUT/RUNS
run() {     # <name> <seqDB> <prefDB> <flags…>
    local name=$1 db=$2 pref=$3; shift 3
    mkdir -p $OUT/ref/$name
    ( cd $OUT && $PENGUIN rescorediagonal $db $db $pref ref/$name/out "$@" > ref/$name.log 2>&1 ) || { cat $OUT/ref/$name.log; exit 1; }
    rm -f $OUT/ref/$name.log
    printf '%s\t%s\t%s\t%s\n' "$name" "$db" "$pref" "$*" >> $OUT/RUNS
}
for pref in pref_nucl7 pref_nucl14; do
    for w in 0 1; do
        run ${pref}_linclust_w$w nucl $pref $LINCLUST --wrapped-scoring $w
        run ${pref}_loose_w$w nucl $pref $LOOSE --wrapped-scoring $w
    done
done
run pref_prot7_linclust_w0 prot pref_prot7 $LINCLUST --wrapped-scoring 0
run pref_prot7_loose_w0 prot pref_prot7 $LOOSE --wrapped-scoring 0
tar -C $W -czf $HERE/hamming.tar.gz hamming
ls -l $HERE/hamming.tar.gz
rm -rf $W
