#!/bin/bash
# GENERATION-TIME ONLY (build container): tests/golden/local.tar.gz — the reference's `rescorediagonal --rescore-mode 2` (the best-scoring ungapped
# local segment on the candidate's diagonal, lib/mmseqs/src/alignment/rescorediagonal.cpp:193-334 with DistanceCalculator.h:93-201), its
# `mergeclusters` (lib/mmseqs/src/util/mergeclusters.cpp) and one `linclust --alignment-mode 4` with its intermediate DBs, pinned on small DBs.
# The inputs are the hand-made pairs of make_local_inputs.py (tests/tools/local_cases.py) and, for mergeclusters, the DBs of clust.tar.gz and
# hamming.tar.gz (they are not copied: a test unpacks the tarballs side by side).  The UNMODIFIED reference runs every step.  The tarball keeps
# DATA only: the hand-written input DBs, NAMES, and
#   RUNS    one line per rescorediagonal run: name, sequence DB, prefilter DB, the flags, and the score-per-column threshold the reference
#           took for --filter-hits 1 ("-": --filter-hits 0).  The threshold is looked up at generation time in the reference's own data file
#           (REF_SRC/lib/mmseqs/data/resources/CovSeqidQscPercMinDiag*.lib) by the rule of parsePrecisionLib, rescorediagonal.cpp:20-43: the
#           first row of (cov, seqid) on the grid with precision >= 0.99, 0 where there is none ("No hit will be filtered").  The table is not copied.
#   MERGES  one line per mergeclusters run: name, sequence DB, first clustering, second clustering (made by the reference's `clust` on the
#           createsubdb of the first one's representatives with the named prefilter DB), the prefilter DB
#   LINCLUST the flags of the linclust run and, on a second line, the threshold its alignment step took; its DBs are under ref/linclust/
# and per run the files the reference wrote.  Reference binary: an out-of-tree cmake + ninja build of the reference (REF_BUILD, default
# /tmp/plass-build; configure with -DCMAKE_POLICY_VERSION_MINIMUM=3.5 where cmake refuses the project's minimum version); REF_SRC: its source tree.
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd)
B=${REF_BUILD:-/tmp/plass-build}; PENGUIN=$B/src/penguin
SRC=${REF_SRC:?set REF_SRC to the source tree of the reference}
W=$(mktemp -d); OUT=$W/local; mkdir -p $OUT/ref
tar -C $W -xzf $HERE/hamming.tar.gz
tar -C $W -xzf $HERE/clust.tar.gz
python3 $HERE/make_local_inputs.py $OUT
: > $OUT/RUNS; : > $OUT/MERGES
threshold() {   # <cov-mode> <min-seq-id> <-c>: parsePrecisionLib on the reference's data file
    local lib=$SRC/lib/mmseqs/data/resources/CovSeqidQscPercMinDiagTargetCov.lib
    [ "$1" = 0 ] && lib=$SRC/lib/mmseqs/data/resources/CovSeqidQscPercMinDiag.lib
    awk -v s="$2" -v c="$3" 'BEGIN { i = int((s + 0.0001) * 100); ts = (i - i % 5) / 100; tc = int((c + 0.0001) * 10) / 10; r = "0" }
        { dc = $1 - tc; ds = $2 - ts; if (dc < 0) dc = -dc; if (ds < 0) ds = -ds; if (dc < 1e-6 && ds < 1e-6 && $4 >= 0.99) { r = $3; exit } }
        END { print r }' "$lib"
}
run() {     # <name> <seqDB> <prefDB> <threshold or -> <flags…>
    local name=$1 db=$2 pref=$3 thr=$4; shift 4
    mkdir -p $OUT/ref/$name
    ( cd $OUT && $PENGUIN rescorediagonal $db $db $pref ref/$name/out "$@" --threads 1 -v 2 > ref/$name.log 2>&1 ) || { cat $OUT/ref/$name.log; exit 1; }
    # the reference says so itself where its table has no row
    if [ "$thr" = 0 ]; then grep -q "No hit will be filtered" $OUT/ref/$name.log; elif grep -q "No hit will be filtered" $OUT/ref/$name.log; then echo "$name: no row"; exit 1; fi
    rm -f $OUT/ref/$name.log
    printf '%s\t%s\t%s\t%s\t%s\n' "$name" "$db" "$pref" "$*" "$thr" >> $OUT/RUNS
}
BASE="--rescore-mode 2 -e 0.001"
for combo in nucl:pref_nucl14 nucl:pref_nucl7 prot:pref_prot7; do
    db=${combo%%:*}; pref=${combo##*:}
    run ${pref}_default $db $pref - $BASE --min-seq-id 0.0 -c 0 --cov-mode 0 --seq-id-mode 0 --min-aln-len 0 -a 0 --filter-hits 0
    run ${pref}_linclust $db $pref - $BASE --min-seq-id 0.99 -c 0.9 --cov-mode 1 --seq-id-mode 0 --min-aln-len 90 -a 1 --filter-hits 0
    run ${pref}_lax $db $pref - --rescore-mode 2 -e 10 --min-seq-id 0.0 -c 0 --cov-mode 0 --seq-id-mode 1 --min-aln-len 0 -a 1 --filter-hits 0
    run ${pref}_long $db $pref - $BASE --min-seq-id 0.5 -c 0.5 --cov-mode 0 --seq-id-mode 2 --min-aln-len 101 -a 0 --filter-hits 0
    run ${pref}_fh_target $db $pref $(threshold 1 0.99 0.9) $BASE --min-seq-id 0.99 -c 0.9 --cov-mode 1 --seq-id-mode 0 --min-aln-len 90 -a 0 --filter-hits 1
    run ${pref}_fh_bidir $db $pref $(threshold 0 0.9 0.8) $BASE --min-seq-id 0.9 -c 0.8 --cov-mode 0 --seq-id-mode 1 --min-aln-len 0 -a 1 --filter-hits 1
    run ${pref}_fh_norow $db $pref $(threshold 0 0.0 0.0) $BASE --min-seq-id 0.0 -c 0 --cov-mode 0 --seq-id-mode 0 --min-aln-len 200 -a 0 --filter-hits 1
done
merge() {   # <name> <seqDB> <first clustering> <prefDB of the representatives>: linclust.sh:39-101 behind pre_clust, with `clust` on the prefilter DB
    local name=$1 db=$2 first=$3 pref=$4 T=$W/tmp_$1
    mkdir -p $OUT/ref/$name $T
    awk '{ print $1 }' $W/$first.index > $T/order
    ( cd $W && $PENGUIN createsubdb $T/order $db $T/sub -v 1 --subdb-mode 1 \
            && $PENGUIN clust $T/sub $pref local/ref/$name/clu2 --cluster-mode 3 --threads 1 -v 1 \
            && $PENGUIN mergeclusters $db local/ref/$name/merged $first local/ref/$name/clu2 --threads 1 -v 1 ) > $T/log 2>&1 || { cat $T/log; exit 1; }
    printf '%s\t%s\t%s\t%s\t%s\n' "$name" "$db" "$first" "local/ref/$name/clu2" "$pref" >> $OUT/MERGES
}
merge merge_cases7 clust/cases clust/ref/cases7_m3/out clust/ref/cases7_subset/pref_filter2
merge merge_ham_nucl14 hamming/nucl clust/ref/ham_nucl14_linclust_m3/out clust/ref/ham_nucl14_subset/pref_filter2
# linclust with the ungapped alignment module, every intermediate DB kept (the workflow's own script and its copies stay behind: data only)
# (-k and --kmer-per-seq given: the automatic choice is the reference's alone; the flags `penguin guided_nuclassemble` passes to its linclust, without
#  --wrapped-scoring 1, which the reference's mode 2 refuses: "wrapped scoring is only allowed with RESCORE_MODE_HAMMING")
LIN="--alignment-mode 4 --min-seq-id 0.97 -c 0.9 --cov-mode 1 -k 22 --kmer-per-seq 60 --kmer-per-seq-scale 0.1 --alph-size nucl:5,aa:13 --hash-shift 67 --ignore-multi-kmer 1 -e 0.001 --cluster-mode 3 --remove-tmp-files 0 --threads 1 -v 1"
mkdir -p $OUT/ref/linclust
( cd $OUT && $PENGUIN linclust nucl ref/linclust/clu $W/lintmp $LIN > $W/linclust.log 2>&1 ) || { cat $W/linclust.log; exit 1; }
for f in pref pref_rescore1 pre_clust pref_filter2 aln clust; do
    for e in "" .index .dbtype; do cp -L $W/lintmp/latest/$f$e $OUT/ref/linclust/; done
done
cp -L $W/lintmp/latest/order_redundancy $OUT/ref/linclust/
# second line: the threshold of the alignment step, which the workflow runs with --filter-hits 1 (workflow/Linclust.cpp:119-127)
printf '%s\n%s\n' "$LIN" "$(threshold 1 0.97 0.9)" > $OUT/LINCLUST
tar -C $W -czf $HERE/local.tar.gz local
ls -l $HERE/local.tar.gz
rm -rf $W
