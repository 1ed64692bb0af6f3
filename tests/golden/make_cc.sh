#!/bin/bash
# GENERATION-TIME ONLY (build container): tests/golden/cc.tar.gz — the reference's `clust --cluster-mode 1` (connected component:
# ClusteringAlgorithms::execute(3), lib/mmseqs/src/clustering/ClusteringAlgorithms.cpp:81-111, on the lists readInClusterData symmetrises) pinned on
# the hand-made graphs of make_cc_inputs.py (tests/tools/cc_cases.py), and one nucleotide and one protein `linclust --alignment-mode 4
# --cluster-mode 1` with their intermediate DBs, on the sequence DBs of local.tar.gz and subst.tar.gz (they are not copied: a test unpacks the
# tarballs side by side).  The UNMODIFIED reference runs every step.  The tarball keeps DATA only: the hand-written input DBs and
#   RUNS           one line per clust run: name, sequence DB, result DB, the flags, and "ok" or "fail" ("fail": the reference ended with an error
#                  and wrote no DB — the result DB without an entry for one sequence)
#   LINCLUST_NUCL, LINCLUST_PROT   the flags of the linclust run and, on a second line, the threshold its rescore steps took for --filter-hits 1
#                  (the lookup make_local.sh states); the DBs are under ref/linclust_nucl/ and ref/linclust_prot/, with rep = result2repseq of clu
# and per run the files the reference wrote.  The run `dup` (an entry that lists one target twice) is made ten times and kept only because the ten
# agree.  Reference binary: an out-of-tree cmake + ninja build of the reference, as the header of make_local.sh describes (REF_BUILD, default
# /tmp/plass-build); REF_SRC: its source tree.
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd)
B=${REF_BUILD:-/tmp/plass-build}; PENGUIN=$B/src/penguin
SRC=${REF_SRC:?set REF_SRC to the source tree of the reference}
W=$(mktemp -d); OUT=$W/cc; mkdir -p $OUT/ref
tar -C $W -xzf $HERE/local.tar.gz
tar -C $W -xzf $HERE/subst.tar.gz
python3 $HERE/make_cc_inputs.py $OUT
: > $OUT/RUNS
threshold() {   # <cov-mode> <min-seq-id> <-c>: parsePrecisionLib on the reference's data file
    local lib=$SRC/lib/mmseqs/data/resources/CovSeqidQscPercMinDiagTargetCov.lib
    [ "$1" = 0 ] && lib=$SRC/lib/mmseqs/data/resources/CovSeqidQscPercMinDiag.lib
    awk -v s="$2" -v c="$3" 'BEGIN { i = int((s + 0.0001) * 100); ts = (i - i % 5) / 100; tc = int((c + 0.0001) * 10) / 10; r = "0" }
        { dc = $1 - tc; ds = $2 - ts; if (dc < 0) dc = -dc; if (ds < 0) ds = -ds; if (dc < 1e-6 && ds < 1e-6 && $4 >= 0.99) { r = $3; exit } }
        END { print r }' "$lib"
}
flag() {        # <name> <flags…>: the value behind a flag
    local want=$1 prev=""; shift
    for a in "$@"; do if [ "$prev" = "$want" ]; then echo "$a"; return; fi; prev=$a; done
}
while IFS=$'\t' read -r name db res flags; do
    mkdir -p $OUT/ref/$name
    status=ok
    # shellcheck disable=SC2086
    ( cd $W && $PENGUIN clust $db $res cc/ref/$name/out $flags --threads 1 -v 1 > $W/$name.log 2>&1 ) || status=fail
    if [ $status = fail ]; then
        [ "$name" = noentry ] || { cat $W/$name.log; exit 1; }
        grep -q "Sequence db size != result db size" $W/$name.log
        rm -rf $OUT/ref/$name
    fi
    if [ "$name" = dup ]; then
        for i in 1 2 3 4 5 6 7 8 9; do
            # shellcheck disable=SC2086
            ( cd $W && $PENGUIN clust $db $res $W/dup_again_$i $flags --threads 4 -v 1 > $W/$name.log 2>&1 ) || { cat $W/$name.log; exit 1; }
            cmp $W/dup_again_$i $OUT/ref/dup/out && cmp $W/dup_again_$i.index $OUT/ref/dup/out.index
        done
    fi
    printf '%s\t%s\t%s\t%s\t%s\n' "$name" "$db" "$res" "$flags" "$status" >> $OUT/RUNS
done < $OUT/RUNLIST
rm -f $OUT/RUNLIST
# linclust with the ungapped alignment module and connected component, every intermediate DB kept: the flags of local.tar.gz's and subst.tar.gz's
# runs with --cluster-mode 1 in place of their greedy mode
lin() {         # <name> <seqDB> <flags file> <intermediate DBs…>
    local name=$1 db=$2 flags; shift 2
    flags=$(head -n 1 "$1" | sed 's/--cluster-mode [0-9]/--cluster-mode 1/'); shift
    mkdir -p $OUT/ref/linclust_$name
    # shellcheck disable=SC2086
    ( cd $W && $PENGUIN linclust $db cc/ref/linclust_$name/clu $W/lintmp_$name $flags > $W/linclust_$name.log 2>&1 ) || { cat $W/linclust_$name.log; exit 1; }
    for f in "$@"; do
        for e in "" .index .dbtype; do cp -L $W/lintmp_$name/latest/$f$e $OUT/ref/linclust_$name/; done
    done
    cp -L $W/lintmp_$name/latest/order_redundancy $OUT/ref/linclust_$name/
    ( cd $W && $PENGUIN result2repseq $db cc/ref/linclust_$name/clu cc/ref/linclust_$name/rep --threads 1 -v 1 ) > $W/rep.log 2>&1 || { cat $W/rep.log; exit 1; }
    # shellcheck disable=SC2086
    printf '%s\n%s\n' "$flags" "$(threshold "$(flag --cov-mode $flags)" "$(flag --min-seq-id $flags)" "$(flag -c $flags)")"
}
lin nucl local/nucl $W/local/LINCLUST pref pref_rescore1 pre_clust pref_filter2 aln clust > $OUT/LINCLUST_NUCL
lin prot subst/fam $W/subst/LINCLUST pref pref_rescore1 pre_clust pref_filter2 pref_rescore2 aln clust > $OUT/LINCLUST_PROT
tar -C $W -czf $HERE/cc.tar.gz cc
ls -l $HERE/cc.tar.gz
rm -rf $W
