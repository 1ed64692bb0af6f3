#!/bin/bash
# GENERATION-TIME ONLY (build container): tests/golden/subst.tar.gz — the reference's `rescorediagonal --rescore-mode 1` (the best local score on
# the candidate's diagonal: the filter step linclust runs on amino-acid DBs, lib/mmseqs/src/alignment/rescorediagonal.cpp:193-334 with
# DistanceCalculator.h:16-38,93-175), one protein `linclust --alignment-mode 4` with its intermediate DBs and two `result2repseq` runs, pinned on
# small DBs.  The inputs are the hand-made pairs of make_subst_inputs.py (tests/tools/subst_cases.py) and the nucleotide DBs of local.tar.gz
# (they are not copied: a test unpacks the tarballs side by side).  The UNMODIFIED reference runs every step.  The tarball keeps DATA only:
# the hand-written input DBs, NAMES, and
#   RUNS     one line per rescorediagonal run: name, sequence DB, prefilter DB, the flags, and the score-per-column threshold the reference took
#            for --filter-hits 1 ("-": --filter-hits 0), looked up at generation time by the rule make_local.sh states (threshold() there and here:
#            parsePrecisionLib on the reference's own data file; 0 where it has no row).  The table is not copied.
#   LINCLUST the flags of the protein linclust run and, on a second line, the threshold its two rescore steps took (one lookup: both run with the
#            same --min-seq-id, -c and --cov-mode); its DBs are under ref/linclust_prot/, with ref/linclust_prot/rep = result2repseq of its clu
#   ref/rep_nucl  result2repseq of local.tar.gz's ref/linclust/clu on local/nucl
# and per run the files the reference wrote.  Reference binary: an out-of-tree cmake + ninja build of the reference, as the header of
# make_local.sh describes (REF_BUILD, default /tmp/plass-build); REF_SRC: its source tree.
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd)
B=${REF_BUILD:-/tmp/plass-build}; PENGUIN=$B/src/penguin
SRC=${REF_SRC:?set REF_SRC to the source tree of the reference}
W=$(mktemp -d); OUT=$W/subst; mkdir -p $OUT/ref
tar -C $W -xzf $HERE/local.tar.gz
python3 $HERE/make_subst_inputs.py $W
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
while IFS=$'\t' read -r name db pref flags; do
    thr=-
    # shellcheck disable=SC2086
    if [ "$(flag --filter-hits $flags)" = 1 ]; then thr=$(threshold "$(flag --cov-mode $flags)" "$(flag --min-seq-id $flags)" "$(flag -c $flags)"); fi
    mkdir -p $OUT/ref/$name
    # shellcheck disable=SC2086
    ( cd $W && $PENGUIN rescorediagonal $db $db $pref subst/ref/$name/out $flags --threads 1 -v 2 > $OUT/ref/$name.log 2>&1 ) || { cat $OUT/ref/$name.log; exit 1; }
    # the reference says so itself where its table has no row
    if [ "$thr" = 0 ]; then grep -q "No hit will be filtered" $OUT/ref/$name.log; elif grep -q "No hit will be filtered" $OUT/ref/$name.log; then echo "$name: no row"; exit 1; fi
    rm -f $OUT/ref/$name.log
    printf '%s\t%s\t%s\t%s\t%s\n' "$name" "$db" "$pref" "$flags" "$thr" >> $OUT/RUNS
done < $OUT/RUNLIST
# linclust on the protein DB with the ungapped alignment module, every intermediate DB kept (the workflow's own script and its copies stay behind)
LIN=$(cat $OUT/LINFLAGS)
mkdir -p $OUT/ref/linclust_prot
# shellcheck disable=SC2086
( cd $OUT && $PENGUIN linclust fam ref/linclust_prot/clu $W/lintmp $LIN > $W/linclust.log 2>&1 ) || { cat $W/linclust.log; exit 1; }
for f in pref pref_rescore1 pre_clust pref_filter2 pref_rescore2 aln clust; do
    for e in "" .index .dbtype; do cp -L $W/lintmp/latest/$f$e $OUT/ref/linclust_prot/; done
done
cp -L $W/lintmp/latest/order_redundancy $OUT/ref/linclust_prot/
# shellcheck disable=SC2086
printf '%s\n%s\n' "$LIN" "$(threshold "$(flag --cov-mode $LIN)" "$(flag --min-seq-id $LIN)" "$(flag -c $LIN)")" > $OUT/LINCLUST
# result2repseq: the sequence DB's ancillary files are soft links of the output (here: none exist besides the DB itself; the file set is recorded)
( cd $OUT && $PENGUIN result2repseq fam ref/linclust_prot/clu ref/linclust_prot/rep --threads 1 -v 1 ) > $W/rep.log 2>&1 || { cat $W/rep.log; exit 1; }
mkdir -p $OUT/ref/rep_nucl
( cd $W && $PENGUIN result2repseq local/nucl local/ref/linclust/clu subst/ref/rep_nucl/rep --threads 1 -v 1 ) > $W/rep.log 2>&1 || { cat $W/rep.log; exit 1; }
( cd $OUT/ref && ls linclust_prot/rep* rep_nucl/rep* ) > $OUT/REPFILES
rm -f $OUT/RUNLIST $OUT/LINFLAGS
tar -C $W -czf $HERE/subst.tar.gz subst
ls -l $HERE/subst.tar.gz
rm -rf $W
