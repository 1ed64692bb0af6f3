#!/bin/bash
# GENERATION-TIME ONLY (build container): tests/golden/clust.tar.gz — the reference's `clust --cluster-mode 3` (and one `--cluster-mode 2`:
# both run ClusteringAlgorithms::greedyIncrementalLowMem, lib/mmseqs/src/clustering/ClusteringAlgorithms.cpp:271-332) pinned on small
# sequence DBs and result DBs of dbtype 7, 14 and 5, and linclust's createsubdb / createsubdb / filterdb subset of a prefilter DB
# (lib/mmseqs/data/workflow/linclust.sh:39-56).  The inputs are the hand-written DBs of make_clust_inputs.py and the DBs of hamming.tar.gz:
# its sequence DBs, and as result DBs the Hamming outputs the reference wrote there (they are not copied: a test unpacks both tarballs side by
# side).  The UNMODIFIED reference runs every step.  The tarball keeps DATA only: the hand-written input DBs, NAMES, RUNS (one line per run:
# name, sequence DB, result DB, the flags), SUBSETS (name, sequence DB, prefilter DB, the run whose cluster DB gives the keys) and per run the
# files the reference wrote.  Reference binary: an out-of-tree cmake + ninja build of the reference (REF_BUILD, default /tmp/plass-build).
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd)
B=${REF_BUILD:-/tmp/plass-build}; PENGUIN=$B/src/penguin
W=$(mktemp -d); OUT=$W/clust; mkdir -p $OUT/ref
tar -C $W -xzf $HERE/hamming.tar.gz
python3 $HERE/make_clust_inputs.py $OUT
: > $OUT/RUNS; : > $OUT/SUBSETS
run() {     # <name> <seqDB> <resultDB> <flags…>   (paths from the directory both tarballs are unpacked in)
    local name=$1 db=$2 res=$3; shift 3
    mkdir -p $OUT/ref/$name
    ( cd $W && $PENGUIN clust $db $res clust/ref/$name/out "$@" --threads 1 -v 1 > clust/ref/$name.log 2>&1 ) || { cat $OUT/ref/$name.log; exit 1; }
    rm -f $OUT/ref/$name.log
    printf '%s\t%s\t%s\t%s\n' "$name" "$db" "$res" "$*" >> $OUT/RUNS
}
subset() {  # <name> <seqDB> <prefDB> <run>: linclust.sh:39-56 with the run's cluster DB as pre_clust
    local name=$1 db=$2 pref=$3 clu=$4 T=$W/tmp_$1
    mkdir -p $OUT/ref/$name $T
    awk '{ print $1 }' $OUT/ref/$clu/out.index > $T/order_redundancy
    ( cd $W && $PENGUIN createsubdb $T/order_redundancy $db $T/input_step_redundancy -v 1 --subdb-mode 1 \
            && $PENGUIN createsubdb $T/order_redundancy $pref $T/pref_filter1 -v 1 --subdb-mode 1 \
            && $PENGUIN filterdb $T/pref_filter1 clust/ref/$name/pref_filter2 --filter-file $T/order_redundancy --threads 1 -v 1 ) > $T/log 2>&1 || { cat $T/log; exit 1; }
    printf '%s\t%s\t%s\t%s\n' "$name" "$db" "$pref" "$clu" >> $OUT/SUBSETS
}
run cases7_m3 clust/cases clust/cases7 --cluster-mode 3
run cases7_m2 clust/cases clust/cases7 --cluster-mode 2
run cases14_m3 clust/cases clust/cases14 --cluster-mode 3
run cases5_m3 clust/cases clust/cases5 --cluster-mode 3 --max-iterations 1000 --similarity-type 2
run star7_m3 clust/star clust/star7 --cluster-mode 3
run equal7_m3 clust/equal clust/equal7 --cluster-mode 3
run ham_nucl7_linclust_m3 hamming/nucl hamming/ref/pref_nucl7_linclust_w1/out --cluster-mode 3
run ham_nucl14_linclust_m3 hamming/nucl hamming/ref/pref_nucl14_linclust_w1/out --cluster-mode 3
run ham_nucl14_loose_m3 hamming/nucl hamming/ref/pref_nucl14_loose_w1/out --cluster-mode 3
run ham_prot7_loose_m3 hamming/prot hamming/ref/pref_prot7_loose_w0/out --cluster-mode 3
subset cases7_subset clust/cases clust/cases7 cases7_m3
subset ham_nucl14_subset hamming/nucl hamming/pref_nucl14 ham_nucl14_linclust_m3
tar -C $W -czf $HERE/clust.tar.gz clust
ls -l $HERE/clust.tar.gz
rm -rf $W
