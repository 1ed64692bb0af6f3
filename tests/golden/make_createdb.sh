#!/bin/bash
# GENERATION-TIME ONLY (build container): tests/golden/createdb.tar.gz — the reference's createdb (lib/mmseqs/src/util/createdb.cpp) pinned
# on small read files.  The inputs come from make_createdb_inputs.py; the UNMODIFIED reference runs on every case the CASES file marks "ok",
# with its defaults (--shuffle 1) and, on the cases named in S0, with --shuffle 0, from inside the input directory so that .source holds bare file names.  The tarball
# keeps DATA only: the inputs, CASES, per case and mode the eight files createdb wrote (DB, .index, .dbtype, _h, _h.index, _h.dbtype, .lookup,
# .source) and a MANIFEST.  Reference binary: an out-of-tree build of the reference (REF_BUILD, default /tmp/plass-build).
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd)
B=${REF_BUILD:-/tmp/plass-build}; PLASS=$B/src/plass
S0="n1 n33 mixed_fq wrapped crlf_fa nonl_fq"
W=$(mktemp -d); OUT=$W/createdb; mkdir -p $OUT/in $OUT/ref
python3 $HERE/make_createdb_inputs.py $OUT/in
echo "# plass createdb <files> <db> [--shuffle 0] -v 1, run in in/" > $OUT/MANIFEST
while IFS=$'\t' read -r name expect files; do
    [ "$expect" = "ok" ] || continue
    for mode in s1 s0; do
        [ $mode = s1 ] || [[ " $S0 " == *" $name "* ]] || continue
        mkdir -p $OUT/ref/$name/$mode
        flag=""; [ $mode = s0 ] && flag="--shuffle 0"
        ( cd $OUT/in && $PLASS createdb $files ../ref/$name/$mode/db $flag -v 1 )
        [ "$(od -An -tu4 $OUT/ref/$name/$mode/db.dbtype | tr -d ' ')" = 1 ] || { echo "$name: the reference does not call this case nucleotides"; exit 1; }
        echo "$name/$mode: createdb $files db $flag" >> $OUT/MANIFEST
    done
done < $OUT/in/CASES
( cd $OUT && sha256sum ref/*/*/db >> MANIFEST )
tar -C $W -czf $HERE/createdb.tar.gz createdb
# mate 1 of the bundled example as a single-end library: the DB the chains of tests/test_gpu_createdb.py start from (a tarball of its own,
# without the input: tests/golden/example_reads/reads_1.fastq.gz is in the repository)
mkdir -p $W/createdb_example
( cd $HERE/example_reads && $PLASS createdb reads_1.fastq.gz $W/createdb_example/db -v 1 )
tar -C $W -czf $HERE/createdb_example.tar.gz createdb_example
ls -l $HERE/createdb.tar.gz $HERE/createdb_example.tar.gz
rm -rf $W
