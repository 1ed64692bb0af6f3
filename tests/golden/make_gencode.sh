#!/bin/bash
# GENERATION-TIME ONLY (build container): tests/golden/gencode.tar.gz — the reference's extractorfs (with and without --translate 1) and translatenucs
# (--add-orf-stop 0 and 1) for EVERY genetic code it accepts (mm/commons/TranslateNucl.h:82-108: 1-6, 9-16, 21-31), each with --use-all-table-starts 0
# and 1, on the hand-made read DB of make_gencode_inputs.py; the same calls with the ids 0, 7, 17 and 32, which it refuses; and the preprocessing of
# data/assemble.sh:41-77 (two extractorfs passes, translatenucs, concatdbs) with --translation-table 11 --use-all-table-starts 1 and with table 4.
# The UNMODIFIED reference runs every step, single-threaded.  The tarball keeps DATA only: the input DB (in, in_h), every DB the reference wrote, and
#   RUNS           one line per run: name, module, input DB(s), output DB, the flags, and "ok" or "fail" ("fail": the reference ended with "Invalid
#                  translation table selected!" — or, for id 0, with "Error in argument --translation-table", the flag's pattern being
#                  ^[1-9]{1}[0-9]*$ — and what it had written by then is not kept)
# Reference binary: an out-of-tree cmake + ninja build of the reference, as the header of make_local.sh describes (REF_BUILD, default
# /tmp/plass-build), on a machine with AVX2: Orf.cpp's codon comparison has one code path per instruction set, and the one without AVX2 never matches
# a list of more than four codons (Orf.cpp:219-223), so --use-all-table-starts 1 with tables 2, 4, 5, 11, 13 and 24 would find no start there.
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd)
B=${REF_BUILD:-/tmp/plass-build}; PLASS=$B/src/plass
grep -q -w avx2 /proc/cpuinfo
W=$(mktemp -d); OUT=$W/gencode; mkdir -p $OUT
python3 $HERE/make_gencode_inputs.py $OUT
: > $OUT/RUNS
while IFS=$'\t' read -r name module src dst flags; do
    status=ok
    # shellcheck disable=SC2086
    ( cd $OUT && $PLASS $module $src $dst $flags --threads 1 -v 3 > $W/$name.log 2>&1 ) || status=fail
    if [ $status = fail ]; then
        grep -q -e "Invalid translation table selected" -e "Error in argument --translation-table" $W/$name.log || { cat $W/$name.log; exit 1; }
        rm -f $OUT/$dst $OUT/$dst.* $OUT/${dst}_h $OUT/${dst}_h.*
    fi
    printf '%s\t%s\t%s\t%s\t%s\t%s\n' "$name" "$module" "$src" "$dst" "$flags" "$status" >> $OUT/RUNS
done < $OUT/RUNLIST
rm -f $OUT/RUNLIST
# links to the input's ancillary files (softlinkDb) carry nothing a test reads
find $OUT -type l -delete
tar -C $W -czf $HERE/gencode.tar.gz gencode
ls -l $HERE/gencode.tar.gz
rm -rf $W
