#!/bin/bash
# GENERATION-TIME ONLY (build container): tests/golden/mergereads_ladder.tar.gz — the hand-made read pairs of tests/tools/merge_ladder.py
# judged by the reference's own FLASH.  The three UNMODIFIED sources of lib/flash (combine_reads.cpp, read.cpp, util.cpp; their only
# include from outside that directory is simde, lib/mmseqs/lib/simde) are compiled with a plain g++ together with the driver
# oracle/tools/flash_pin.cpp into a temporary directory; the driver runs reverse_complement and combine_reads with mergereads'
# parameters (src/assembler/mergereads.cpp:19-24,75-111) on every rung.  The tarball keeps DATA only: per rung the two FASTQ files and
# <rung>.expected (per pair a status line, 1 combined or 0 not, then the one or two sequence entries), RUNGS (name, pairs, purpose) and a
# MANIFEST.  Nothing compiled and no source goes into it.  Reference sources: REF_SRC, the root of the reference's source tree.
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(cd "$HERE/../.." && pwd)
: "${REF_SRC:?set REF_SRC to the root of the reference source tree}"
W=$(mktemp -d); OUT=$W/mergereads_ladder; mkdir -p $OUT
g++ -O2 -std=c++17 -I$REF_SRC/lib -I$REF_SRC/lib/flash -I$REF_SRC/lib/mmseqs/lib/simde \
    $REF_SRC/lib/flash/combine_reads.cpp $REF_SRC/lib/flash/read.cpp $REF_SRC/lib/flash/util.cpp $ROOT/oracle/tools/flash_pin.cpp -lpthread -o $W/flash_pin
python3 $ROOT/tests/tools/merge_ladder.py $OUT
{
    echo "mergereads_ladder: the read pairs of tests/tools/merge_ladder.py and what the reference's FLASH makes of them."
    echo "<rung>_1.fastq, <rung>_2.fastq: the pairs (mate 2 as sequenced).  <rung>.expected: per pair a line 1 (combined) or 0 (not), then the one"
    echo "or two sequence entries of the reference's mergereads, one per line.  RUNGS: name, pairs, purpose."
    echo "Judge: lib/flash of the reference, unmodified (reverse_complement, combine_reads), min_overlap 15, max_overlap 65,"
    echo "max_mismatch_density 0.10, cap_mismatch_quals false, allow_outies false, called by oracle/tools/flash_pin.cpp."
    echo "The driver reads strict four-line FASTQ itself and bypasses kseq: the parser's rules (CR LF, names, refusals) are not pinned here."
    echo "rung pairs combined"
} > $OUT/MANIFEST
while IFS=$'\t' read -r name pairs purpose; do
    $W/flash_pin $OUT/${name}_1.fastq $OUT/${name}_2.fastq > $OUT/$name.expected
    echo "$name $pairs $(grep -c '^1$' $OUT/$name.expected || true)" >> $OUT/MANIFEST
done < $OUT/RUNGS
tar -C $W --sort=name --mtime=@0 --owner=0 --group=0 --numeric-owner -cf - mergereads_ladder | gzip -9n > $HERE/mergereads_ladder.tar.gz
ls -l $HERE/mergereads_ladder.tar.gz
rm -rf $W
