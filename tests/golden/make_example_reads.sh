#!/bin/bash
# GENERATION-TIME ONLY (build container): tests/golden/example_reads/ — the reference's bundled example read pairs (examples/reads_1.fastq.gz,
# examples/reads_2.fastq.gz of the reference repository: 5 000 pairs of 2 x 150 nt, 116 reads of mate 2 with an 'N'), copied unchanged.  They
# are the input the reference's `penguin nuclassemble` turned into nucl/seq_0 of example_nucl.tar.gz (make_golden.sh) with its mergereads
# step, so tests/test_gpu_mergereads.py can pin plass-hip mergereads on them.  Kept as the two .fastq.gz files (each under 1 MiB).
set -e
HERE=$(cd "$(dirname "$0")" && pwd); EX=${REF_EXAMPLES:?set REF_EXAMPLES to the examples/ directory of the reference repository}
mkdir -p $HERE/example_reads
cp $EX/reads_1.fastq.gz $EX/reads_2.fastq.gz $HERE/example_reads/
sha256sum $HERE/example_reads/*.fastq.gz
