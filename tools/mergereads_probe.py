#!/usr/bin/env python3
"""mergereads throughput on the GPU box: N synthetic 2 x 150 nt pairs (plass_amd.synth: gene-dense genome, inserts ~N(320, 40), plus a
quarter of the pairs from short inserts so that they merge) written as FASTQ, plain and gz, then plasship_mergereads on each and the read DB
written out.  Reports pairs/s and the split into parse (read / gunzip, validate, pack, header DB), upload, kernels and write.
    python tools/mergereads_probe.py [pairs] [--gz-only | --plain-only]    (PLASSHIP_MERGE_BATCH, PLASSHIP_HOST_THREADS as usual)"""
import gzip
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plass_amd  # noqa: E402
from plass_amd import synth  # noqa: E402

pairs = int(float(sys.argv[1])) if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else 5000000
modes = ["plain", "gz"]
if "--gz-only" in sys.argv:
    modes = ["gz"]
if "--plain-only" in sys.argv:
    modes = ["plain"]
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def write_fastq(paths, n, seed=5, chunk=1000000):
    """both mates of n pairs, chunk by chunk; every record has the same width ("@r<10 digits>/<mate>"), so a chunk is one uint8 array"""
    rng = np.random.default_rng(seed)
    genome = synth.make_genome(rng, 20000000)
    outs = [open(p, "wb") if not p.endswith(".gz") else gzip.open(p, "wb", compresslevel=1) for p in paths]
    qual = np.frombuffer(b"FFFFF:FFF,FFFFFFF:F", dtype=np.uint8)
    col = lambda m, c: np.full((m, 1), c, np.uint8)
    for c0 in range(0, n, chunk):
        m = min(chunk, n - c0)
        reads = synth.make_reads(rng, genome, m, read_len=150)
        short = rng.random(m) < 0.25                                   # short inserts: the mates overlap
        ins = rng.integers(160, 281, size=m)
        pos = rng.integers(0, genome.size - 300, size=m)
        idx = np.arange(150)
        a, b = reads[0::2], reads[1::2]
        a[short] = genome[pos[short][:, None] + idx[None, :]]
        b[short] = 3 - genome[(pos + ins)[short][:, None] - 1 - idx[None, :]]
        digits = ((np.arange(c0, c0 + m, dtype=np.int64)[:, None] // 10 ** np.arange(9, -1, -1)[None, :]) % 10 + 48).astype(np.uint8)
        for mate, (f, r) in enumerate(zip(outs, (a, b))):
            rec = np.concatenate([col(m, 64), col(m, 114), digits, col(m, 47), col(m, 49 + mate), col(m, 10), ACGT[r], col(m, 10), col(m, 43),
                                  col(m, 10), qual[rng.integers(0, qual.size, size=r.shape)], col(m, 10)], axis=1)
            f.write(rec.tobytes())
    for f in outs:
        f.close()


with tempfile.TemporaryDirectory(dir=os.environ.get("PROBE_TMP")) as td, plass_amd.Context(0) as ctx:
    for mode in modes:
        ext = ".fastq" if mode == "plain" else ".fastq.gz"
        paths = [os.path.join(td, "r_%d%s" % (k, ext)) for k in (1, 2)]
        t0 = time.perf_counter()
        write_fastq(paths, pairs)
        mb = sum(os.path.getsize(p) for p in paths) / 1e6
        print("%s: %d pairs written in %.1f s (%.0f MB on disk)" % (mode, pairs, time.perf_counter() - t0, mb), flush=True)
        t1 = time.perf_counter()
        reads, hdr, st = ctx.mergereads(paths)
        ctx.sync()
        t2 = time.perf_counter()
        reads.write(os.path.join(td, "out")); hdr.write(os.path.join(td, "out_h"))
        t3 = time.perf_counter()
        call = t2 - t1
        print("%s: pairs %d combined %d (%.1f %%) | call %.3f s = %.2f M pairs/s | parse %.3f s upload %.3f s kernels %.3f s | write %.3f s"
              % (mode, st.pairs, st.combined, 100.0 * st.combined / max(st.pairs, 1), call, st.pairs / call / 1e6, st.ms_parse * 1e-3,
                 st.ms_upload * 1e-3, st.ms_kernel * 1e-3, t3 - t2), flush=True)
        reads.free(); hdr.free()
        for p in paths:
            os.unlink(p)
