#!/usr/bin/env python3
"""createdb throughput on the GPU box: N synthetic single 150-nt reads written as one FASTQ file, plain and gz, then plasship_createdb_write
on each.  Reports reads/s and the split into read (pread / gunzip on the host), upload (with the newline count under it), kernels (of these:
the kernel that writes the entries, with its fraction of the HBM peak from its algorithmic bytes) and the DB files.
    python tools/createdb_probe.py [reads] [--gz-only | --plain-only]    (PLASSHIP_TUNE_FASTQ_CHUNK_KB, PLASSHIP_HOST_THREADS as usual)"""
import gzip
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plass_amd  # noqa: E402
from plass_amd import synth  # noqa: E402

n_reads = int(float(sys.argv[1])) if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else 10000000
modes = ["plain", "gz"]
if "--gz-only" in sys.argv:
    modes = ["gz"]
if "--plain-only" in sys.argv:
    modes = ["plain"]
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
HBM_PEAK = 8.0e12       # bytes/s, MI355X data sheet


def write_fastq(path, n, seed=5, chunk=1000000):
    """the records of tools/mergereads_probe.py ("@r<10 digits>/1", 150 bases, '+', 150 quality bytes), all in one file"""
    rng = np.random.default_rng(seed)
    genome = synth.make_genome(rng, 20000000)
    out = open(path, "wb") if not path.endswith(".gz") else gzip.open(path, "wb", compresslevel=1)
    qual = np.frombuffer(b"FFFFF:FFF,FFFFFFF:F", dtype=np.uint8)
    col = lambda m, c: np.full((m, 1), c, np.uint8)
    for c0 in range(0, n, chunk):
        m = min(chunk, n - c0)
        r = synth.make_reads(rng, genome, (m + 1) // 2, read_len=150)[:m]
        digits = ((np.arange(c0, c0 + m, dtype=np.int64)[:, None] // 10 ** np.arange(9, -1, -1)[None, :]) % 10 + 48).astype(np.uint8)
        rec = np.concatenate([col(m, 64), col(m, 114), digits, col(m, 47), col(m, 49), col(m, 10), ACGT[r], col(m, 10), col(m, 43), col(m, 10),
                              qual[rng.integers(0, qual.size, size=r.shape)], col(m, 10)], axis=1)
        out.write(rec.tobytes())
    out.close()


with tempfile.TemporaryDirectory(dir=os.environ.get("PROBE_TMP")) as td, plass_amd.Context(0) as ctx:
    for mode in modes:
        path = os.path.join(td, "r" + (".fastq" if mode == "plain" else ".fastq.gz"))
        t0 = time.perf_counter()
        write_fastq(path, n_reads)
        print("%s: %d reads written in %.1f s (%.0f MB on disk)" % (mode, n_reads, time.perf_counter() - t0, os.path.getsize(path) / 1e6), flush=True)
        for rep in range(2):                                  # the second call finds the staging buffers and the pool warm
            t1 = time.perf_counter()
            reads, st = ctx.createdb([path])
            ctx.sync()
            t2 = time.perf_counter()
            reads.write(os.path.join(td, "out"))
            t3 = time.perf_counter()
            # the write kernel reads the sequence and header bytes and the per-line tables once and writes the two DBs once
            alg = 2 * st.bytes_out + st.lines * (8 + 4 + 4 + 8 + 8)
            print("%s #%d: reads %d | call %.3f s = %.2f M reads/s | read %.3f s upload+count %.3f s kernels %.4f s (write kernel %.3f ms: %.0f GB/s, "
                  "%.1f %% of HBM peak) | device parse = upload+count+kernels %.3f s | DB write %.3f s"
                  % (mode, rep, st.entries, t2 - t1, st.entries / (t2 - t1) / 1e6, st.ms_read * 1e-3, st.ms_upload * 1e-3, st.ms_kernel * 1e-3, st.ms_write_kernel,
                     alg / max(st.ms_write_kernel, 1e-6) / 1e6, 100.0 * alg / max(st.ms_write_kernel, 1e-6) * 1e3 / HBM_PEAK,
                     (st.ms_upload + st.ms_kernel) * 1e-3, t3 - t2), flush=True)
            reads.free()
        os.unlink(path)
