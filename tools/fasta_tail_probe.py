"""Probe of the workflows' tail on the device (plasship_select_contigs + plasship_fasta_write) after the bench chain.

Builds the bench workload (default: configs[2], 50 M reads), runs the bench's iterations on it (bench.one_iteration: kmermatcher ->
rescorediagonal -> assembleresults, 12 by default) with the fragment DB kept as SOURCE, then selects the contigs as `plass assemble
--filter-proteins 0` does (data/assemble.sh:170-189) and writes the FASTA file.  Prints one JSON line: selection and FASTA kernel times,
bytes written, file-write time (the whole plasship_fasta_write call: formatting, device -> host copies, fwrite, rename).

    python tools/fasta_tail_probe.py [--config c3] [--iterations 12] [--out /tmp/probe.fasta] [--json FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--pairs", type=int, default=0)
    ap.add_argument("--iterations", type=int, default=12)
    ap.add_argument("--out", default="/tmp/fasta_tail_probe.fasta")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import bench
    import plass_amd
    with plass_amd.Context(0) as ctx:
        frag, wl = bench.build_workload(ctx, a.config, a.pairs or None)
        db = frag
        t0 = time.perf_counter()
        for it in range(a.iterations):
            out = bench.one_iteration(ctx, db, it)[0]
            if db is not frag:
                db.free()
            db = out
        ctx.sync()
        t1 = time.perf_counter()
        if os.path.exists(a.out):
            os.remove(a.out)
        ts = time.perf_counter()
        sel, st = ctx.select_contigs(db, frag, "protein")
        ts = time.perf_counter() - ts
        fs = ctx.write_fasta(sel, a.out)
        info = db.info()
        res = {"config": a.config, "reads": wl["reads"], "iterations": a.iterations, "chain_s": round(t1 - t0, 3),
               "result_entries": info["n"], "result_bytes": info["data_bytes"], "selected": st.n_selected, "s1_only": st.n_s1_only,
               "s2_only": st.n_s2_only, "both": st.n_both, "select_kernel_ms": round(st.ms_kernel, 3), "select_call_ms": round(ts * 1e3, 3),
               "fasta_bytes": fs.bytes, "fasta_chunks": fs.n_chunks, "fasta_kernel_ms": round(fs.ms_kernel, 3), "fasta_call_s": round(fs.ms_total * 1e-3, 3)}
        sel.free(); db.free(); frag.free()
    os.remove(a.out)
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
