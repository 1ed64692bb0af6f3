"""GPU tests of the workflows' tail (`-m gpu`): plasship_select_contigs + plasship_fasta_write (Context.select_contigs / write_fasta) and
`plass-hip assemble-chain / nuclassemble-chain --fasta-out`, against the FASTA files the unmodified reference wrote
(tests/golden/fasta_tail_*.tar.gz) and against tests/tools/contigcheck.py (pinned on those files by tests/test_contigcheck.py).
Every comparison is exact."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import contigcheck  # noqa: E402
from test_contigcheck import CASES, extract_case  # noqa: E402

HIP = os.path.join(ROOT, "plass_amd", "plass-hip")
EXAMPLE = [os.path.join(ROOT, "tests", "golden", "example_reads", "reads_%d.fastq.gz" % i) for i in (1, 2)]


@pytest.fixture
def ctx():
    # (per test: a context keeps its device arena until it is closed, and the chain tests start plass-hip processes of their own)
    import plass_amd
    c = plass_amd.Context(0)
    yield c
    c.close()


def file_matches(path, ref):
    got = open(path, "rb").read()
    return contigcheck.matches(got, ref), len(got)


def upload(ctx, seqs, keys, dbtype):
    """a DB of the byte strings `seqs` under `keys` (any order)"""
    ent = [s + b"\n\0" for s in seqs]
    elen = np.array([len(e) for e in ent], dtype=np.uint32)
    off = np.zeros(len(ent), dtype=np.uint64)
    if len(ent) > 1:
        off[1:] = np.cumsum(elen[:-1], dtype=np.uint64)
    return ctx.upload_seqdb(b"".join(ent), off, elen, np.asarray(keys, dtype=np.uint32), dbtype)


def upload_index(ctx, db, dbtype):
    """SOURCE / the cycle DB of a fixture are indexes only: a DB with the same keys and entry lengths (residues 'A')"""
    return upload(ctx, [b"A" * (int(l) - 2) for l in db.elen], db.keys, dbtype)


def checker_db(seqs, keys):
    ent = [s + b"\n\0" for s in seqs]
    elen = np.array([len(e) for e in ent], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(elen)[:-1]]) if len(ent) else np.zeros(0, dtype=np.int64)
    # the checker's data file in KEY order (the canonical layout the device DB has)
    o = np.argsort(np.asarray(keys), kind="stable")
    data = np.frombuffer(b"".join(ent[i] for i in o), dtype=np.uint8) if len(ent) else np.zeros(0, dtype=np.uint8)
    off_sorted = np.zeros(len(ent), dtype=np.int64)
    if len(ent):
        off_sorted[o] = np.concatenate([[0], np.cumsum(elen[o])[:-1]])
    return contigcheck.DB(np.asarray(keys, dtype=np.int64), off_sorted, elen, data)


@pytest.mark.parametrize("case", CASES)
def test_capi_matches_reference_fasta(case, ctx, tmp_path):
    """the fixture's RESULT, SOURCE and cycle DBs through select_contigs + write_fasta: the reference's FASTA byte for byte"""
    d = extract_case(case, tmp_path)
    mode, flags, result, source, cyc, ref = contigcheck.fixture_case(d)
    only, mn = contigcheck.case_params(flags)
    dbtype = 0 if mode == "protein" else 1
    r = ctx.read_seqdb(os.path.join(d, "result"))
    s = upload_index(ctx, source, dbtype)
    c = upload(ctx, [b"A"] * len(cyc), cyc, dbtype) if cyc is not None else None
    sel, st = ctx.select_contigs(r, s, mode, cycles=c, only_extended=only, min_contig_len=mn)
    out = tmp_path / "out.fasta"
    fs = ctx.write_fasta(sel, out, cycles=c)
    ok, n = file_matches(out, ref)
    print("%s: %d selected (S1 only %d, S2 only %d, both %d, circular %d), %d bytes, select %.3f ms, format %.3f ms"
          % (case, st.n_selected, st.n_s1_only, st.n_s2_only, st.n_both, st.n_cycle, n, st.ms_kernel, fs.ms_kernel))
    assert ok, "%s: the GPU FASTA differs from the reference's" % case
    assert st.n_selected > 0 and fs.bytes == n
    sel.free(); s.free(); r.free()
    if c is not None:
        c.free()


def run_chain(args, timeout=900):
    p = subprocess.run([HIP] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert p.returncode == 0 and "Time for processing" in p.stdout, p.stdout[-3000:]
    return p


def test_chains_end_to_end_match_reference(tmp_path):
    """plass-hip chains from the FASTQ pairs with --fasta-out: the FASTA of the unmodified workflows on cases 1-5"""
    for c in CASES + ["reads"]:
        with __import__("tarfile").open(os.path.join(ROOT, "tests", "golden", "fasta_tail_%s.tar.gz" % c)) as t:
            t.extractall(tmp_path)
    F = tmp_path / "fasta_tail"
    circ = [F / "reads" / "circ_1.fastq.gz", F / "reads" / "circ_2.fastq.gz"]
    runs = {
        "case1": ["assemble-chain"] + EXAMPLE + ["--filter-proteins", "0"],
        "case2": ["assemble-chain"] + EXAMPLE + ["--filter-proteins", "0", "--keep-target", "0"],
        "case3": ["nuclassemble-chain"] + circ,
        "case4": ["nuclassemble-chain"] + EXAMPLE + ["--contig-output-mode", "0", "--min-contig-len", "200"],
        "case5": ["nuclassemble-chain"] + circ,
    }
    bad = []
    for case, args in runs.items():
        out = tmp_path / (case + ".fasta")
        p = run_chain(args[:3] + [tmp_path / (case + "_db")] + args[3:] + ["--fasta-out", out])
        _, _, _, _, _, ref = contigcheck.fixture_case(str(F / case))
        ok, n = file_matches(out, ref)
        print(case, "match" if ok else "DIFFERS", n, [l for l in p.stdout.splitlines() if l.startswith("fasta:")])
        if not ok:
            bad.append(case)
    assert not bad, "chain FASTA differs from the reference's: %s" % bad


def crafted_protein():
    big = b"*" + bytes(np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYZ", dtype=np.uint8)[np.arange(59998) % 21]) + b"*"
    big_bad = big[:59000] + b"a" + big[59001:]                        # one lower-case byte deep inside: the wavefront must find it
    mid = b"*" + b"Q" * 400 + b"*"                                    # longer than the per-thread scan
    seqs = [b"**", b"*A*", b"*X*", b"*a*", b"*AB*CD*", b"*", b"", b"A*", b"*A", big, big_bad, mid, b"*AZ*", b"*@*", b"*[*", b"MKV", b"*M" * 3]
    seqs += [b"*" + b"B" * (i % 7) + b"*" for i in range(40)] + [b"K" * (5 + i) for i in range(40)]
    n = len(seqs)
    # non-contiguous keys: the first part keeps keys 0.., the rest jumps (rank k and key k disagree from there on)
    keys = list(range(20)) + [20 + 3 * i for i in range(n - 20)]
    # SOURCE: shorter, equal and longer entries for some keys, keys RESULT does not have, RESULT keys it lacks
    skeys, sseqs = [], []
    for i, (k, s) in enumerate(zip(keys, seqs)):
        if i % 4 == 0:
            continue                                                    # RESULT key absent from SOURCE
        L = len(s) + (-1 if i % 4 == 1 else 0 if i % 4 == 2 else 1)   # shorter (S1), equal (not S1), longer
        skeys.append(k); sseqs.append(b"A" * max(0, L))
    skeys += [10 ** 6 + i for i in range(5)]; sseqs += [b"A"] * 5
    return seqs, keys, sseqs, skeys


def crafted_nucl(thr):
    seqs, keys = [], []
    for i, L in enumerate([thr - 1, thr, thr + 1, 0, 1, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 199999]):
        seqs.append(b"ACGT" * (L // 4) + b"ACG"[:L % 4]); keys.append(5 * i + 1)
    return seqs, keys


def compare(ctx, tmp_path, name, r_seqs, r_keys, s_seqs, s_keys, mode, dbtype, cyc_keys=None, only=True, mn=1000):
    r = upload(ctx, r_seqs, r_keys, dbtype); s = upload(ctx, s_seqs, s_keys, dbtype)
    c = upload(ctx, [b"A"] * len(cyc_keys), cyc_keys, dbtype) if cyc_keys is not None else None
    sel, st = ctx.select_contigs(r, s, mode, cycles=c, only_extended=only, min_contig_len=mn)
    out = tmp_path / (name + ".fasta")
    ctx.write_fasta(sel, out, cycles=c)
    got = open(out, "rb").read()
    R = checker_db(r_seqs, r_keys); S = checker_db(s_seqs, s_keys)
    ids, sets = contigcheck.select(mode, R, S, only, mn)
    want = contigcheck.fasta(R, ids, cyc_keys)
    print("%s: %d of %d selected, %d bytes" % (name, st.n_selected, len(r_seqs), len(got)))
    assert got == want, name
    assert st.n_selected == len(ids)
    if mode == "protein":
        assert (st.n_s1_only, st.n_s2_only, st.n_both) == (int(np.sum(sets["s1"] & ~sets["s2"])), int(np.sum(sets["s2"] & ~sets["s1"])), int(np.sum(sets["s1"] & sets["s2"])))
    sel.free(); r.free(); s.free()
    if c is not None:
        c.free()
    return len(ids), got


def test_crafted_dbs_against_checker(ctx, tmp_path):
    seqs, keys, sseqs, skeys = crafted_protein()
    n, got = compare(ctx, tmp_path, "protein", seqs, keys, sseqs, skeys, "protein", 0)
    assert n > 0
    # every key order: RESULT uploaded shuffled (the handle is key-ordered whatever the input order)
    p = np.random.default_rng(5).permutation(len(seqs))
    n2, got2 = compare(ctx, tmp_path, "protein_shuffled", [seqs[i] for i in p], [keys[i] for i in p], sseqs, skeys, "protein", 0)
    assert got2 == got
    # nucleotide: min length at thr-1 / thr / thr+1, lengths at every digit boundary, mode 0 and 1, cycle field on and off
    thr = 1000
    nseqs, nkeys = crafted_nucl(thr)
    src = [s[:-1] if i % 3 == 0 else s if i % 3 == 1 else s[:0] for i, s in enumerate(nseqs)]    # shorter / equal / (much) shorter
    for only in (True, False):
        for cyc in (None, nkeys[::2], []):
            compare(ctx, tmp_path, "nucl_%d_%s" % (only, "none" if cyc is None else len(cyc)), nseqs, nkeys, src, nkeys, "nucleotide", 1, cyc, only, thr)
    # an empty selection gives an empty file
    n0, got0 = compare(ctx, tmp_path, "empty", nseqs, nkeys, src, nkeys, "nucleotide", 1, None, False, 10 ** 6)
    assert n0 == 0 and got0 == b""


def test_ranks_at_every_digit_boundary(ctx, tmp_path):
    """200 000 selected entries (ranks 0..199 999), in output chunks of 1 MB"""
    rng = np.random.default_rng(11)
    n = 200000
    lens = rng.integers(0, 12, n)
    lens[[9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 199999]] = [9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 199999]
    seqs = [b"C" * int(L) for L in lens]
    keys = list(range(0, 2 * n, 2))
    os.environ["PLASSHIP_TUNE_FASTA_CHUNK_MB"] = "1"
    try:
        for cyc in (None, keys[::7]):
            compare(ctx, tmp_path, "digits", seqs, keys, [b""], [1], "nucleotide", 1, cyc, False, 0)
    finally:
        del os.environ["PLASSHIP_TUNE_FASTA_CHUNK_MB"]


def sha_file(path):
    h = hashlib.sha256(); n = 0
    with open(path, "rb") as f:
        while True:
            b = f.read(1 << 24)
            if not b:
                break
            h.update(b); n += len(b)
    return h.hexdigest(), n


@pytest.mark.timeout(1500)
def test_configs1_chain_fasta_against_checker(tmp_path):
    """configs[1] (1 M reads, 6 iterations): the fused chain's final DB and its --fasta-out file, the FASTA against the checker on the DB files"""
    import bench
    import plass_amd
    with plass_amd.Context(0) as c:
        frag, _ = bench.build_workload(c, "c2")
        frag.write(tmp_path / "frag")
        frag.free()
    out = tmp_path / "c2.fasta"
    run_chain(["assemble-chain", tmp_path / "frag", tmp_path / "asm", "--num-iterations", "6", "--filter-proteins", "0", "--fasta-out", out], timeout=1200)
    R = contigcheck.read_db(str(tmp_path / "asm"))
    S = contigcheck.read_db(str(tmp_path / "frag"), with_data=False)
    ids, sets = contigcheck.select("protein", R, S)
    want = contigcheck.fasta_sha256(R, ids)
    got = sha_file(out)
    print("configs[1]: %d of %d selected (S2 only %d), %d bytes" % (len(ids), R.n, int(np.sum(sets["s2"] & ~sets["s1"])), got[1]))
    assert len(ids) > 0 and got == want


@pytest.mark.timeout(1500)
def test_data_beyond_4gib_every_entry(ctx, tmp_path):
    """the filler DB of test_offsets_beyond_4gib_against_oracle_checksums (4.48 GB), every entry selected: the FASTA's sha256 against the
    checker's, streamed in chunks"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_big_offsets as mk
    fb = mk.write_filler_db(str(tmp_path / "filler"))
    assert fb > (1 << 32)
    db = ctx.read_seqdb(tmp_path / "filler")
    src = upload(ctx, [b""], [0], 0)
    sel, st = ctx.select_contigs(db, src, "nucleotide", only_extended=False, min_contig_len=0)
    assert st.n_selected == db.info()["n"]
    out = tmp_path / "big.fasta"
    fs = ctx.write_fasta(sel, out)
    sel.free(); src.free(); db.free()
    got = sha_file(out)
    os.remove(out)
    k, o, l = contigcheck.read_index(str(tmp_path / "filler") + ".index")
    R = contigcheck.DB(k, o, l, np.memmap(str(tmp_path / "filler"), dtype=np.uint8, mode="r"))
    want = contigcheck.fasta_sha256(R, np.arange(R.n))
    print("beyond 4 GiB: %d entries, %d bytes in %d chunks, format %.1f ms, call %.1f s" % (fs.n_entries, fs.bytes, fs.n_chunks, fs.ms_kernel, fs.ms_total * 1e-3))
    assert got == want and fs.n_chunks > 1
