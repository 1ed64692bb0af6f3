"""GPU tests of mergereads (`-m gpu`): plass-hip mergereads / plasship_mergereads against the reference's own output (nucl/seq_0 of
example_nucl.tar.gz is `nucl_reads` of the bundled example pairs) and against tests/tools/mergecheck.py (pinned on that output by
tests/test_mergereads_host.py) on synthetic pairs built to reach every rule of src/assembler/mergereads.cpp and lib/flash."""
import gzip
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_same_db, read_db

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import mergecheck  # noqa: E402

HIP = os.path.join(ROOT, "plass_amd", "plass-hip")
EXAMPLE = [os.path.join(ROOT, "tests", "golden", "example_reads", "reads_%d.fastq.gz" % i) for i in (1, 2)]


def run(args, env=None, ok=True):
    p = subprocess.run([HIP] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900,
                       env=dict(os.environ, **(env or {})))
    if ok:
        assert p.returncode == 0 and "Time for processing" in p.stdout, p.stdout[-3000:]
    return p


@pytest.fixture(scope="module")
def ctx():
    import plass_amd
    c = plass_amd.Context(0)
    yield c
    c.close()


def check_against(out, seqs, hdrs):
    t, ent = read_db(out)
    assert t == 1 and sorted(ent) == list(range(len(seqs)))
    bad = [k for k in range(len(seqs)) if ent[k] != seqs[k] + b"\0"]
    assert not bad, "%d entries differ, first key %d:\n%r\n%r" % (len(bad), bad[0], ent[bad[0]][:300], seqs[bad[0]][:300])
    th, hent = read_db(str(out) + "_h")
    assert th == 12 and sorted(hent) == list(range(len(hdrs)))
    assert all(hent[k] == hdrs[k] + b"\0" for k in range(len(hdrs)))


def test_mergereads_cli_is_the_reference(golden, tmp_path):
    run(["mergereads", EXAMPLE[0], EXAMPLE[1], tmp_path / "r", "--threads", "4", "-v", "3"])
    assert_same_db(os.path.join(golden, "nucl", "seq_0"), tmp_path / "r", "mergereads of the example pairs")
    seqs, hdrs = mergecheck.merge_files(EXAMPLE)
    check_against(tmp_path / "r", seqs, hdrs)
    # the same bytes uncompressed, and with CRLF line ends: the same DBs
    plain, crlf = [], []
    for k, src in enumerate(EXAMPLE):
        data = gzip.open(src).read()
        plain.append(tmp_path / ("p%d.fastq" % k)); plain[-1].write_bytes(data)
        crlf.append(tmp_path / ("c%d.fq" % k)); crlf[-1].write_bytes(data.replace(b"\n", b"\r\n"))
    for tag, files in (("plain", plain), ("crlf", crlf)):
        run(["mergereads"] + files + [tmp_path / tag])
        assert_same_db(tmp_path / "r", tmp_path / tag, "mergereads, %s input" % tag)
        assert_same_db(str(tmp_path / "r") + "_h", str(tmp_path / tag) + "_h", "mergereads header DB, %s input" % tag)


def _fastq(names, seqs, quals):
    return b"".join(b"@%s\n%s\n+\n%s\n" % (n, s, q) for n, s, q in zip(names, seqs, quals))


def synthetic_pairs(n, seed=11):
    """n pairs from a gene-dense genome (plass_amd.synth) with unequal mate lengths 1..400 (most 100..160), mates over 512 bases, 'N',
    lowercase and IUPAC letters, seeded qualities, tandem repeats (ties of density and quality over many offsets) and constant-quality
    pairs (ties of quality on mismatches, the 'N' rule of generate_combined_read); mate 2's file holds three records more than mate 1's"""
    from plass_amd import synth
    rng = np.random.default_rng(seed)
    genome = synth.make_genome(rng, 400000)
    codes = synth.make_reads(rng, genome, n, read_len=160)                # inserts ~N(320, 40): Illumina-like pairs
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
    kind = rng.random(n)
    L = rng.integers(100, 161, size=(n, 2))
    s1, s2, q1, q2 = [], [], [], []
    for k in range(n):
        if kind[k] < 0.60:
            a, b = letters[2 * k, :L[k, 0]].copy(), letters[2 * k + 1, :L[k, 1]].copy()
        else:                                                          # 20..400 bases (1..14 for some), inserts 30..700
            l1, l2 = (int(x) for x in rng.integers(20, 401, size=2)) if kind[k] < 0.99 else (int(x) for x in rng.integers(1, 15, size=2))
            ins = int(rng.integers(max(l1, l2, 30), 701)); g = int(rng.integers(0, genome.size - ins))
            frag = np.frombuffer(b"ACGT", dtype=np.uint8)[genome[g:g + ins]]
            a, b = frag[:l1].copy(), mergecheck.COMP[frag[::-1][:l2]].copy()
        qa = rng.integers(35, 75, size=a.size, dtype=np.uint8); qb = rng.integers(35, 75, size=b.size, dtype=np.uint8)
        r = rng.random()
        if r < 0.02:                                                   # tandem repeats
            unit = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(rng.integers(1, 4)))
            a = np.resize(unit, a.size); b = np.resize(mergecheck.COMP[unit[::-1]], b.size)
            qa[:] = 40; qb[:] = 40
        elif r < 0.06:                                                 # constant quality: equal-quality mismatches
            qa[:] = 50; qb[:] = 50
        for x in (a, b):
            u = rng.random(x.size)
            if rng.random() < 0.10:
                x[u < 0.01] = ord("N")
            if rng.random() < 0.02:
                x[u > 0.97] += 32                                      # lowercase
            if rng.random() < 0.02:
                x[(u > 0.5) & (u < 0.505)] = np.frombuffer(b"RYKMSWBDHVU", dtype=np.uint8)[rng.integers(0, 11)]
        s1.append(a.tobytes()); s2.append(b.tobytes()); q1.append(qa.tobytes()); q2.append(qb.tobytes())
    for k in range(20):                                                # mates over 512 bases (the wave-per-pair kernel)
        g = int(rng.integers(0, genome.size - 2000)); l1 = int(rng.integers(513, 800)); l2 = int(rng.integers(300, 900)); ins = int(rng.integers(600, 1300))
        frag = np.frombuffer(b"ACGT", dtype=np.uint8)[genome[g:g + ins]]
        a = frag[:l1].copy(); b = mergecheck.COMP[frag[::-1][:l2]].copy()
        if k % 3 == 0:
            a[rng.integers(0, a.size, size=5)] = ord("N")
        s1.append(a.tobytes()); s2.append(b.tobytes())
        q1.append(rng.integers(35, 75, size=a.size, dtype=np.uint8).tobytes()); q2.append(rng.integers(35, 75, size=b.size, dtype=np.uint8).tobytes())
    m = len(s1)
    n1 = [b"pair%d/1 extra words" % k for k in range(m)]
    n2 = [b"pair%d/2\tx" % k for k in range(m)]
    s2 += [b"ACGT" * 10] * 3; q2 += [b"I" * 40] * 3; n2 += [b"extra%d" % k for k in range(3)]
    return _fastq(n1, s1, q1), _fastq(n2, s2, q2)


def test_mergereads_synthetic_against_the_checker(tmp_path):
    f1, f2 = synthetic_pairs(200000)
    p1, p2 = tmp_path / "s_1.fastq", tmp_path / "s_2.fastq.gz"
    p1.write_bytes(f1)
    with gzip.open(p2, "wb", compresslevel=1) as g:
        g.write(f2)
    seqs, hdrs, comb = mergecheck.merge_records(mergecheck.parse_fastq(f1), mergecheck.parse_fastq(f2))
    assert 0 < comb < 200020
    out = run(["mergereads", p1, p2, tmp_path / "s"], env={"PLASSHIP_MERGE_BATCH": "65536"}).stdout     # four batches
    assert "combined: %d " % comb in out, out
    check_against(tmp_path / "s", seqs, hdrs)
    # two file pairs in one call: keys continue over the second pair
    run(["mergereads", EXAMPLE[0], EXAMPLE[1], p1, p2, tmp_path / "two"], env={"PLASSHIP_MERGE_BATCH": "100000"})
    es, eh = mergecheck.merge_files(EXAMPLE)
    check_against(tmp_path / "two", es + seqs, eh + hdrs)


def test_fastq_to_fragments_on_the_device(ctx, golden, tmp_path):
    reads, hdr, st = ctx.mergereads(EXAMPLE)
    assert (st.pairs, st.combined, st.not_combined) == (5000, 4277, 723)
    assert reads.info()["n"] == 5723 and hdr.info()["dbtype"] == 12
    frag = ctx.plass_fragments(reads)
    frag.write(tmp_path / "aa")
    assert_same_db(os.path.join(golden, "aa", "seq_0"), tmp_path / "aa", "FASTQ -> mergereads -> fragments, all on the device")


def test_chains_from_fastq(golden, tmp_path):
    run(["assemble-chain", EXAMPLE[0], EXAMPLE[1], tmp_path / "a0", "--num-iterations", "1"])
    assert_same_db(os.path.join(golden, "fs", "assembly_0"), tmp_path / "a0", "assemble-chain from FASTQ, 1 iteration")
    s = os.path.join(golden, "nucl", "seq_0")
    run(["nuclassemble-chain", s, tmp_path / "n_db", "--num-iterations", "2"])
    run(["nuclassemble-chain", EXAMPLE[0], EXAMPLE[1], tmp_path / "n_fq", "--num-iterations", "2"])
    assert_same_db(tmp_path / "n_db", tmp_path / "n_fq", "nuclassemble-chain from FASTQ")
    run(["guidedassemble-chain", s, tmp_path / "g_db_n", tmp_path / "g_db_a", "--num-iterations", "2"])
    run(["guidedassemble-chain", EXAMPLE[0], EXAMPLE[1], tmp_path / "g_fq_n", tmp_path / "g_fq_a", "--num-iterations", "2"])
    assert_same_db(tmp_path / "g_db_n", tmp_path / "g_fq_n", "guidedassemble-chain from FASTQ, nucleotide contigs")
    assert_same_db(tmp_path / "g_db_a", tmp_path / "g_fq_a", "guidedassemble-chain from FASTQ, protein contigs")


def test_refusals_leave_nothing_behind(tmp_path):
    good = gzip.open(EXAMPLE[0]).read()
    fasta = tmp_path / "r.fasta"; fasta.write_bytes(b">r1\nACGTACGTACGTACGTACGT\n>r2\nACGTACGTACGTACGTACGT\n")
    hiq = tmp_path / "hq.fastq"; hiq.write_bytes(b"@r1\nACGTACGTACGTACGTACGT\n+\n" + b"I" * 19 + b"\xc8\n")
    multi = tmp_path / "ml.fastq"; multi.write_bytes(b"@r1\nACGTACGTAC\nGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIII\n")
    bz = tmp_path / "r.fastq.bz2"; shutil.copy(EXAMPLE[0], bz)
    ok = tmp_path / "ok.fastq"; ok.write_bytes(good)
    for k, files in enumerate(([ok, bz], ["stdin", ok], [fasta, fasta], [ok, hiq], [multi, ok])):
        out = tmp_path / ("o%d" % k)
        p = run(["mergereads"] + files + [out], ok=False)
        assert p.returncode == 95, p.stdout[-2000:]
        assert not any(x.startswith("o%d" % k) for x in os.listdir(tmp_path)), os.listdir(tmp_path)
    p = run(["assemble-chain", ok, hiq, tmp_path / "oc"], ok=False)
    assert p.returncode == 95 and not os.path.exists(tmp_path / "oc"), p.stdout[-2000:]
