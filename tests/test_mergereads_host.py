"""Host tests of the mergereads restatement (`-m "not gpu"`): tests/tools/mergecheck.py, the checker the GPU tests judge plass-hip mergereads
with, must reproduce the reference's own mergereads output — nucl/seq_0 of example_nucl.tar.gz is `nucl_reads` of `penguin nuclassemble` on
the bundled example pairs (tests/golden/make_golden.sh, make_example_reads.sh) — byte for byte before it judges anything else.  And the
drop-in wrapper routes `mergereads` to plass-hip."""
import os
import subprocess
import sys

import numpy as np

from conftest import read_db

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import mergecheck  # noqa: E402

EXAMPLE = [os.path.join(ROOT, "tests", "golden", "example_reads", "reads_%d.fastq.gz" % i) for i in (1, 2)]


def test_checker_reproduces_the_reference_mergereads(golden):
    seqs, hdrs = mergecheck.merge_files(EXAMPLE)
    dbtype, ent = read_db(os.path.join(golden, "nucl", "seq_0"))
    assert dbtype == 1
    assert sorted(ent) == list(range(len(seqs))) and len(seqs) == 5723
    assert all(ent[k] == seqs[k] + b"\0" for k in range(len(seqs)))
    assert len(hdrs) == len(seqs)
    # 5 000 pairs, 723 of them left as two entries; the uncalled-base path is exercised (116 reads of mate 2 hold an 'N')
    r2 = mergecheck.read_fastq(EXAMPLE[1])
    assert len(r2) == 5000 and sum(b"N" in s for _, s, _ in r2) == 116


def test_checker_semantics_by_hand():
    # the complement of lib/flash/read.cpp: IUPAC and lowercase complemented, U -> A, anything else '.'
    assert mergecheck.revcomp(b"ACGTN") == b"NACGT"
    assert mergecheck.revcomp(b"ux.Rk") == b"mY..a"
    assert mergecheck.revcomp(b"RYKMSWBDHV") == b"BDHVWSKMRY"
    assert mergecheck.revcomp(b"U") == b"A" and mergecheck.revcomp(b"x") == b"." and mergecheck.revcomp(b"r") == b"y"
    # a perfect 20-base overlap merges; the mismatch decided by quality, then mate 2 on equal quality unless it is 'N'
    a = b"AAAAACCCCCGGGGGTTTTTACGTAACCGGTTA"
    b_rc = a[13:] + b"GATTACA"
    q = b"I" * len(a)
    seqs, _, comb = mergecheck.merge_records([(b"x", a, q)], [(b"y", mergecheck.revcomp(b_rc), (b"I" * len(b_rc))[::-1])])
    assert comb == 1 and seqs[0] == a + b"GATTACA\n"
    mut = bytearray(b_rc); mut[3] = ord("N")
    seqs, _, comb = mergecheck.merge_records([(b"x", a, q)], [(b"y", mergecheck.revcomp(bytes(mut)), b"I" * len(b_rc))])
    assert comb == 1 and seqs[0] == a + b"GATTACA\n"
    # too short to overlap (< 15 bases): never merged, mate 2 written reverse-complemented
    seqs, hdrs, comb = mergecheck.merge_records([(b"x", b"ACGTACGTAC", b"IIIIIIIIII")], [(b"y", b"GGGAAA", b"IIIIII")])
    assert comb == 0 and seqs == [b"ACGTACGTAC\n", b"TTTCCC\n"] and hdrs == [b"x\n", b"y\n"]


def test_checker_ties_take_the_first_offset():
    # a tandem repeat overlaps without mismatches at every offset: (density 0, qual 0) everywhere, the first offset wins
    a = b"AC" * 30
    seqs, _, comb = mergecheck.merge_records([(b"x", a, b"I" * 60)], [(b"y", mergecheck.revcomp(b"AC" * 40), b"I" * 80)])
    assert comb == 1 and seqs[0] == b"AC" * 40 + b"\n"           # offset 0: mate 2 covers mate 1 completely (start = max(0, L1 - L2) = 0)


def test_wrapper_routes_mergereads_to_plass_hip(tmp_path):
    hip = os.path.join(ROOT, "plass_amd", "plass-hip")
    assert os.path.exists(hip), "build() makes plass_amd/plass-hip"
    log = tmp_path / "wrapper.log"
    env = dict(os.environ, PLASSHIP_CLI_DRYRUN="1", PLASS_REF_BIN="/bin/true", PLASS_WRAPPER_LOG=str(log))
    p = subprocess.run([os.path.join(ROOT, "plass_amd", "plass-gpu-wrapper"), "mergereads", EXAMPLE[0], EXAMPLE[1], str(tmp_path / "nucl_reads"),
                        "--threads", "4", "-v", "3"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    text = log.read_text()
    assert "GPU path   (dry run: accepted" in text and "mergereads" in text, text
    assert not os.path.exists(tmp_path / "nucl_reads")
    # stdin and bzip2 are handed to the reference by name, before anything is read
    for args in (["stdin", "stdin"], [str(tmp_path / "a.fastq.bz2"), str(tmp_path / "b.fastq.bz2")]):
        q = subprocess.run([hip, "mergereads"] + args + [str(tmp_path / "o")], env=dict(os.environ, PLASSHIP_CLI_DRYRUN="1"),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert q.returncode == 95, q.stdout
    np.testing.assert_equal(os.path.exists(tmp_path / "o"), False)
