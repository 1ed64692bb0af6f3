"""The inputs of tests/test_gpu_csr_compact.py, validated without a GPU: on the same files the CPU statements of both rescore modes keep
exactly the planted pattern.  Mode 3 is the CPU oracle's rescorediagonal (oracle/); the oracle has no Hamming score, so mode 0 is the
Python restatement tests/tools/hamming_check.py, which tests/test_hamming_host.py pins on the reference's own output."""
import os
import sys

import pytest

from conftest import ROOT, read_db, run_oracle

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import csr_compact_cases as cs  # noqa: E402
import hamming_check as hc  # noqa: E402


@pytest.fixture(scope="module")
def seqdb(tmp_path_factory):
    return cs.write_seqdb(tmp_path_factory.mktemp("csr") / "seq")


@pytest.mark.parametrize("case", cs.CASES, ids=cs.CASE_IDS)
def test_oracle_keeps_the_planted_lines_in_mode_3(oracle_bin, seqdb, tmp_path, case):
    pref, kept = cs.case(*case)
    cs.write_pref(tmp_path / "pref", pref)
    run_oracle(oracle_bin, ["rescorediagonal", seqdb, seqdb, tmp_path / "pref", tmp_path / "aln"])          # the default flags
    dbtype, got = read_db(tmp_path / "aln")
    assert dbtype == 5 and got.keys() == kept.keys()
    assert {k: cs.first_columns(e) for k, e in got.items()} == kept
    # every kept line is 32 of 32 columns on diagonal 0
    lines = {l.split(b"\t", 1)[1] for e in got.values() for l in e.rstrip(b"\0").split(b"\n") if l}
    assert len(lines) <= 1 and all(l.split(b"\t")[1:] == [b"1.00", l.split(b"\t")[2], b"0", b"31", b"32", b"0", b"31", b"32"] for l in lines), lines


@pytest.mark.parametrize("case", cs.CASES, ids=cs.CASE_IDS)
def test_restatement_keeps_the_planted_lines_in_mode_0(case):
    pref, kept = cs.case(*case)
    got = dict(hc.rescore_hamming(cs.seqs(), True, [(k, e.rstrip(b"\0")) for k, e in sorted(pref.items())], 7, cs.HAMMING_PAR))
    assert got.keys() == kept.keys()
    assert got == {k: b"".join(b"%d\t100\t0\n" % t for t in ts) for k, ts in kept.items()}


def test_the_cases_are_the_shapes_around_the_scan_tile():
    totals = {(lay, total) for lay, total, _ in cs.CASES}
    assert totals == {("spread", t) for t in (0, 1, 2047, 2048, 2049)} | {("single", 2049)} and cs.SCAN_TILE == 2048
    for lay, total, pattern in cs.CASES:
        holders = cs.layout(lay, total)
        assert sum(n for _, n in holders) == total
        if total > 1:        # queries without lines in front of, between and behind the queries that hold some
            assert holders[0][0] > 0 and holders[-1][0] < cs.N - 1 and (lay == "single" or holders[1][0] - holders[0][0] > 1)
    assert {p for _, t, p in cs.CASES if t == 2049} == set(cs.PATTERNS)
