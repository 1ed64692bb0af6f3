"""Host tests of the mergereads ladder (`-m "not gpu"`): the hand-made pairs of tests/tools/merge_ladder.py, judged by the reference's own
FLASH (tests/golden/mergereads_ladder.tar.gz, written by make_mergereads_ladder.sh with oracle/tools/flash_pin.cpp), pin the checker
tests/tools/mergecheck.py beyond the example pairs: per rung it must reproduce the fixture byte for byte.  And every pair must be where it
was meant to be: its reach conditions are asserted on the checker's own intermediate values (align_pairs' trace), so a rung that names the
threshold sits on it, a tie rung has its equal keys at the stated distance, a mask rung is decided by the one designed mismatch.

Rules the checker had misread: none; it reproduces all 14 rungs (296 pairs) as first written."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import merge_ladder as L  # noqa: E402
import mergecheck  # noqa: E402

NAMES = [r[0] for r in L._RUNGS]


@pytest.fixture(scope="module")
def fixture():
    return L.fixture()


def test_fixture_holds_the_ladder_as_built(fixture):
    """the committed FASTQ files are what the seeded builder writes today, rung by rung and in order"""
    assert list(fixture) == NAMES == list(L.rungs())
    for name, r in L.rungs().items():
        assert r.fastq() == fixture[name][:2], name
        assert r.purpose and r.pairs and all(p.reach for p in r.pairs), name
    assert sum(len(r.pairs) for r in L.rungs().values()) == 296


@pytest.mark.parametrize("name", NAMES)
def test_checker_reproduces_flash_and_the_rung_reaches_its_edge(fixture, name):
    f1, f2, exp = fixture[name]
    want_seqs, want_hdrs, want_comb = L.expected_dbs(f1, f2, exp)
    trace = []
    seqs, hdrs, comb = mergecheck.merge_records(mergecheck.parse_fastq(f1), mergecheck.parse_fastq(f2), trace)
    pairs = L.rungs()[name].pairs
    # pair by pair first, so that a difference names its pair
    k = 0
    for p, (st, ent) in zip(pairs, exp):
        n = 1 if st else 2
        assert seqs[k:k + n] == ent, "%s: the checker and FLASH differ on %s" % (name, p.name.decode())
        k += n
    assert (seqs, hdrs, comb) == (want_seqs, want_hdrs, want_comb)
    for p, T, (st, _) in zip(pairs, trace, exp):
        T["pos"] = T["bp"] if T["bd"] <= mergecheck.MAX_DENSITY else -1
        assert (T["pos"] >= 0) == bool(st)
        for text, ok in p.reach:
            assert ok(T), "%s: %s" % (p.name.decode(), text)


def test_trace_leaves_align_pairs_as_it_was():
    f1, f2, _ = L.fixture()["ties_keys"]
    r1, r2 = mergecheck.parse_fastq(f1), mergecheck.parse_fastq(f2)
    assert mergecheck.merge_records(r1, r2) == mergecheck.merge_records(r1, r2, [])


def test_mask_rungs_flip_on_the_named_mismatch(fixture):
    """in the mask rung the pair with all three mismatches is rejected and each pair with one of them left out is accepted (20-23), the
    pair with three is accepted and the one with a fourth rejected (30-33): FLASH's own statuses, pair names taken from the builder"""
    st = {p.name.decode().split(".", 2)[2]: s for p, (s, _) in zip(L.rungs()["mask"].pairs, fixture["mask"][2])}
    for a in range(4):
        for ov in (20, 21, 22, 23):
            assert st["i%d_ov%d_all" % (a, ov)] == 0 and all(st["i%d_ov%d_no_%s" % (a, ov, w)] == 1 for w in ("first", "middle", "last"))
        for ov in (30, 31, 32, 33):
            assert st["i%d_ov%d_three" % (a, ov)] == 1 and st["i%d_ov%d_four" % (a, ov)] == 0
