"""The hash partition of the k-mer records (linePartKernel, KEY_HASH) at its edges (run with `-m gpu` on an MI355X).

A protein sequence of 13 residues owns exactly one record slot, its identity record (tests/tools/group_ladder.py), so a DB of such
sequences in id order IS the partition's input, record for record, and identical sequences share the record's key and with it the bucket.
PLASSHIP_TUNE_PART_BITS fixes the bucket bits whatever the size: 10 bits = one level of 1024 buckets (the dense-input kernel, 1024
threads x 2 records = tiles of 2048), 20 bits = two levels of 1024 (the line-list kernel, tiles of 4096, one piece per level-1 bucket),
3 bits = 8 buckets (the 512-thread kernel, tiles of 2048).  Every case is one kmermatcher call whose candidate DB equals the CPU oracle's
byte for byte with N_k / N_m / N_c equal; before that the case states on the host, from the restated hash, that its DB has the edge it is
named for:
  a bucket of exactly one full line (8 copies of a sequence, nothing else in the bucket), one of a line and one record (9 copies), a
  bucket without records; a run of hot copies longer than a tile at the start of the input, so that the first tile's records all fall
  into one bucket (every lane ranks on one counter and the tile closes 256 / 512 lines of one bucket, round after round); record counts of
  one tile - 1, a tile, a tile + 1, odd counts (no multiple of the records per lane) and an input of 117 records, less than a tile.
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, assert_same_db, run_oracle

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import group_ladder as G  # noqa: E402

pytestmark = pytest.mark.gpu

VARS = ("PLASSHIP_TUNE_PART_BITS", "PLASSHIP_TUNE_GROUP_SHAPE", "PLASSHIP_DEBUG_GROUPHIST", "PLASSHIP_TUNE_FORCE_LONG")
FULL, OVER = G.RPL, G.RPL + 1


@pytest.fixture(autouse=True)
def _clear(monkeypatch):
    for v in VARS:
        monkeypatch.delenv(v, raising=False)


@pytest.fixture(scope="module")
def ctx():
    import plass_amd
    c = plass_amd.Context(0)
    yield c
    c.close()


def edge_db(bits, records, hot=0, seed=1):
    """`hot` copies of one sequence first, then 8 copies of a second and 9 of a third, then distinct sequences up to `records`; none of the
    distinct ones shares a final bucket (of `bits` bits) with the three, and one more bucket is kept free of records"""
    rng = np.random.default_rng(seed); taken = set()
    words = iter(G._words(rng, 4 * records + 64, G.K - 1, taken))
    special, used = [], set()
    while len(special) < 4:                                  # hot, full, over, and a word whose bucket stays empty
        w = next(words); b = G.bucket_of(G.identity_key(w), bits)
        if b not in used:
            used.add(b); special.append(w)
    seqs = [special[0]] * hot + [special[1]] * FULL + [special[2]] * OVER
    assert len(seqs) <= records
    while len(seqs) < records:
        w = next(words)
        if G.bucket_of(G.identity_key(w), bits) not in used:
            seqs.append(w)
    db = G.GroupDb(seqs, [False] * len(seqs))
    assert db.records == records
    per = {}
    for key in db.keys:
        b = G.bucket_of(key, bits); per[b] = per.get(b, 0) + 1
    bk = [G.bucket_of(G.identity_key(w), bits) for w in special]
    assert per.get(bk[0], 0) == hot and per[bk[1]] == FULL and per[bk[2]] == OVER and bk[3] not in per, "the DB misses its edges"
    if hot:
        assert len({G.bucket_of(key, bits) for key in db.keys[:hot]}) == 1
    return db


def _run(ctx, oracle_bin, tmp_path, monkeypatch, capfd, db, bits):
    import plass_amd
    seq = db.write(tmp_path / "seq")
    log = run_oracle(oracle_bin, ["kmermatcher", seq, str(tmp_path / "o_pref")] + G.oracle_flags())
    monkeypatch.setenv("PLASSHIP_TUNE_PART_BITS", str(bits))
    monkeypatch.setenv("PLASSHIP_DEBUG_GROUPHIST", "1")
    sdb = ctx.read_seqdb(seq)
    capfd.readouterr()
    cands, kst = ctx.kmermatcher(sdb, plass_amd.KmermatchParams(**G.param_kwargs()))
    err = capfd.readouterr().err
    cands.write(tmp_path / "g_pref")
    cands.free()
    got, want = (int(kst.n_kmer_records), int(kst.n_grouped), int(kst.n_candidates)), G.oracle_counts(log)
    print("bits %d, %d records: GPU (N_k, N_m, N_c) = %r, oracle %r" % (bits, db.records, got, want))
    assert_same_db(str(tmp_path / "o_pref"), tmp_path / "g_pref", "partition edges, %d bits, %d records" % (bits, db.records))
    assert got == want and want[0] == db.records
    assert kst.record_bytes == 16
    hist = G.group_hist(err)
    assert hist and hist[-1]["buckets"] == 1 << bits and hist[-1]["records"] == db.records, err


# one tile of the dense-input kernel (2048) and of the line-list kernel (4096) on both sides, odd counts, and less than a tile
@pytest.mark.parametrize("records", [117, 2047, 2048, 2049, 4095, 4096, 4097, 6151])
def test_counts_one_level(ctx, oracle_bin, tmp_path, monkeypatch, capfd, records):
    _run(ctx, oracle_bin, tmp_path, monkeypatch, capfd, edge_db(10, records, seed=records), 10)


@pytest.mark.parametrize("bits,hot,records", [(10, 2057, 3083), (10, 4105, 5122), (20, 4105, 5122), (3, 2057, 2583), (3, 0, 117), (20, 0, 117)])
def test_one_bucket_tile(ctx, oracle_bin, tmp_path, monkeypatch, capfd, bits, hot, records):
    """a tile (and a line more) of records of ONE bucket at the start of the input, in every kernel shape; the two small inputs take the
    512-thread kernel and the two-level path below one tile"""
    _run(ctx, oracle_bin, tmp_path, monkeypatch, capfd, edge_db(bits, records, hot=hot, seed=bits * 100000 + records), bits)
