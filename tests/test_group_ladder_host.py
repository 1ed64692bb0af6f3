"""Host tests (`-m "not gpu"`) of the group ladder (tests/tools/group_ladder.py): what the oracle's output alone must show before
tests/test_gpu_group_ladder.py compares a GPU result with it.  Every rung sequence takes part in a candidate line, the record and key counts
of every DB are the ones the rung is named after (the oracle's N_k, and the keys restated on the host), the head of each hand-made run of rung
D is the one the restated rule names, and in rung E the oracle's N_m moves between the flag values by exactly the hand-placed members."""
import os
import sys

import pytest

from conftest import ROOT, run_oracle

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import group_ladder as G  # noqa: E402


def _oracle(oracle_bin, tmp_path, db, **flags):
    seq = db.write(tmp_path / "seq")
    log = run_oracle(oracle_bin, ["kmermatcher", seq, tmp_path / "pref"] + G.oracle_flags(**flags))
    return G.read_pref(tmp_path / "pref"), G.oracle_counts(log)


@pytest.mark.parametrize("shape", ["narrow", "wide"])
def test_size_rung(oracle_bin, tmp_path, shape):
    C = G.REG_CAP[shape]
    steps = G.size_steps(C)
    pos = [(r + G.RPL - 1) // G.RPL * G.RPL for r in steps]
    assert any(C - 64 < p <= C for p in pos) and any(C < p <= C + 64 for p in pos) and any(abs(p - 3 * C) < 64 for p in pos)
    for r in steps:
        db = G.size_db(r)
        assert db.records == r and db.distinct <= G.MAX_KEYS[shape]          # no retry in this rung
        pref, (nk, nm, nc) = _oracle(oracle_bin, tmp_path, db)
        assert nk == r and nm == int(db.rung.sum()) + sum(len(s) >= G.K for s, g in zip(db.seqs, db.rung) if g)
        G.check_rungs_connected(db, pref)


@pytest.mark.parametrize("kernel", sorted(G.MAX_KEYS))
def test_distinct_rung(oracle_bin, tmp_path, kernel):
    M = G.MAX_KEYS[kernel]
    for d in G.distinct_steps(M):
        db = G.distinct_db(d)
        assert db.distinct == d and db.records == 2 * d and db.rung.all()
        pref, (nk, nm, nc) = _oracle(oracle_bin, tmp_path, db)
        assert (nk, nm) == (2 * d, 2 * d) and nc == len(db.seqs) // 2
        G.check_rungs_connected(db, pref)
    assert [G.replay_sub_passes(G.distinct_db(d).keys, M) for d in (M - 1, M, M + 1)] == [1, 1, 2]
    assert G.replay_sub_passes(G.distinct_db(2 * M + 1).keys, M) >= 4 and G.replay_sub_passes(G.distinct_db(6 * M).keys, M) >= 8
    # nucleotide: the same key counts on both strands, no (rep, target, diagonal) triple with both strands (the oracle names such ties)
    for d in G.distinct_steps(M):
        db = G.nucl_distinct_db(d)
        assert db.distinct == d and db.rung.all()
        seq = db.write(tmp_path / "nseq")
        log = run_oracle(oracle_bin, ["kmermatcher", seq, tmp_path / "npref"] + G.oracle_flags(nucl=True))
        assert "hold both strands" not in log
        nk, nm, nc = G.oracle_counts(log)
        assert nk == nm == db.records
        lines = G.read_pref_lines(tmp_path / "npref")
        G.check_rungs_connected(db, lines)
        assert any(sc < 0 for t in lines.values() for sc, _ in t.values()) and any(sc > 0 for t in lines.values() for sc, _ in t.values())
    assert [G.replay_sub_passes(G.nucl_distinct_db(d).keys, M) for d in (M - 1, M, M + 1)] == [1, 1, 2]
    if kernel == "long":
        return
    # the same key counts in a bucket that still fits the registers: records = C, the keys beyond records - distinct occur once
    for d in (M - 1, M, M + 1):
        db = G.distinct_db(d, G.REG_CAP[kernel])
        assert db.distinct == d and db.records == G.REG_CAP[kernel] and db.rung.sum() >= 2 * (G.REG_CAP[kernel] - d) // 2
        pref, (nk, nm, nc) = _oracle(oracle_bin, tmp_path, db)
        assert nk == db.records and nm == 2 * (db.records - d)
        G.check_rungs_connected(db, pref)


def test_neighbour_rung(oracle_bin, tmp_path):
    db = G.neighbours_db()
    assert db.records == 2 * len(db.seqs) and 80000 < db.records < 150000
    pref, (nk, nm, nc) = _oracle(oracle_bin, tmp_path, db)
    assert nk == db.records and nm == db.records
    G.check_rungs_connected(db, pref)
    occ = {G.bucket_of(k, G.C_BITS) for k in db.keys}
    hot = [G.bucket_of(G.kmer_index(h), G.C_BITS) for h in db.hot]
    assert any(b % G.C_BPB == 0 and b + 1 in occ for b in hot) and any(b % G.C_BPB == 1 and b - 1 in occ and b + 1 in occ for b in hot)
    empty = set(range(1 << G.C_BITS)) - occ
    assert any(b % G.C_BPB and b - 1 in empty for b in empty) and any(b % G.C_BPB and b - 1 in empty for b in occ) and any(b % G.C_BPB and b - 1 in occ for b in empty)


def test_head_word_rung(oracle_bin, tmp_path):
    db = G.head_word_db()
    assert max(len(s) for s in db.seqs) == G.LAYOUT16_MAX_L == 32767 - 2 - 1          # SHRT_MAX > entry length = L + 2
    assert G.head_rule(db.runs["tie"])[0] == 70001 and G.head_rule(db.runs["longer"])[0] == 131200 and G.head_rule(db.runs["twice"]) == (300, 70, 5)
    assert G.head_rule(db.runs["last"]) == (66000, G.LAYOUT16_MAX_L, G.LAYOUT16_MAX_L - G.K)
    pref, (nk, nm, nc) = _oracle(oracle_bin, tmp_path, db, multi=0)
    assert nk < 150000
    G.check_rungs_connected(db, pref)
    G.check_heads(db, pref)
    assert pref[66000][5] == 32750 and pref[300][400] == -5


def test_filter_rung(oracle_bin, tmp_path):
    db = G.filter_db()
    nm = {}
    for f in G.FILTER_FLAGS:
        pref, (nk, nm_f, nc) = _oracle(oracle_bin, tmp_path, db, **f)
        assert nk == db.records
        assert nm_f == G.expected_grouped(db, f["ext"], f["c"], f["cov_mode"]), f
        nm[(f["ext"], f["c"], f["cov_mode"])] = nm_f
        if not f["ext"] and f["c"] == 0.0:
            G.check_rungs_connected(db, pref); G.check_heads(db, pref)
    # --include-only-extendable: of 16 records the two members on diagonals 21 and -1 stay; the heads and the members on 20 and 0 go
    assert nm[(0, 0.0, 0)] == 16 and nm[(1, 0.0, 0)] == 2
    # coverage: 48 / 60 = 0.8 and 54 / 60 = 0.9 pass `>=` in single precision, 47 and 53 do not; mode 1 tests query / target only
    assert nm[(0, 0.8, 0)] == 16 - 5 and nm[(0, 0.9, 1)] == 16 and nm[(0, 0.9, 2)] == 16 - 7


def test_nucl_head_rung(oracle_bin, tmp_path):
    """rung D, nucleotide: a head on each strand against a member on each strand, and the call's first run with two members"""
    db = G.nucl_head_db()
    assert {(ms[0][3], m[3]) for ms in db.runs.values() for m in ms[1:]} == {(True, True), (True, False), (False, True), (False, False)}
    first = db.runs["first"]
    assert len(first) == 3 and not first[0][3] and min(db.keys) == (1 | G.BIT63)
    # run 0 keeps repIsReverse = false: the forward member is NOT reversed, which an ordinary run with a reverse head would do
    assert G.nucl_line(first[0], first[1], True)[0] == 1 and G.nucl_line(first[0], first[1], False)[0] == -1
    seq = db.write(tmp_path / "seq")
    log = run_oracle(oracle_bin, ["kmermatcher", seq, tmp_path / "pref"] + G.oracle_flags(nucl=True))
    assert "hold both strands" not in log and G.oracle_counts(log)[0] == db.records
    lines = G.read_pref_lines(tmp_path / "pref")
    G.check_rungs_connected(db, lines)
    G.check_nucl_heads(db, lines)
