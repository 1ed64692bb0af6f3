"""compactCsr (plass_amd/csrc/scan.hip) on the GPU, through the public calls that end in it: the kept lines of a Hamming rescore (16-byte
records), the download and the DB file of a sparse alignment list (64-byte records) and plasship_cands_filter, on hand-made lists whose
keep pattern is planted (tests/tools/csr_compact_cases.py; tests/test_csr_compact_host.py validates them on the CPU).  The expected output
is the planted pattern applied to the input list, compared exactly."""
import os
import sys

import pytest

from conftest import ROOT, read_db

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import clust_check as cc  # noqa: E402
import csr_compact_cases as cs  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import plass_amd
    with plass_amd.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def seqdb(ctx, tmp_path_factory):
    path = cs.write_seqdb(tmp_path_factory.mktemp("csr") / "seq")
    db = ctx.read_seqdb(path)
    yield path, db
    db.free()


@pytest.mark.parametrize("case", cs.CASES, ids=cs.CASE_IDS)
def test_kept_lines_of_the_hamming_rescore(ctx, seqdb, tmp_path, case):
    pref, kept = cs.case(*case)
    db = seqdb[1]
    cands = ctx.read_prefdb(db, db, cs.write_pref(tmp_path / "pref", pref))
    out, st = ctx.rescore_hamming(db, db, cands, wrapped=False, min_seq_id=1.0)
    n_kept = sum(len(v) for v in kept.values())
    assert (st.n_scored, st.n_accepted) == (case[1], n_kept)
    # the records, in input order ...
    q, t, s, d = out.download()
    assert list(zip(q.tolist(), t.tolist())) == [(k, x) for k in sorted(kept) for x in kept[k]]
    assert out.count() == n_kept and (s == 100).all() and (d == 0).all()
    # ... and the CSR over them: the DB file has every query's lines under its key
    out.write(str(tmp_path / "out"))
    dbtype, got = read_db(tmp_path / "out")
    assert dbtype == 7 and got == {k: b"".join(b"%d\t100\t0\n" % x for x in ts) + b"\0" for k, ts in kept.items()}
    out.free(); cands.free()


@pytest.mark.parametrize("case", cs.CASES, ids=cs.CASE_IDS)
def test_dense_copy_of_a_sparse_alignment_list(ctx, seqdb, tmp_path, case):
    pref, kept = cs.case(*case)
    db = seqdb[1]
    cands = ctx.read_prefdb(db, db, cs.write_pref(tmp_path / "pref", pref))
    alns, st = ctx.rescorediagonal(db, db, cands)                                  # the default parameters; the list is sparse
    n_kept = sum(len(v) for v in kept.values())
    assert (st.n_scored, st.n_accepted, alns.count()) == (case[1], n_kept, n_kept)
    recs = alns.download()
    assert [(r.query_key, r.target_key) for r in recs] == [(k, x) for k in sorted(kept) for x in kept[k]]
    # every kept pair is 32 of 32 columns on diagonal 0: the other 56 bytes of every record are the same
    rest = {(r.bit_score, r.raw_score, r.seq_id, r.q_start, r.q_end, r.q_len, r.db_start, r.db_end, r.db_len, r.aln_len, r.reversed) for r in recs}
    assert len(rest) <= 1 and all(x[1:] == (64, 1.0, 0, 31, 32, 0, 31, 32, 32, 0) for x in rest), rest
    alns.write(str(tmp_path / "aln"))
    dbtype, got = read_db(tmp_path / "aln")
    assert dbtype == 5 and {k: cs.first_columns(e) for k, e in got.items()} == kept
    alns.free(); cands.free()


def test_cands_filter_across_the_scan_tile(ctx, seqdb, tmp_path):
    """2049 lines through plasship_cands_filter: index i joins the cluster of i - 1 where i % 3 == 1, so a third of the sequences are no
    representatives, and the lines of their entries and the lines that name them go"""
    path, db = seqdb
    pref, _ = cs.case("spread", cs.SCAN_TILE + 1, "all")
    edges = {cs.key(i): (b"%d\t90\t0\n" % cs.key(i + 1) if i % 3 == 0 else b"") + b"\0" for i in range(cs.N)}
    cs.write_pref(tmp_path / "pref", pref); cs.write_pref(tmp_path / "edges", edges)
    reps = [k for k, _ in cc.cluster_entries(cc.greedy_low_mem(cc.read_index(path), cc.read_db(str(tmp_path / "edges"))[0]))]
    assert len(reps) == cs.N - cs.N // 3
    expect = dict(cc.subset_rule(cc.read_db(str(tmp_path / "pref"))[0], reps))
    n_in, n_out = sum(e.count(b"\n") for e in pref.values()), sum(e.count(b"\n") for e in expect.values())
    assert n_in == cs.SCAN_TILE + 1 and 0 < n_out < n_in - 500
    cands = ctx.read_prefdb(db, db, str(tmp_path / "pref"))
    edge_list = ctx.read_prefdb(db, db, str(tmp_path / "edges"))
    clu, _ = ctx.clust_greedy(db, edge_list)
    sub = ctx.filter_cands(cands, clu)
    sub.write(str(tmp_path / "pref_filter2"))
    dbtype, got = read_db(tmp_path / "pref_filter2")
    assert dbtype == 7 and got == {k: e + b"\0" for k, e in expect.items()}
    for h in (sub, clu, edge_list, cands):
        h.free()
