"""plasship_rescore_local on the GPU: `rescorediagonal --rescore-mode 2` on hand-made pairs at every edge of the kernel
(tests/tools/local_cases.py: the lane's 16 residues, the step's 1024, ties, wraps, strands, every gate on its threshold), byte for byte
against the Python restatement (tests/tools/local_check.py, itself pinned on the CPU oracle by tests/test_local_host.py) — through the
Python binding and through the command line — and chained on handles between kmermatcher and the greedy clustering."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, assert_same_db, read_db

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import local_cases as cs  # noqa: E402
import local_check as lc  # noqa: E402

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "plass_amd", "plass-hip")
CASES = [(db, pref, name, flags, thr) for db, pref in cs.COMBOS for name, flags, thr in cs.RUNS]


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("local"))
    cs.write_all(d)
    return d


@pytest.fixture(scope="module")
def expected(root):
    """the restatement, computed once"""
    return {(db, pref, name): cs.expected(root, db, pref, flags, thr) for db, pref, name, flags, thr in CASES}


@pytest.fixture(scope="module")
def ctx():
    import plass_amd
    with plass_amd.Context(0) as c:
        yield c


def _kwargs(flags, thr):
    par = lc.parse_flags(flags)
    return dict(min_seq_id=par["min_seq_id"], seq_id_mode=par["seq_id_mode"], cov_mode=par["cov_mode"], c=par["c"], min_aln_len=par["min_aln_len"], e=par["e"],
                a=bool(par["a"]), score_per_col_thr=thr)


def _same(got_path, want, what):
    dbtype, got = read_db(got_path)
    assert dbtype == 5 and got.keys() == want.keys(), what
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, "%s: %d entries differ, first key %d:\n%r\n%r" % (what, len(bad), bad[0], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("case", CASES, ids=["%s-%s" % (c[1], c[2]) for c in CASES])
def test_edges_through_the_binding(ctx, root, expected, tmp_path, case):
    db, pref, name, flags, thr = case
    want, recs, _ = expected[(db, pref, name)]
    sdb = ctx.read_seqdb(os.path.join(root, db))
    cands = ctx.read_prefdb(sdb, sdb, os.path.join(root, pref))
    alns, st = ctx.rescore_local(sdb, cands, **_kwargs(flags, thr))
    alns.write(str(tmp_path / "out"))
    _same(tmp_path / "out", want, "%s %s" % (pref, name))
    assert st.n_scored == sum(e.count(b"\n") for _, e in lc.read_db(os.path.join(root, pref))[0]) and st.n_accepted == len(recs) == alns.count()
    got = alns.download()
    assert [(g.query_key, g.target_key, g.raw_score, g.aln_len, g.reversed) for g in got] == [(r["query"], r["target"], r["raw_score"], r["aln_len"], r["reversed"]) for r in recs]
    for h in (alns, cands, sdb):
        h.free()


@pytest.mark.parametrize("case", [c for c in CASES if c[2] in ("linclust", "filter1")], ids=lambda c: "%s-%s" % (c[1], c[2]))
def test_edges_through_the_command_line(root, expected, tmp_path, case):
    db, pref, name, flags, thr = case
    extra = [] if thr is None else ["--score-per-col-thr", repr(thr)]
    p = subprocess.run([EXE, "rescorediagonal-local", os.path.join(root, db), os.path.join(root, db), os.path.join(root, pref), str(tmp_path / "out")] + flags.split() + extra,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    _same(tmp_path / "out", expected[(db, pref, name)][0], "%s %s" % (pref, name))


def test_equals_every_reference_db_of_the_fixture(ctx, tmp_path):
    """tests/golden/local.tar.gz: what the unmodified reference wrote with --rescore-mode 2 on the hand-made pairs; for --filter-hits 1 the
    threshold is the one the reference took from its own table (RUNS), 0 where its table has no row"""
    d = str(tmp_path / "golden")
    runs, _ = cs.unpack_fixture(d)
    assert len(runs) == 21
    handles = {}
    for name, db, pref, flags, thr in runs:
        if db not in handles:
            handles[db] = ctx.read_seqdb(os.path.join(d, db))
        sdb = handles[db]
        cands = ctx.read_prefdb(sdb, sdb, os.path.join(d, pref))
        alns, _ = ctx.rescore_local(sdb, cands, **_kwargs(flags, thr))
        alns.write(str(tmp_path / name))
        assert_same_db(tmp_path / name, os.path.join(d, "local", "ref", name, "out"), name)
        alns.free(); cands.free()
    for h in handles.values():
        h.free()


def test_chained_between_kmermatcher_and_clust_on_handles(ctx, tmp_path):
    """kmermatcher -> mode 2 -> clust-greedy on the alignment list, nothing on disk in between; the written DBs against the restatement"""
    import plass_amd
    r = random.Random(11)
    seqs = []
    for i in range(40):
        n = r.randrange(900, 2600)
        base = "".join(r.choice("ACGT") for _ in range(n))
        seqs.append(base)
        for rate, cut in ((0.004, 30), (0.06, 0)):                     # within and beyond --min-seq-id 0.97; the near copy is a little shorter
            x = list(base[cut:])
            for p in r.sample(range(len(x)), int(len(x) * rate)):
                x[p] = "ACGT"[("ACGT".index(x[p]) + 1 + r.randrange(3)) % 4]
            seqs.append("".join(x))
    r.shuffle(seqs)
    data = b"".join(s.encode() + b"\n\0" for s in seqs)
    elen = np.array([len(s) + 2 for s in seqs], dtype=np.uint32)
    off = np.concatenate([[0], np.cumsum(elen[:-1], dtype=np.uint64)]).astype(np.uint64)
    db = ctx.upload_seqdb(data, off, elen, np.arange(len(seqs), dtype=np.uint32), 1)
    cands, kst = ctx.kmermatcher(db, plass_amd.KmermatchParams(k=22, alph_size=5, kmer_per_seq=60, kmer_per_seq_scale=0.1, hash_shift=67,
                                                             include_only_extendable=False, ignore_multi_kmer=True, cov_mode=1, c=0.9))
    assert kst.n_candidates >= 40
    flags = "--rescore-mode 2 -e 0.001 --min-seq-id 0.97 -c 0.9 --cov-mode 1 --seq-id-mode 0 --min-aln-len 0 -a 0"
    alns, st = ctx.rescore_local(db, cands, **_kwargs(flags, None))
    clu, cst = ctx.clust_greedy(db, alns)
    cands.write(str(tmp_path / "pref")); alns.write(str(tmp_path / "aln")); clu.write(str(tmp_path / "clu"))
    pref_ent, pref_type = lc.read_db(str(tmp_path / "pref"))
    counts = {}
    out, recs = lc.rescore_local({k: s.encode() for k, s in enumerate(seqs)}, True, pref_ent, pref_type, lc.parse_flags(flags), counts=counts)
    _same(tmp_path / "aln", {k: e + b"\0" for k, e in out}, "chained")
    # the set is what it is meant to be: near copies kept, 6 % copies found and dropped, some on either strand
    assert pref_type == 14 and counts["hasSeqId"][0] >= 20 and counts["hasSeqId"][1] >= 5, counts
    assert st.n_accepted == len(recs)
    # the clustering of the GPU's alignment list equals the one of the DB it wrote, read back
    back = ctx.read_alndb(db, str(tmp_path / "aln"))
    clu2, _ = ctx.clust_greedy(db, back)
    clu2.write(str(tmp_path / "clu2"))
    assert_same_db(tmp_path / "clu", tmp_path / "clu2", "clustering of the list on handles and of the list read back")
    assert cst.n_clusters < len(seqs)
    for h in (clu2, back, clu, alns, cands, db):
        h.free()


def _clu_entry(rep, members):
    """an entry as Clustering::writeData lays it out: the representative's key first, the others ascending"""
    return b"".join(b"%d\n" % k for k in [rep] + sorted(m for m in members if m != rep))


# keys with gaps; (first clustering, second clustering on the subset of the first one's representatives) as {representative: members}
MERGE_KEYS = [2, 3, 7, 11, 12, 20, 31, 40, 41, 57, 90, 1000]
MERGE_CASES = {
    # 57: a singleton in both steps; 12: a second-step representative that is not the smallest key of its lists (a member in the first step's
    # order: its own list comes first, then 3's and 40's); 31: its second-step entry is there and empty; 90: no second-step entry at all
    "mixed": ({3: [3, 2, 7], 12: [12, 11, 1000], 40: [40, 20, 41], 31: [31], 57: [57], 90: [90]}, {12: [12, 3, 40], 31: [], 57: [57]}),
    "second_empty": ({3: [3, 2, 7], 12: [12, 11, 1000], 40: [40, 20, 41], 31: [31], 57: [57], 90: [90]}, {}),
    "all_into_the_largest_key": ({k: [k] for k in MERGE_KEYS}, {1000: MERGE_KEYS}),
    "singletons": ({k: [k] for k in MERGE_KEYS}, {k: [k] for k in MERGE_KEYS}),
}


@pytest.mark.parametrize("case", sorted(MERGE_CASES))
def test_merge_on_hand_made_clusterings(ctx, tmp_path, case):
    first, second = MERGE_CASES[case]
    cs.write_db(str(tmp_path / "seq"), [(k, b"ACGT" * (3 + k % 5) + b"\n") for k in MERGE_KEYS], 1)
    f = [(r, _clu_entry(r, first[r])) for r in sorted(first)]
    s = [(r, _clu_entry(r, second[r]) if second[r] else b"") for r in sorted(second)]
    cs.write_db(str(tmp_path / "clu1"), f, 6); cs.write_db(str(tmp_path / "clu2"), s, 6)
    want = lc.merge_clusters(MERGE_KEYS, f, s)
    db = ctx.read_seqdb(str(tmp_path / "seq"))
    c1, c2 = ctx.read_clusters(db, str(tmp_path / "clu1")), ctx.read_clusters(db, str(tmp_path / "clu2"))
    m = ctx.merge_clusters(db, c1, c2)
    m.write(str(tmp_path / "merged"))
    assert read_db(tmp_path / "merged") == (6, {k: e + b"\0" for k, e in want}), case
    assert m.count() == (len(MERGE_KEYS), len(want))
    rep, mem = m.download()
    assert [(int(a), int(b)) for a, b in zip(rep, mem)] == [(k, int(l)) for k, e in want for l in e.split()]
    if case == "mixed":
        assert dict(want)[12] == b"12\n11\n1000\n3\n2\n7\n40\n20\n41\n" and dict(want)[31] == b"31\n" and 3 not in dict(want)
    # through the command line
    p = subprocess.run([EXE, "mergeclusters-greedy", str(tmp_path / "seq"), str(tmp_path / "cli"), str(tmp_path / "clu1"), str(tmp_path / "clu2")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    assert_same_db(tmp_path / "merged", tmp_path / "cli", case)
    for h in (m, c2, c1, db):
        h.free()


# every decimal length of a 32-bit key and both sides of each boundary (0 and 1: the one-digit end); the fixtures' keys have at most 4 digits
EDGE_KEYS = [0, 1] + [v for d in range(1, 10) for v in (10 ** d - 1, 10 ** d)] + [4294967295]
# 1000 and 4294967295: the largest key of their members, so the representative's line moves to the front; 9999 and 10000000: the smallest; 0 and 1: singletons
EDGE_FIRST = {0: [0], 1: [1], 1000: [9, 10, 99, 100, 999, 1000], 9999: [9999, 10000, 99999, 100000], 10000000: [10000000, 99999999, 100000000, 999999999, 1000000000],
              4294967295: [999999, 1000000, 9999999, 4294967295]}
EDGE_SECOND = {9999: [9999], 4294967295: [4294967295, 1000]}       # two first-step clusters joined under the larger key


def _written_downloaded_counted(handle, path, keys, want):
    """want: [(key, entry bytes)] in key order, from the restatement"""
    handle.write(str(path))
    assert read_db(path) == (6, {k: e + b"\0" for k, e in want})
    assert handle.count() == (len(keys), len(want))
    return [(int(a), int(b)) for a, b in zip(*handle.download())]


def test_cluster_db_writers_at_every_key_length(ctx, tmp_path):
    """the one writer behind Clusters.write (representative first) and MergedClusters.write (pair order), on keys of 1 to 10 digits"""
    assert len(EDGE_KEYS) == 21 and sorted(k for m in EDGE_FIRST.values() for k in m) == EDGE_KEYS
    cs.write_db(str(tmp_path / "seq"), [(k, b"ACGT" * (1 + i % 3) + b"\n") for i, k in enumerate(EDGE_KEYS)], 1)
    f = [(r, _clu_entry(r, EDGE_FIRST[r])) for r in sorted(EDGE_FIRST)]
    s = [(r, _clu_entry(r, EDGE_SECOND[r])) for r in sorted(EDGE_SECOND)]
    assert dict(f)[1000] == b"1000\n9\n10\n99\n100\n999\n" and dict(f)[4294967295] == b"4294967295\n999999\n1000000\n9999999\n"
    cs.write_db(str(tmp_path / "clu1"), f, 6); cs.write_db(str(tmp_path / "clu2"), s, 6)
    db = ctx.read_seqdb(str(tmp_path / "seq"))
    c1, c2 = ctx.read_clusters(db, str(tmp_path / "clu1")), ctx.read_clusters(db, str(tmp_path / "clu2"))
    # a clustering's pairs ascend by (representative, member), the representative among its members
    assert _written_downloaded_counted(c1, tmp_path / "out1", EDGE_KEYS, f) == [(r, k) for r in sorted(EDGE_FIRST) for k in sorted(EDGE_FIRST[r])]
    m = ctx.merge_clusters(db, c1, c2)
    want = lc.merge_clusters(EDGE_KEYS, f, s)
    assert dict(want)[4294967295] == b"4294967295\n999999\n1000000\n9999999\n1000\n9\n10\n99\n100\n999\n" and 1000 not in dict(want)
    assert _written_downloaded_counted(m, tmp_path / "merged", EDGE_KEYS, want) == [(k, int(l)) for k, e in want for l in e.split()]
    for h in (m, c2, c1, db):
        h.free()


def test_cluster_db_writers_on_a_db_of_one_sequence(ctx, tmp_path):
    """head and tail of the only entry fall on the only pair"""
    cs.write_db(str(tmp_path / "seq"), [(0, b"ACGT\n")], 1)
    f = [(0, _clu_entry(0, [0]))]
    cs.write_db(str(tmp_path / "clu"), f, 6)
    db = ctx.read_seqdb(str(tmp_path / "seq"))
    c1, c2 = ctx.read_clusters(db, str(tmp_path / "clu")), ctx.read_clusters(db, str(tmp_path / "clu"))
    assert _written_downloaded_counted(c1, tmp_path / "out1", [0], f) == [(0, 0)]
    m = ctx.merge_clusters(db, c1, c2)
    assert lc.merge_clusters([0], f, f) == f
    assert _written_downloaded_counted(m, tmp_path / "merged", [0], f) == [(0, 0)]
    for h in (m, c2, c1, db):
        h.free()


def test_merge_equals_the_reference_on_the_fixture(ctx, tmp_path):
    d = str(tmp_path / "golden")
    _, merges = cs.unpack_fixture(d)
    merges = list(merges) + [("linclust", "local/nucl", "local/ref/linclust/pre_clust", "local/ref/linclust/clust")]
    for name, seq, first, second in merges:
        db = ctx.read_seqdb(os.path.join(d, seq))
        c1, c2 = ctx.read_clusters(db, os.path.join(d, first)), ctx.read_clusters(db, os.path.join(d, second))
        m = ctx.merge_clusters(db, c1, c2)
        m.write(str(tmp_path / name))
        want = os.path.join(d, "local", "ref", "linclust", "clu") if name == "linclust" else os.path.join(d, "local", "ref", name, "merged")
        assert_same_db(tmp_path / name, want, name)
        for h in (m, c2, c1, db):
            h.free()


def _run(*args):
    p = subprocess.run([EXE] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    return p.stdout


def test_linclust_ungapped_equals_the_reference_and_the_modules_one_by_one(tmp_path):
    """`plass-hip linclust-ungapped` on the fixture's nucleotide DB against the `clu` DB the reference's `linclust --alignment-mode 4` wrote
    with the same flags, and against the same steps as single commands with every DB on disk in between (the subset DB of pre_clust's
    representatives, which the reference makes with createsubdb, is written here)"""
    d = str(tmp_path / "golden")
    cs.unpack_fixture(d)
    ref = os.path.join(d, "local", "ref", "linclust")
    nucl = os.path.join(d, "local", "nucl")
    lin, thr = open(os.path.join(d, "local", "LINCLUST")).read().splitlines()
    lin = lin.split()
    lin = [a for i, a in enumerate(lin) if a not in ("--alignment-mode", "--remove-tmp-files") and lin[i - 1] not in ("--alignment-mode", "--remove-tmp-files")]
    _run("linclust-ungapped", nucl, tmp_path / "clu", *lin, "--score-per-col-thr", thr)
    assert_same_db(tmp_path / "clu", os.path.join(ref, "clu"), "linclust-ungapped against the reference's linclust")
    # one module after the other
    kmer = ["-k", "22", "--kmer-per-seq", "60", "--kmer-per-seq-scale", "0.1", "--alph-size", "nucl:5,aa:13", "--hash-shift", "67", "--ignore-multi-kmer", "1"]
    gates = ["--min-seq-id", "0.97", "-c", "0.9", "--cov-mode", "1", "-e", "0.001"]
    _run("linclust-pre", nucl, tmp_path / "pre_clust", tmp_path / "pref_filter2", *kmer, *gates, "--rescore-mode", "0", "--cluster-mode", "3")
    assert_same_db(tmp_path / "pre_clust", os.path.join(ref, "pre_clust"), "pre_clust")
    assert_same_db(tmp_path / "pref_filter2", os.path.join(ref, "pref_filter2"), "pref_filter2")
    seqs, _ = lc.read_seqdb(nucl)
    reps = sorted(read_db(tmp_path / "pre_clust")[1])
    cs.write_db(str(tmp_path / "sub"), [(k, seqs[k] + b"\n") for k in reps], 1)
    _run("rescorediagonal-local", tmp_path / "sub", tmp_path / "sub", tmp_path / "pref_filter2", tmp_path / "aln", *gates, "--rescore-mode", "2", "--filter-hits", "1", "--score-per-col-thr", thr)
    assert_same_db(tmp_path / "aln", os.path.join(ref, "aln"), "the alignment step against the reference's aln")
    _run("clust-greedy", tmp_path / "sub", tmp_path / "aln", tmp_path / "clust", "--cluster-mode", "3")
    assert_same_db(tmp_path / "clust", os.path.join(ref, "clust"), "clust")
    _run("mergeclusters-greedy", nucl, tmp_path / "clu_steps", tmp_path / "pre_clust", tmp_path / "clust")
    assert_same_db(tmp_path / "clu_steps", tmp_path / "clu", "module by module against the driver")


def test_sharded_context_is_unsupported(root):
    import plass_amd
    from plass_amd.shard import LocalGroup
    ctxs = [plass_amd.Context(0) for _ in range(2)]

    def work(rank, c):
        sdb = c.read_seqdb(os.path.join(root, "prot"))
        cands = c.read_prefdb(sdb, sdb, os.path.join(root, "pref_prot7"))
        try:
            c.rescore_local(sdb, cands)
            return "no error"
        except plass_amd.PlasshipError as e:
            return str(e)
        finally:
            cands.free(); sdb.free()

    try:
        msgs = LocalGroup(2).run(work, ctxs)
    finally:
        for c in ctxs:
            c.close()
    assert len(msgs) == 2 and all("(-4)" in m and "sharded" in m for m in msgs), msgs
