"""plasship_clust_greedy_* and plasship_cands_filter on the GPU: `clust --cluster-mode 2 | 3` and linclust's createsubdb / filterdb subset,
against the DBs the unmodified reference wrote (tests/golden/clust.tar.gz, a reference pin) — through the command line and through the Python
binding — and, on generated graphs and chained behind kmermatcher and the Hamming rescore on handles, against the sequential Python
restatement (tests/tools/clust_check.py, itself pinned on the reference by tests/test_clust_host.py)."""
import os
import random
import struct
import subprocess
import sys
import tarfile

import numpy as np
import pytest

from conftest import ROOT, assert_same_db, read_db

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import clust_check as cc  # noqa: E402

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "plass_amd", "plass-hip")
with tarfile.open(os.path.join(ROOT, "tests", "golden", "clust.tar.gz")) as _t:
    RUNS = [l.split("\t") for l in _t.extractfile("clust/RUNS").read().decode().splitlines()]
    SUBSETS = [l.split("\t") for l in _t.extractfile("clust/SUBSETS").read().decode().splitlines()]


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return cc.extract_fixtures(tmp_path_factory.mktemp("clust"))


@pytest.fixture(scope="module")
def ctx():
    import plass_amd
    with plass_amd.Context(0) as c:
        yield c


def _same_files(ref, got, what):
    """the data file and the index byte for byte: one writer thread wrote the reference's"""
    for sfx in ("", ".index", ".dbtype"):
        assert open(str(ref) + sfx, "rb").read() == open(str(got) + sfx, "rb").read(), "%s: %s differs" % (what, sfx or "data file")


def _read_result(ctx, sdb, path):
    dbtype = cc.read_db(path)[1]
    return ctx.read_alndb(sdb, path) if dbtype == 5 else ctx.read_prefdb(sdb, sdb, path)


@pytest.mark.parametrize("run", RUNS, ids=[r[0] for r in RUNS])
def test_fixture_through_the_command_line(root, tmp_path, run):
    name, db, res, flags = run
    p = subprocess.run([EXE, "clust-greedy", os.path.join(root, db), os.path.join(root, res), str(tmp_path / "out")] + flags.split(),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    ref = os.path.join(root, "clust", "ref", name, "out")
    assert_same_db(ref, tmp_path / "out", name)
    _same_files(ref, tmp_path / "out", name)


def test_fixture_through_the_binding(ctx, root, tmp_path):
    for name, db, res, flags in RUNS:
        sdb = ctx.read_seqdb(os.path.join(root, db))
        lst = _read_result(ctx, sdb, os.path.join(root, res))
        clu, st = ctx.clust_greedy(sdb, lst)
        clu.write(str(tmp_path / name))
        ref = os.path.join(root, "clust", "ref", name, "out")
        _same_files(ref, tmp_path / name, name)
        rep, mem = clu.download()
        pairs = cc.greedy_low_mem(cc.read_index(os.path.join(root, db)), cc.read_db(os.path.join(root, res))[0])
        assert list(zip(rep.tolist(), mem.tolist())) == pairs, name
        assert clu.count() == (len(pairs), len(cc.read_db(ref)[0])) and st.n_clusters == clu.count()[1] and st.n_sequences == len(pairs), name
        for h in (clu, lst, sdb):
            h.free()


@pytest.mark.parametrize("sub", SUBSETS, ids=[s[0] for s in SUBSETS])
def test_subset_of_the_fixture(ctx, root, tmp_path, sub):
    """pre_clust and pref_filter2 of linclust.sh:33-56 from the fixture's pref and rescored DBs, on handles"""
    name, db, pref, clu_run = sub
    res = next(r[2] for r in RUNS if r[0] == clu_run)
    sdb = ctx.read_seqdb(os.path.join(root, db))
    cands = ctx.read_prefdb(sdb, sdb, os.path.join(root, pref))
    rescored = _read_result(ctx, sdb, os.path.join(root, res))
    clu, _ = ctx.clust_greedy(sdb, rescored)
    kept = ctx.filter_cands(cands, clu)
    clu.write(str(tmp_path / "pre_clust")); kept.write(str(tmp_path / "pref_filter2"))
    _same_files(os.path.join(root, "clust", "ref", clu_run, "out"), tmp_path / "pre_clust", name)
    assert_same_db(os.path.join(root, "clust", "ref", name, "pref_filter2"), tmp_path / "pref_filter2", name)
    for h in (kept, clu, rescored, cands, sdb):
        h.free()


def _write_db(path, entries, dbtype):
    off = 0
    with open(path, "wb") as fd, open(path + ".index", "w") as fi:
        for key, data in entries:
            e = data + b"\0"
            fd.write(e); fi.write("%d\t%d\t%d\n" % (key, off, len(e))); off += len(e)
    with open(path + ".dbtype", "wb") as ft:
        ft.write(struct.pack("<i", dbtype))


def _graph_dbs(tmp, tag, lens, edges, dbtype=7):
    """a sequence DB with these lengths under keys with gaps and a prefilter DB with these edges (query index -> target indices)"""
    keys = [3 * i + (i % 3) for i in range(len(lens))]
    seq, res = os.path.join(str(tmp), tag + "_seq"), os.path.join(str(tmp), tag + "_res")
    _write_db(seq, [(k, b"A" * n + b"\n") for k, n in zip(keys, lens)], 1)
    _write_db(res, [(keys[q], b"".join(b"%d\t%d\t0\n" % (keys[t], 90 + j % 10) for j, t in enumerate(edges.get(q, ())))) for q in range(len(lens))], dbtype)
    return seq, res


def _check_against_restatement(ctx, seq, res, tmp, tag):
    sdb = ctx.read_seqdb(seq)
    cands = ctx.read_prefdb(sdb, sdb, res)
    clu, st = ctx.clust_greedy(sdb, cands)
    pairs = cc.greedy_low_mem(cc.read_index(seq), cc.read_db(res)[0])
    rep, mem = clu.download()
    assert list(zip(rep.tolist(), mem.tolist())) == pairs, tag
    out = os.path.join(str(tmp), tag + "_clu")
    clu.write(out)
    data, index = cc.cluster_db_files(cc.cluster_entries(pairs))
    assert open(out, "rb").read() == data and open(out + ".index", "rb").read() == index and cc.read_db(out)[1] == 6, tag
    for h in (clu, cands, sdb):
        h.free()
    return st, pairs


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4097])
def test_generated_graph_against_the_restatement(ctx, tmp_path, n):
    r = random.Random(n)
    lens = [r.randrange(1, 12) for _ in range(n)]                              # few distinct lengths: many ties
    edges = {q: [q] + [r.randrange(n) for _ in range(r.randrange(0, 5))] for q in range(n) if r.random() < 0.9}
    seq, res = _graph_dbs(tmp_path, "g%d" % n, lens, edges)
    st, pairs = _check_against_restatement(ctx, seq, res, tmp_path, "g%d" % n)
    assert st.n_sequences == n and st.n_edges == sum(len(v) for v in edges.values())
    if n >= 63:
        assert st.n_promoted >= 1 and 1 < st.n_clusters < n                    # both outcomes of the correction pass occur


@pytest.mark.parametrize("lines", [64, 65, 1024, 1025, 4097])
def test_one_long_list(ctx, tmp_path, lines):
    """one query with this many lines, at the hand-overs of the kernels: a wavefront's step (64) and the workgroup kernel (more than 1024)"""
    n = 4200
    r = random.Random(lines)
    lens = [r.randrange(20, 60) for _ in range(n)]
    lens[77] = 40                                                              # the query: longer than some of its targets, shorter than others
    targets = r.sample([i for i in range(n) if i != 77], lines - 1) + [77]
    edges = {q: [q] for q in range(0, n, 2)}
    edges[77] = targets
    seq, res = _graph_dbs(tmp_path, "l%d" % lines, lens, edges)
    st, pairs = _check_against_restatement(ctx, seq, res, tmp_path, "l%d" % lines)
    assert st.n_long_queries == (1 if lines > 1024 else 0)
    assert sum(1 for rep, _ in pairs if rep == 3 * 77 + 77 % 3) > lines // 4


def test_hubs_are_deterministic(ctx, tmp_path):
    """20 000 sequences, 200 000 edges, ten hubs that a tenth of the lines name: many wavefronts lower the same slots"""
    n, m = 20000, 200000
    r = random.Random(7)
    lens = [r.randrange(30, 300) for _ in range(n)]
    hubs = r.sample(range(n), 10)
    edges = {}
    for _ in range(m):
        q = r.choice(hubs) if r.random() < 0.08 else r.randrange(n)
        t = r.choice(hubs) if r.random() < 0.1 else r.randrange(n)
        edges.setdefault(q, []).append(t)
    seq, res = _graph_dbs(tmp_path, "hub", lens, edges, dbtype=14)
    pairs = cc.greedy_low_mem(cc.read_index(seq), cc.read_db(res)[0])
    sdb = ctx.read_seqdb(seq)
    cands = ctx.read_prefdb(sdb, sdb, res)
    got = []
    for _ in range(2):
        clu, st = ctx.clust_greedy(sdb, cands)
        rep, mem = clu.download()
        got.append((rep.copy(), mem.copy()))
        assert st.n_edges == m and st.n_long_queries >= 1
        clu.free()
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    assert list(zip(got[0][0].tolist(), got[0][1].tolist())) == pairs
    cands.free(); sdb.free()


def _contigs(n_base=110, seed=5):
    """rotated and mutated copies of seeded contigs: the circular-contig redundancy linclust's pre-clustering removes"""
    r = random.Random(seed)
    seqs = []
    for i in range(n_base):
        n = r.randrange(1200, 3500)
        base = "".join(r.choice("ACGT") for _ in range(n))
        seqs.append(base)
        for rate in (0.002, 0.05):                               # within and beyond --min-seq-id 0.97
            s = r.randrange(1, n)
            x = list(base[s:] + base[:s])
            for p in r.sample(range(n), int(n * rate)):
                x[p] = "ACGT"[("ACGT".index(x[p]) + 1 + r.randrange(3)) % 4]
            seqs.append("".join(x))
    r.shuffle(seqs)
    return seqs


def test_chained_behind_kmermatcher_and_hamming_on_handles(ctx, tmp_path):
    """kmermatch -> rescore_hamming -> clust_greedy -> filter_cands on handles against the restatement fed with the written DBs, and
    `plass-hip linclust-pre` on the same sequence DB against both"""
    import plass_amd
    seqs = _contigs()
    seq = str(tmp_path / "seq")
    _write_db(seq, [(2 * k + 5, s.encode() + b"\n") for k, s in enumerate(seqs)], 1)
    db = ctx.read_seqdb(seq)
    cands, kst = ctx.kmermatcher(db, plass_amd.KmermatchParams(k=22, alph_size=5, kmer_per_seq=60, kmer_per_seq_scale=0.1, hash_shift=67,
                                                             include_only_extendable=False, ignore_multi_kmer=True, cov_mode=1, c=0.99))
    kept, _ = ctx.rescore_hamming(db, db, cands, wrapped=True, min_seq_id=0.97, seq_id_mode=0, cov_mode=1, c=0.99, min_aln_len=0, e=1e-3)
    clu, st = ctx.clust_greedy(db, kept)
    sub = ctx.filter_cands(cands, clu)
    for h, name in ((cands, "pref"), (kept, "pref_rescore1"), (clu, "pre_clust"), (sub, "pref_filter2")):
        h.write(str(tmp_path / name))
    pairs = cc.greedy_low_mem(cc.read_index(seq), cc.read_db(str(tmp_path / "pref_rescore1"))[0])
    ent = cc.cluster_entries(pairs)
    data, index = cc.cluster_db_files(ent)
    assert open(tmp_path / "pre_clust", "rb").read() == data and open(str(tmp_path / "pre_clust") + ".index", "rb").read() == index
    expect = dict(cc.subset_rule(cc.read_db(str(tmp_path / "pref"))[0], [k for k, _ in ent]))
    got_type, got = read_db(tmp_path / "pref_filter2")
    assert got_type == 14 and got == {k: e + b"\0" for k, e in expect.items()}
    # the set is what it is meant to be: the near-identical rotated copies join their contig, the 5 % copies stay apart
    assert sum(1 for _, e in ent if e.count(b"\n") > 1) >= 50 and len(ent) == st.n_clusters <= len(seqs) - 50, (len(ent), st.n_clusters)
    pref = dict(cc.read_db(str(tmp_path / "pref"))[0])
    assert len(got) == len(ent) < len(pref) and sum(e.count(b"\n") for e in got.values()) < sum(pref[k].count(b"\n") for k in got)      # entries and lines were dropped
    p = subprocess.run([EXE, "linclust-pre", seq, str(tmp_path / "cli_pre_clust"), str(tmp_path / "cli_pref_filter2"), "--alph-size", "nucl:5,aa:13", "--min-seq-id", "0.97",
                        "--kmer-per-seq", "60", "--kmer-per-seq-scale", "0.100", "--cov-mode", "1", "-k", "22", "-c", "0.99", "--hash-shift", "67", "--include-only-extendable", "0",
                        "--ignore-multi-kmer", "1", "--rescore-mode", "0", "--wrapped-scoring", "1", "-e", "0.001", "--cluster-mode", "3"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    _same_files(tmp_path / "pre_clust", tmp_path / "cli_pre_clust", "linclust-pre")
    assert_same_db(tmp_path / "pref_filter2", tmp_path / "cli_pref_filter2", "linclust-pre")
    for h in (sub, clu, kept, cands, db):
        h.free()


def test_lists_of_another_db_are_refused(ctx, root, tmp_path):
    import plass_amd
    cases = ctx.read_seqdb(os.path.join(root, "clust", "cases"))
    twin = ctx.read_seqdb(os.path.join(root, "clust", "cases"))          # the same files, another handle
    star = ctx.read_seqdb(os.path.join(root, "clust", "star"))
    c7 = ctx.read_prefdb(cases, cases, os.path.join(root, "clust", "cases7"))
    a5 = ctx.read_alndb(cases, os.path.join(root, "clust", "cases5"))
    with pytest.raises(plass_amd.PlasshipError, match=r"\(-1\).*another number of queries"):
        ctx.clust_greedy(star, c7)                                         # the size differs: the reference exits there too
    with pytest.raises(plass_amd.PlasshipError, match=r"\(-1\).*another number of queries"):
        ctx.clust_greedy(star, a5)
    with pytest.raises(plass_amd.PlasshipError, match=r"\(-1\).*built on another DB"):
        ctx.clust_greedy(twin, a5)
    clu, _ = ctx.clust_greedy(cases, c7)
    s7 = ctx.read_prefdb(star, star, os.path.join(root, "clust", "star7"))
    with pytest.raises(plass_amd.PlasshipError, match=r"\(-1\).*different sizes"):
        ctx.filter_cands(s7, clu)
    with pytest.raises(plass_amd.PlasshipError, match=r"\(-1\).*does not belong to this DB"):
        clu.download(twin)
    with pytest.raises(plass_amd.PlasshipError, match=r"\(-1\).*does not belong to this DB"):
        clu.write(str(tmp_path / "no"), star)
    assert not os.path.exists(tmp_path / "no") and not os.path.exists(str(tmp_path / "no") + ".index")
    for h in (clu, s7, a5, c7, star, twin, cases):
        h.free()


def test_command_line_refuses_a_result_db_of_another_size(root, tmp_path):
    p = subprocess.run([EXE, "clust-greedy", os.path.join(root, "clust", "star"), os.path.join(root, "clust", "cases7"), str(tmp_path / "out"), "--cluster-mode", "3"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 1 and "Sequence db size != result db size" in p.stdout and not os.path.exists(tmp_path / "out")


def test_sharded_context_is_unsupported(root):
    import plass_amd
    from plass_amd.shard import LocalGroup
    ctxs = [plass_amd.Context(0) for _ in range(2)]

    def work(rank, c):
        sdb = c.read_seqdb(os.path.join(root, "clust", "cases"))
        cands = c.read_prefdb(sdb, sdb, os.path.join(root, "clust", "cases7"))
        alns = c.read_alndb(sdb, os.path.join(root, "clust", "cases5"))
        msgs = []
        for lst in (cands, alns):
            try:
                c.clust_greedy(sdb, lst)
                msgs.append("no error")
            except plass_amd.PlasshipError as e:
                msgs.append(str(e))
        alns.free(); cands.free(); sdb.free()
        return msgs

    try:
        msgs = LocalGroup(2).run(work, ctxs)
    finally:
        for c in ctxs:
            c.close()
    assert len(msgs) == 2 and all("(-4)" in m and "sharded" in m for pair in msgs for m in pair), msgs
