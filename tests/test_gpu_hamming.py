"""plasship_rescore_hamming on the GPU: `rescorediagonal --rescore-mode 0` with and without --wrapped-scoring 1, byte for byte against
the DBs the unmodified reference wrote (tests/golden/hamming.tar.gz) — through the Python binding and through the command line — and,
chained behind kmermatcher on handles, against the Python restatement (tests/tools/hamming_check.py, itself pinned on the reference by
tests/test_hamming_host.py)."""
import os
import random
import subprocess
import sys
import tarfile

import numpy as np
import pytest

from conftest import ROOT, assert_same_db, read_db

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import hamming_check as hc  # noqa: E402

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "plass_amd", "plass-hip")
with tarfile.open(os.path.join(ROOT, "tests", "golden", "hamming.tar.gz")) as _t:
    RUNS = [l.split("\t") for l in _t.extractfile("hamming/RUNS").read().decode().splitlines()]


@pytest.fixture(scope="module")
def fixture_root(tmp_path_factory):
    d = tmp_path_factory.mktemp("hamming")
    with tarfile.open(os.path.join(ROOT, "tests", "golden", "hamming.tar.gz")) as t:
        t.extractall(d)
    return os.path.join(str(d), "hamming")


@pytest.fixture(scope="module")
def ctx():
    import plass_amd
    with plass_amd.Context(0) as c:
        yield c


def _kwargs(par):
    return dict(wrapped=bool(par["wrapped"]), min_seq_id=par["min_seq_id"], seq_id_mode=par["seq_id_mode"], cov_mode=par["cov_mode"], c=par["c"],
                min_aln_len=par["min_aln_len"], e=par["e"])


@pytest.mark.parametrize("run", RUNS, ids=[r[0] for r in RUNS])
def test_fixture_through_the_binding(ctx, fixture_root, tmp_path, run):
    name, db, pref, flags = run
    sdb = ctx.read_seqdb(os.path.join(fixture_root, db))
    cands = ctx.read_prefdb(sdb, sdb, os.path.join(fixture_root, pref))
    kept, st = ctx.rescore_hamming(sdb, sdb, cands, **_kwargs(hc.parse_flags(flags)))
    kept.write(str(tmp_path / "out"))
    assert_same_db(os.path.join(fixture_root, "ref", name, "out"), tmp_path / "out", name)
    n_lines = sum(e.count(b"\n") for e in read_db(tmp_path / "out")[1].values())
    assert st.n_scored == sum(e.count(b"\n") for e in read_db(os.path.join(fixture_root, pref))[1].values()) and st.n_accepted == n_lines
    # a download shows every line but "<own key>\t0\t0", which it takes for kmermatcher's implicit self line; count() agrees with it
    hidden = sum(e.rstrip(b"\0").split(b"\n").count(b"%d\t0\t0" % k) for k, e in read_db(tmp_path / "out")[1].items())
    q, t, s, d = kept.download()
    assert len(q) == kept.count() == n_lines - hidden
    for h in (kept, cands, sdb):
        h.free()


@pytest.mark.parametrize("run", RUNS, ids=[r[0] for r in RUNS])
def test_fixture_through_the_command_line(fixture_root, tmp_path, run):
    name, db, pref, flags = run
    p = subprocess.run([EXE, "rescorediagonal-hamming", os.path.join(fixture_root, db), os.path.join(fixture_root, db), os.path.join(fixture_root, pref),
                        str(tmp_path / "out")] + flags.split(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    assert_same_db(os.path.join(fixture_root, "ref", name, "out"), tmp_path / "out", name)


def _contigs(n_base=110, seed=5):
    """rotated and mutated copies of seeded contigs: the circular-contig redundancy linclust's Hamming step removes"""
    r = random.Random(seed)
    seqs = []
    for i in range(n_base):
        n = r.randrange(1200, 3500) if i else 70000             # one contig beyond 65536: the aliases of its diagonals come into play
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


def test_chained_behind_kmermatcher_on_handles(ctx, tmp_path):
    import plass_amd
    seqs = _contigs()
    assert len(seqs) == 330
    data = b"".join(s.encode() + b"\n\0" for s in seqs)
    elen = np.array([len(s) + 2 for s in seqs], dtype=np.uint32)
    off = np.concatenate([[0], np.cumsum(elen[:-1], dtype=np.uint64)]).astype(np.uint64)
    key = np.arange(len(seqs), dtype=np.uint32)
    db = ctx.upload_seqdb(data, off, elen, key, 1)
    cands, kst = ctx.kmermatcher(db, plass_amd.KmermatchParams(k=22, alph_size=5, kmer_per_seq=60, kmer_per_seq_scale=0.1, hash_shift=67,
                                                             include_only_extendable=False, ignore_multi_kmer=True, cov_mode=1, c=0.99))
    assert kst.n_candidates >= 100
    par = dict(wrapped=1, min_seq_id=0.97, seq_id_mode=0, cov_mode=1, c=0.99, min_aln_len=0, e=1e-3, rescore_mode=0)
    kept, st = ctx.rescore_hamming(db, db, cands, **_kwargs(par))
    cands.write(str(tmp_path / "pref")); kept.write(str(tmp_path / "pref_rescore1"))
    pref_ent, pref_type = hc.read_db(str(tmp_path / "pref"))
    assert pref_type == 14
    counts = {}
    expect = dict(hc.rescore_hamming({k: s.encode() for k, s in enumerate(seqs)}, True, pref_ent, pref_type, par, counts))
    got_type, got = read_db(tmp_path / "pref_rescore1")
    assert got_type == 14 and got.keys() == expect.keys()
    bad = [k for k in expect if got[k] != expect[k] + b"\0"]
    assert not bad, "%d entries differ, first key %d:\n%r\n%r" % (len(bad), bad[0], got[bad[0]], expect[bad[0]])
    # the set is what it is meant to be: rotated copies are found and kept, the 5 % copies are found (a 22-mer survives 5 % mutations with p = 0.32, a contig
    # selects 180 k-mers or more) and dropped
    assert counts["hasSeqId"][0] >= 50 and counts["hasSeqId"][1] >= 20, counts
    assert st.n_scored == sum(e.count(b"\n") for _, e in pref_ent) and st.n_accepted == sum(e.count(b"\n") for e in expect.values())
    for h in (kept, cands, db):
        h.free()


def test_wrapped_scoring_on_proteins_is_an_error(ctx, fixture_root):
    import plass_amd
    sdb = ctx.read_seqdb(os.path.join(fixture_root, "prot"))
    cands = ctx.read_prefdb(sdb, sdb, os.path.join(fixture_root, "pref_prot7"))
    with pytest.raises(plass_amd.PlasshipError, match="Wrapped scoring is only supported for nucleotides"):
        ctx.rescore_hamming(sdb, sdb, cands, wrapped=True)
    kept, _ = ctx.rescore_hamming(sdb, sdb, cands, wrapped=False)
    for h in (kept, cands, sdb):
        h.free()


def test_sharded_context_is_unsupported(fixture_root):
    import plass_amd
    from plass_amd.shard import LocalGroup
    ctxs = [plass_amd.Context(0) for _ in range(2)]

    def work(rank, c):
        sdb = c.read_seqdb(os.path.join(fixture_root, "nucl"))
        cands = c.read_prefdb(sdb, sdb, os.path.join(fixture_root, "pref_nucl7"))
        try:
            c.rescore_hamming(sdb, sdb, cands, wrapped=True)
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
