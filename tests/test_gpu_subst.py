"""plasship_rescore_subst and plasship_*_repseqs on the GPU: `rescorediagonal --rescore-mode 1` on every run of tests/golden/subst.tar.gz
(the hand-made pairs of tests/tools/subst_cases.py at every edge of the kernel's two tiers), byte for byte against the reference's DBs and
the Python restatement (tests/tools/subst_check.py, pinned on the reference by tests/test_subst_host.py) — through the Python binding and
through the command line —, the subset call against the plain call on the createsubdb of the representatives, the protein driver against
the reference's linclust run step by step, and the representatives' sequence DBs with their file set."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, assert_same_db, read_db

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import local_cases as lcs  # noqa: E402
import subst_cases as cs  # noqa: E402
import subst_check as sc  # noqa: E402

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "plass_amd", "plass-hip")


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("subst_golden"))
    return d, cs.unpack_fixture(d)


@pytest.fixture(scope="module")
def ctx():
    import plass_amd
    with plass_amd.Context(0) as c:
        yield c


def _kwargs(flags, thr):
    par = sc.parse_flags(flags)
    return dict(min_seq_id=par["min_seq_id"], cov_mode=par["cov_mode"], c=par["c"], min_aln_len=par["min_aln_len"], e=par["e"], score_per_col_thr=thr)


def _run(*args):
    p = subprocess.run([EXE] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    return p.stdout


def _lin_flags(path):
    lin, thr = open(path).read().splitlines()
    lin = lin.split()
    return [a for i, a in enumerate(lin) if a not in ("--alignment-mode", "--remove-tmp-files") and lin[i - 1] not in ("--alignment-mode", "--remove-tmp-files")], thr


@pytest.mark.parametrize("combo", cs.COMBOS, ids=[os.path.basename(c[1]) for c in cs.COMBOS])
def test_equals_the_reference_and_the_restatement_on_every_run(ctx, fixture, tmp_path, combo):
    d, runs = fixture
    sdb = ctx.read_seqdb(os.path.join(d, combo[0]))
    cands = ctx.read_prefdb(sdb, sdb, os.path.join(d, combo[1]))
    n_in = sum(e.count(b"\n") for _, e in sc.read_db(os.path.join(d, combo[1]))[0])
    mine = [r for r in runs if (r[1], r[2]) == combo]
    assert len(mine) == len(cs.RUNS)
    for name, db, pref, flags, thr in mine:
        kept, st = ctx.rescore_subst(sdb, cands, **_kwargs(flags, thr))
        kept.write(str(tmp_path / name))
        assert_same_db(os.path.join(d, "subst", "ref", name, "out"), tmp_path / name, name)
        want, recs = cs.expected(d, db, pref, flags, thr)
        assert read_db(tmp_path / name)[1] == want and st.n_scored == n_in and st.n_accepted == len(recs) == kept.count(), name
        kept.free()
    cands.free(); sdb.free()


def test_each_tier_is_met_by_the_cases():
    """the hand-over is by min(qLen, tLen) against GROUP_MAX (rescore_subst.hip: SB_GROUP_MAX): the runs above hold pairs on both sides of it
    in every DB kind, the lengths next to it included, and wavefronts whose eight pairs are of both kinds"""
    for c, long_labels, short_labels in ((cs.prot_cases(), ("len1025", "len2049", "wave_ov1", "twice_wave", "wstep"), ("len1", "len1023", "len1024", "mixed_tier", "twice")),
                                         (cs.nuclx_cases(), ("rev1301", "rev_shift", "wave_ov20"), ("len127", "len129", "rev333")),
                                         (lcs.nucl_cases(), ("len1025", "wrap_tie", "rev_long"), ("len1", "len1024", "rev"))):
        m = lambda label: min(len(c.seqs[c.label[label + ".q"]]), len(c.seqs[c.label[label + ".t"]]))
        assert all(m(l) > cs.GROUP_MAX for l in long_labels) and all(m(l) <= cs.GROUP_MAX for l in short_labels)
        # a wavefront takes eight consecutive lines of the list: some hold both kinds
        kinds = [min(len(c.seqs[k]), len(c.seqs[t])) > cs.GROUP_MAX for k in sorted(c.seqs) for t, _, _ in c.lines[k]]
        assert any(0 < sum(kinds[i:i + 8]) < len(kinds[i:i + 8]) for i in range(0, len(kinds), 8))


def test_thresholds_met_with_equality(ctx, fixture, tmp_path):
    """score per column == threshold: kept, the next float above as threshold: dropped; -e == the pair's E-value: kept, the next double below: dropped"""
    d, _ = fixture
    p = cs.prot_cases()
    seqs, _ = sc.read_seqdb(os.path.join(d, "subst", "prot"))
    q, t = p.label["len300.q"], p.label["len300.t"]
    lcs.write_db(str(tmp_path / "pref"), [(k, (b"%d\t17\t0\n" % t) if k == q else b"") for k in sorted(seqs)], 7)
    pref = sc.read_db(str(tmp_path / "pref"))[0]
    sdb = ctx.read_seqdb(os.path.join(d, "subst", "prot"))
    cands = ctx.read_prefdb(sdb, sdb, str(tmp_path / "pref"))
    par = sc.parse_flags("--rescore-mode 1 -e 10 --min-seq-id 0.0 -c 0 --cov-mode 0 --min-aln-len 0")
    r = sc.rescore_subst(seqs, False, pref, 7, par)[1][0]
    per_col, evalue = float(r["per_col"]), r["evalue"]
    for kw, n in ((dict(min_seq_id=0.9, e=10, score_per_col_thr=per_col), 1), (dict(min_seq_id=0.9, e=10, score_per_col_thr=float(np.nextafter(np.float32(per_col), np.float32(np.inf)))), 0),
                  (dict(e=evalue), 1), (dict(e=float(np.nextafter(evalue, 0.0))), 0), (dict(e=10, min_aln_len=1), 0)):
        kept, st = ctx.rescore_subst(sdb, cands, **kw)
        par2 = dict(par, min_seq_id=kw.get("min_seq_id", 0.0), e=kw["e"], min_aln_len=kw.get("min_aln_len", 0), thr=kw.get("score_per_col_thr"))
        assert st.n_accepted == n == len(sc.rescore_subst(seqs, False, pref, 7, par2)[1]), kw
        kept.free()
    cands.free(); sdb.free()


def test_through_the_command_line(fixture, tmp_path):
    d, runs = fixture
    for name, db, pref, flags, thr in runs:
        if name not in ("pref_prot7_fh_lin", "pref_prot7_lax", "pref_nuclx14_fh_norow", "pref_nucl14_cov"):
            continue
        extra = [] if thr is None else ["--score-per-col-thr", repr(thr)]
        _run("rescorediagonal-subst", os.path.join(d, db), os.path.join(d, db), os.path.join(d, pref), tmp_path / name, *flags.split(), *extra)
        assert_same_db(os.path.join(d, "subst", "ref", name, "out"), tmp_path / name, name)


def test_subset_equals_the_plain_call_on_the_subset_db(ctx, fixture, tmp_path):
    """plasship_rescore_subst_subset on the whole DB with the clustering against plasship_rescore_subst on the createsubdb of its representatives
    (written here), and both against the reference's pref_rescore2"""
    d, _ = fixture
    ref = os.path.join(d, "subst", "ref", "linclust_prot")
    _, thr = _lin_flags(os.path.join(d, "subst", "LINCLUST"))
    kw = dict(min_seq_id=0.9, cov_mode=1, c=0.8, e=0.001, score_per_col_thr=float(thr))
    fam = ctx.read_seqdb(os.path.join(d, "subst", "fam"))
    pre = ctx.read_clusters(fam, os.path.join(ref, "pre_clust"))
    pref = ctx.read_prefdb(fam, fam, os.path.join(ref, "pref"))
    filtered = ctx.filter_cands(pref, pre)
    kept, st = ctx.rescore_subst(fam, filtered, subset=pre, **kw)
    kept.write(str(tmp_path / "subset"))
    assert_same_db(os.path.join(ref, "pref_rescore2"), tmp_path / "subset", "the subset call against the reference's pref_rescore2")
    seqs, _ = sc.read_seqdb(os.path.join(d, "subst", "fam"))
    reps = sorted(read_db(os.path.join(ref, "pre_clust"))[1])
    lcs.write_db(str(tmp_path / "sub"), [(k, seqs[k] + b"\n") for k in reps], 0)
    sub = ctx.read_seqdb(str(tmp_path / "sub"))
    c2 = ctx.read_prefdb(sub, sub, os.path.join(ref, "pref_filter2"))
    kept2, st2 = ctx.rescore_subst(sub, c2, **kw)
    kept2.write(str(tmp_path / "plain"))
    assert_same_db(tmp_path / "plain", tmp_path / "subset", "plain call on the subset DB against the subset call")
    assert st.n_accepted == st2.n_accepted and 0 < st.n_accepted < st.n_scored == st2.n_scored
    # the list goes on to the alignment step on handles
    alns, _ = ctx.rescore_local(fam, kept, min_seq_id=0.9, cov_mode=1, c=0.8, e=0.001, score_per_col_thr=float(thr), subset=pre)
    alns.write(str(tmp_path / "aln"))
    # (an alignment list made on the whole DB is written with an entry per sequence: the representatives' are the reference's, the others are empty)
    want, got = read_db(os.path.join(ref, "aln")), read_db(tmp_path / "aln")
    assert got[0] == want[0] == 5 and {k: got[1][k] for k in want[1]} == want[1] and all(e == b"\0" for k, e in got[1].items() if k not in want[1])
    for h in (alns, kept2, c2, sub, kept, filtered, pref, pre, fam):
        h.free()


def _files(prefix):
    d, b = os.path.dirname(str(prefix)), os.path.basename(str(prefix))
    return sorted(f for f in os.listdir(d) if f == b or f.startswith(b + ".") or f.startswith(b + "_"))


def test_linclust_ungapped_prot_equals_the_reference_and_the_modules_one_by_one(fixture, tmp_path):
    """`plass-hip linclust-ungapped-prot --rep-out` on the fixture's protein DB against the `clu` DB the reference's `linclust --alignment-mode 4`
    wrote with the same flags and against its result2repseq, and the same steps as single commands against every intermediate DB"""
    d, _ = fixture
    ref = os.path.join(d, "subst", "ref", "linclust_prot")
    fam = os.path.join(d, "subst", "fam")
    lin, thr = _lin_flags(os.path.join(d, "subst", "LINCLUST"))
    _run("linclust-ungapped-prot", fam, tmp_path / "clu", *lin, "--score-per-col-thr", thr, "--rep-out", tmp_path / "rep")
    assert_same_db(os.path.join(ref, "clu"), tmp_path / "clu", "linclust-ungapped-prot against the reference's linclust")
    assert_same_db(os.path.join(ref, "rep"), tmp_path / "rep", "--rep-out against the reference's result2repseq")
    assert _files(tmp_path / "rep") == ["rep", "rep.dbtype", "rep.index"] == [os.path.basename(f) for f in open(os.path.join(d, "subst", "REPFILES")).read().split() if f.startswith("linclust_prot/")]
    # one module after the other
    kmer = ["-k", "14", "--kmer-per-seq", "60", "--kmer-per-seq-scale", "0", "--alph-size", "aa:13,nucl:5", "--hash-shift", "67", "--ignore-multi-kmer", "1"]
    gates = ["--min-seq-id", "0.9", "-c", "0.8", "--cov-mode", "1", "-e", "0.001"]
    _run("kmermatcher", fam, tmp_path / "pref", *kmer, *gates[:6])
    assert_same_db(os.path.join(ref, "pref"), tmp_path / "pref", "pref")
    _run("rescorediagonal-hamming", fam, fam, tmp_path / "pref", tmp_path / "pref_rescore1", *gates, "--rescore-mode", "0")
    assert_same_db(os.path.join(ref, "pref_rescore1"), tmp_path / "pref_rescore1", "pref_rescore1")
    _run("linclust-pre", fam, tmp_path / "pre_clust", tmp_path / "pref_filter2", *kmer, *gates, "--rescore-mode", "0", "--cluster-mode", "2")
    assert_same_db(os.path.join(ref, "pre_clust"), tmp_path / "pre_clust", "pre_clust")
    assert_same_db(os.path.join(ref, "pref_filter2"), tmp_path / "pref_filter2", "pref_filter2")
    seqs, _ = sc.read_seqdb(fam)
    reps = sorted(read_db(tmp_path / "pre_clust")[1])
    lcs.write_db(str(tmp_path / "sub"), [(k, seqs[k] + b"\n") for k in reps], 0)
    _run("rescorediagonal-subst", tmp_path / "sub", tmp_path / "sub", tmp_path / "pref_filter2", tmp_path / "pref_rescore2", *gates, "--rescore-mode", "1", "--filter-hits", "1", "--score-per-col-thr", thr)
    assert_same_db(os.path.join(ref, "pref_rescore2"), tmp_path / "pref_rescore2", "the filter step against the reference's pref_rescore2")
    _run("rescorediagonal-local", tmp_path / "sub", tmp_path / "sub", tmp_path / "pref_rescore2", tmp_path / "aln", *gates, "--rescore-mode", "2", "--filter-hits", "1", "--score-per-col-thr", thr)
    assert_same_db(os.path.join(ref, "aln"), tmp_path / "aln", "the alignment step against the reference's aln")
    _run("clust-greedy", tmp_path / "sub", tmp_path / "aln", tmp_path / "clust", "--cluster-mode", "2")
    assert_same_db(os.path.join(ref, "clust"), tmp_path / "clust", "clust")
    _run("mergeclusters-greedy", fam, tmp_path / "clu_steps", tmp_path / "pre_clust", tmp_path / "clust")
    assert_same_db(tmp_path / "clu", tmp_path / "clu_steps", "module by module against the driver")
    _run("clust-repseq", fam, tmp_path / "clu_steps", tmp_path / "rep_steps", "--threads", "1")
    assert_same_db(tmp_path / "rep", tmp_path / "rep_steps", "clust-repseq against --rep-out")


def test_repseq_on_the_nucleotide_fixture_with_its_file_set(ctx, fixture, tmp_path):
    """`linclust-ungapped --rep-out` and `clust-repseq` on local.tar.gz's nucleotide run against the reference's result2repseq; a sequence DB
    with header, lookup and source files gets their soft links, as DBReader::softlinkDb(..., SEQUENCE_ANCILLARY) makes them"""
    d, _ = fixture
    want = os.path.join(d, "subst", "ref", "rep_nucl", "rep")
    nucl = str(tmp_path / "nucl")
    for e in ("", ".index", ".dbtype"):
        os.symlink(os.path.join(d, "local", "nucl") + e, nucl + e)
    keys = sorted(read_db(nucl)[1])
    lcs.write_db(nucl + "_h", [(k, b"seq%d\n" % k) for k in keys], 12)
    open(nucl + ".lookup", "w").write("".join("%d\tseq%d\t0\n" % (k, k) for k in keys))
    open(nucl + ".source", "w").write("0\tnucl.fasta\n")
    lin, thr = _lin_flags(os.path.join(d, "local", "LINCLUST"))
    _run("linclust-ungapped", nucl, tmp_path / "clu", *lin, "--score-per-col-thr", thr, "--rep-out", tmp_path / "rep")
    assert_same_db(os.path.join(d, "local", "ref", "linclust", "clu"), tmp_path / "clu", "linclust-ungapped")
    assert_same_db(want, tmp_path / "rep", "linclust-ungapped --rep-out against the reference's result2repseq")
    _run("clust-repseq", nucl, os.path.join(d, "local", "ref", "linclust", "clu"), tmp_path / "rep2")
    assert_same_db(want, tmp_path / "rep2", "clust-repseq against the reference's result2repseq")
    for rep in ("rep", "rep2"):
        assert _files(tmp_path / rep) == sorted(rep + s for s in ("", ".dbtype", ".index", ".lookup", ".source", "_h", "_h.dbtype", "_h.index"))
        for s in (".lookup", ".source", "_h", "_h.dbtype", "_h.index"):
            assert os.path.islink(str(tmp_path / rep) + s) and os.readlink(str(tmp_path / rep) + s) == os.path.realpath(nucl + s)
        assert not os.path.islink(str(tmp_path / rep)) and not os.path.islink(str(tmp_path / rep) + ".index")
    # through the binding, from both kinds of clustering; a list that does not start with its own key is not taken
    sdb = ctx.read_seqdb(nucl)
    c1 = ctx.read_clusters(sdb, os.path.join(d, "local", "ref", "linclust", "pre_clust"))
    c2 = ctx.read_clusters(sdb, os.path.join(d, "local", "ref", "linclust", "clust"))
    m = ctx.merge_clusters(sdb, c1, c2)
    r1, r2 = ctx.repseqs(m), ctx.repseqs(c1)
    r1.write(str(tmp_path / "rep3")); r2.write(str(tmp_path / "rep4"))
    assert_same_db(want, tmp_path / "rep3", "Context.repseqs of the merged clustering")
    seqs = dict(sc.read_db(nucl)[0])
    assert read_db(tmp_path / "rep4") == (1, sc.repseqs(seqs, sc.read_db(os.path.join(d, "local", "ref", "linclust", "pre_clust"))[0]))
    assert r1.info()["n"] == m.count()[1] and r2.info()["n"] == c1.count()[1] > r1.info()["n"]
    for h in (r2, r1, m, c2, c1, sdb):
        h.free()
    lcs.write_db(str(tmp_path / "odd"), [(keys[0], b"%d\n%d\n" % (keys[1], keys[0]))], 6)
    p = subprocess.run([EXE, "clust-repseq", nucl, str(tmp_path / "odd"), str(tmp_path / "rep5")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 95 and not os.path.exists(str(tmp_path / "rep5"))


def test_sharded_context_is_unsupported(fixture):
    import plass_amd
    from plass_amd.shard import LocalGroup
    d, _ = fixture
    ctxs = [plass_amd.Context(0) for _ in range(2)]

    def work(rank, c):
        sdb = c.read_seqdb(os.path.join(d, "subst", "prot"))
        cands = c.read_prefdb(sdb, sdb, os.path.join(d, "subst", "pref_prot7"))
        msgs = []
        try:
            c.rescore_subst(sdb, cands)
            msgs.append("no error")
        except plass_amd.PlasshipError as e:
            msgs.append(str(e))
        finally:
            cands.free(); sdb.free()
        return msgs[0]

    try:
        msgs = LocalGroup(2).run(work, ctxs)
    finally:
        for c in ctxs:
            c.close()
    assert len(msgs) == 2 and all("(-4)" in m and "sharded" in m for m in msgs), msgs
