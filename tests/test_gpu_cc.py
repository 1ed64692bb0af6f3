"""clust-connected on the GPU: every `clust --cluster-mode 1` DB of tests/golden/cc.tar.gz through the library and through the command line, byte
for byte against the files the unmodified reference wrote; seeded random graphs against the restatement (tests/tools/cc_check.py, pinned on the
same fixture by tests/test_cc_host.py); the path one step too deep for --max-iterations, which is refused; and both fused linclust drivers with
--cluster-mode 1 against the reference's linclust runs, with the same steps as single commands."""
import os
import random
import subprocess
import sys

import pytest

from conftest import ROOT, assert_same_db, read_db

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import cc_cases  # noqa: E402
import cc_check as cc  # noqa: E402
import local_cases as lcs  # noqa: E402

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "plass_amd", "plass-hip")
N_RANDOM_GPU = cc_cases.N_RANDOM


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    return cc.extract_fixtures(tmp_path_factory.mktemp("cc_golden"))


@pytest.fixture(scope="module")
def ctx():
    import plass_amd
    with plass_amd.Context(0) as c:
        yield c


def _exe(*args):
    return subprocess.run([EXE] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _run(*args):
    p = _exe(*args)
    assert p.returncode == 0, p.stdout
    return p.stdout


def _same_files(ref, got, what):
    """data file, index and dbtype byte for byte"""
    for sfx in ("", ".index", ".dbtype"):
        assert open(str(ref) + sfx, "rb").read() == open(str(got) + sfx, "rb").read(), "%s: %s differs" % (what, sfx or "data file")


def _lin_flags(path):
    lin, thr = open(path).read().splitlines()
    lin = lin.split()
    return [a for i, a in enumerate(lin) if a not in ("--alignment-mode", "--remove-tmp-files") and lin[i - 1] not in ("--alignment-mode", "--remove-tmp-files")], thr


def _library(ctx, db_path, res_path, max_iterations, out):
    db = ctx.read_seqdb(db_path)
    lst = ctx.read_alndb(db, res_path) if read_db(res_path)[0] == 5 else ctx.read_prefdb(db, db, res_path)
    try:
        cl, st = ctx.clust_connected(db, lst, max_iterations=max_iterations)
    finally:
        lst.free()
    cl.write(out)
    rep, mem = cl.download()
    count = cl.count()
    cl.free(); db.free()
    return st, rep, mem, count


def test_every_golden_run_through_the_library_and_the_command_line(ctx, fixture, tmp_path):
    import plass_amd
    for name, db, res, flags, status in cc.runs(fixture):
        db, res, m = os.path.join(fixture, db), os.path.join(fixture, res), cc.parse_max_iterations(flags)
        want = os.path.join(fixture, "cc", "ref", name, "out")
        cli = _exe("clust-connected", db, res, tmp_path / (name + "_cli"), *flags.split())
        if status == "fail":                                  # no entry for one sequence: the reference's own error
            assert cli.returncode == 1 and "Sequence db size != result db size" in cli.stdout and not os.path.exists(tmp_path / (name + "_cli"))
            continue
        if name == "depth_m2":                                # one step too deep: refused, nothing written
            assert cli.returncode == 95 and "nothing was written" in cli.stdout and not os.path.exists(tmp_path / (name + "_cli")) and not os.path.exists(tmp_path / (name + "_cli.index"))
            with pytest.raises(plass_amd.PlasshipError, match="max-iterations"):
                _library(ctx, db, res, m, str(tmp_path / name))
            assert not os.path.exists(tmp_path / name)
            continue
        assert cli.returncode == 0, cli.stdout
        assert_same_db(want, tmp_path / (name + "_cli"), name + " through the command line")
        _same_files(want, tmp_path / (name + "_cli"), name + " through the command line")
        st, rep, mem, count = _library(ctx, db, res, m, str(tmp_path / name))
        assert_same_db(want, tmp_path / name, name + " through the library")
        _same_files(want, tmp_path / name, name + " through the library")
        entries = read_db(want)[1]
        assert count == (len(rep), len(entries)) and st.n_clusters == len(entries) and st.n_sequences == len(rep)
        assert sorted(zip(rep.tolist(), mem.tolist())) == list(zip(rep.tolist(), mem.tolist()))
        assert set(rep.tolist()) == set(entries)
        if name == "star":
            assert st.n_edges == 10001 and st.n_missing_links == 5000 and st.n_bfs_levels == 1
        if name == "star_in":
            assert st.n_missing_links == 1499
        if name == "path300":
            assert st.n_hook_rounds > 2 and st.n_bfs_levels >= 150
        if name == "depth_m1":
            assert st.n_bfs_levels == 4


def test_random_graphs_equal_the_restatement(ctx, tmp_path):
    """the seeded graphs of tests/test_cc_host.py (all of them): the restatement's DB where the eccentricity condition holds, a refusal where it does not"""
    import plass_amd
    refused = 0
    for seed in range(N_RANDOM_GPU):
        seqs, lists, dbtype, m = cc_cases.random_case(seed)
        cc_cases.write_case(str(tmp_path), "g%d" % seed, seqs, lists, dbtype, random.Random(seed))
        db, res = str(tmp_path / ("g%d" % seed)), str(tmp_path / ("g%d_res" % seed))
        if cc.condition_holds(db, res, m):
            _library(ctx, db, res, m, str(tmp_path / ("o%d" % seed)))
            assert read_db(tmp_path / ("o%d" % seed)) == (6, {k: e + b"\0" for k, e in cc.clust(db, res, m)}), seed
        else:
            refused += 1
            with pytest.raises(plass_amd.PlasshipError, match="max-iterations"):
                _library(ctx, db, res, m, str(tmp_path / ("o%d" % seed)))
    assert refused < N_RANDOM_GPU // 2


@pytest.mark.parametrize("kind,driver,dbname", [("nucl", "linclust-ungapped", "local/nucl"), ("prot", "linclust-ungapped-prot", "subst/fam")])
def test_linclust_drivers_in_mode_1_equal_the_reference_and_the_modules_one_by_one(fixture, tmp_path, kind, driver, dbname):
    """`plass-hip linclust-ungapped[-prot] --cluster-mode 1 --rep-out` against the `clu` DB the reference's `linclust --alignment-mode 4 --cluster-mode 1`
    wrote with the same flags and against its result2repseq, and the same steps as single commands with clust-connected in place of clust-greedy"""
    ref = os.path.join(fixture, "cc", "ref", "linclust_" + kind)
    db = os.path.join(fixture, dbname)
    lin, thr = _lin_flags(os.path.join(fixture, "cc", "LINCLUST_" + kind.upper()))
    out = _run(driver, db, tmp_path / "clu", *lin, "--score-per-col-thr", thr, "--rep-out", tmp_path / "rep")
    assert "hook rounds" in out
    assert_same_db(os.path.join(ref, "clu"), tmp_path / "clu", driver + " --cluster-mode 1 against the reference's linclust")
    assert_same_db(os.path.join(ref, "rep"), tmp_path / "rep", "--rep-out against the reference's result2repseq")
    # one module after the other, from the reference's own intermediate lists
    _run("clust-connected", db, os.path.join(ref, "pref_rescore1"), tmp_path / "pre_clust", "--cluster-mode", "1")
    _same_files(os.path.join(ref, "pre_clust"), tmp_path / "pre_clust", "pre_clust")
    seqs = dict(cc.read_db(db)[0])
    reps = sorted(read_db(tmp_path / "pre_clust")[1])
    lcs.write_db(str(tmp_path / "sub"), [(k, seqs[k]) for k in reps], read_db(db)[0])
    gates = [a for i, a in enumerate(lin) if a in ("--min-seq-id", "-c", "--cov-mode", "-e") or lin[i - 1] in ("--min-seq-id", "-c", "--cov-mode", "-e")]
    last = os.path.join(ref, "pref_rescore2" if kind == "prot" else "pref_filter2")
    _run("rescorediagonal-local", tmp_path / "sub", tmp_path / "sub", last, tmp_path / "aln", *gates, "--rescore-mode", "2", "--filter-hits", "1", "--score-per-col-thr", thr)
    assert_same_db(os.path.join(ref, "aln"), tmp_path / "aln", "the alignment step against the reference's aln")
    _run("clust-connected", tmp_path / "sub", tmp_path / "aln", tmp_path / "clust", "--cluster-mode", "1")
    assert_same_db(os.path.join(ref, "clust"), tmp_path / "clust", "clust")
    _run("mergeclusters-greedy", db, tmp_path / "clu_steps", tmp_path / "pre_clust", tmp_path / "clust")
    assert_same_db(tmp_path / "clu", tmp_path / "clu_steps", "module by module against the driver")
    _run("clust-repseq", db, tmp_path / "clu_steps", tmp_path / "rep_steps", "--threads", "1")
    assert_same_db(os.path.join(ref, "rep"), tmp_path / "rep_steps", "clust-repseq behind a mode 1 run against the reference's result2repseq")


def test_refusals_of_the_library(ctx, fixture):
    import plass_amd
    db = ctx.read_seqdb(os.path.join(fixture, "cc", "mixed7"))
    other = ctx.read_seqdb(os.path.join(fixture, "cc", "dup"))
    lst = ctx.read_prefdb(db, db, os.path.join(fixture, "cc", "mixed7_res"))
    with pytest.raises(plass_amd.PlasshipError, match="max_iterations must be at least 1"):
        ctx.clust_connected(db, lst, max_iterations=0)
    with pytest.raises(plass_amd.PlasshipError, match="another number of queries"):
        ctx.clust_connected(other, lst)
    for h in (lst, other, db):
        h.free()
