"""clust-connected (`clust --cluster-mode 1`, connected component) without a GPU: the sequential Python restatement (tests/tools/cc_check.py)
against every DB the unmodified reference wrote (tests/golden/cc.tar.gz), the order-free rule the GPU computes against the restatement on seeded
random graphs, the new command lines in dry run, the wrapper's opt-in routing and the exported symbols of the new extension library."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import cc_cases  # noqa: E402
import cc_check as cc  # noqa: E402

EXE = os.path.join(ROOT, "plass_amd", "plass-hip")
WRAPPER = os.path.join(ROOT, "plass_amd", "plass-gpu-wrapper")
CLUST = ["--cluster-mode", "1", "--max-iterations", "1000", "--similarity-type", "2", "--threads", "4", "--compressed", "0", "-v", "3"]


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    return cc.extract_fixtures(tmp_path_factory.mktemp("cc_golden"))


def _cli(*args, level="1"):
    p = subprocess.run([EXE] + list(args), env=dict(os.environ, PLASSHIP_CLI_DRYRUN=level), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return p.returncode, p.stdout


def test_restatement_equals_the_reference_byte_for_byte(fixture):
    """every `clust --cluster-mode 1` DB the unmodified reference wrote, the path that is one step too deep for --max-iterations included (there
    the later search steals the node at the cut: two clusters), and the result DB without an entry for one sequence, which the reference refuses"""
    seen = set()
    for name, db, res, flags, status in cc.runs(fixture):
        db, res = os.path.join(fixture, db), os.path.join(fixture, res)
        if status == "fail":
            with pytest.raises(ValueError, match="Sequence db size != result db size"):
                cc.clust(db, res)
            assert not os.path.exists(os.path.join(fixture, "cc", "ref", name))
        else:
            want = cc.read_db(os.path.join(fixture, "cc", "ref", name, "out"))
            assert want[1] == 6 and cc.clust(db, res, cc.parse_max_iterations(flags)) == want[0], name
        seen.add(name)
    assert seen == {c[0] for c in cc_cases.hand_made(__import__("random").Random(0))}
    # the depth rule: eccentricity m + 1 and m + 2 of the representative
    by = {r[0]: r for r in cc.runs(fixture)}
    holds = {n: cc.condition_holds(os.path.join(fixture, by[n][1]), os.path.join(fixture, by[n][2]), cc.parse_max_iterations(by[n][3])) for n in by if by[n][4] == "ok"}
    assert not holds.pop("depth_m2") and all(holds.values())
    assert len(cc.read_db(os.path.join(fixture, "cc", "ref", "depth_m1", "out"))[0]) == 1 and len(cc.read_db(os.path.join(fixture, "cc", "ref", "depth_m2", "out"))[0]) == 2


@pytest.mark.parametrize("kind,db", [("nucl", "local/nucl"), ("prot", "subst/fam")])
def test_restatement_equals_the_reference_linclust_runs(fixture, kind, db):
    """both `clust` calls of the reference's `linclust --alignment-mode 4 --cluster-mode 1`: on the whole DB with the Hamming step's list, and on the
    subset DB of the first call's representatives with the alignment step's"""
    ref = os.path.join(fixture, "cc", "ref", "linclust_" + kind)
    assert "--cluster-mode 1" in open(os.path.join(fixture, "cc", "LINCLUST_" + kind.upper())).readline()
    assert cc.clust(os.path.join(fixture, db), os.path.join(ref, "pref_rescore1")) == cc.read_db(os.path.join(ref, "pre_clust"))[0]
    reps = {int(l) for l in open(os.path.join(ref, "order_redundancy"))}
    sub = [(k, l) for k, l in cc.read_index(os.path.join(fixture, db)) if k in reps]
    local_key, lists = cc.read_lists(sub, cc.read_db(os.path.join(ref, "aln"))[0])
    assert cc.cluster_entries(cc.pairs_of(local_key, cc.connected_component(cc.symmetrise(lists), 1000))) == cc.read_db(os.path.join(ref, "clust"))[0]


def _numpy_rule(n, q, t):
    """the order-free rule on arrays: q, t = the lines (ids), an entry without lines already given as the line to itself -> representative of every id.
    Sizes by a sorted search for the reverse line, rank by one lexsort, components by minimum-rank label propagation until nothing changes"""
    key = q.astype(np.int64) << 32 | t
    srt = np.sort(key)
    rev = t.astype(np.int64) << 32 | q
    at = np.searchsorted(srt, rev)
    missing = (at == len(srt)) | (srt[np.minimum(at, len(srt) - 1)] != rev)
    size = np.bincount(q, minlength=n) + np.bincount(t[missing], minlength=n)
    order = np.lexsort((-np.arange(n), -size))              # (size descending, id descending)
    rank = np.empty(n, np.int64); rank[order] = np.arange(n)
    label = rank.copy()
    while True:
        new = label.copy()
        np.minimum.at(new, q, label[t]); np.minimum.at(new, t, label[q])
        if (new == label).all():
            return order[label]
        label = new


def test_order_free_rule_equals_the_restatement_on_random_graphs():
    """components + the largest (symmetric list size, id) member, in numpy, against the sequential restatement with its depth cut on seeded random
    graphs with one-directional lines and small --max-iterations: equal wherever no node lies deeper than max_iterations + 1 below its
    representative; at most 20 % of the graphs may fail that condition"""
    excluded = 0
    for seed in range(cc_cases.N_RANDOM):
        seqs, lists, _, m = cc_cases.random_case(seed)
        seqs = sorted(seqs)
        local_key, ll = cc.read_lists([(k, n + 2) for k, n in seqs], [(k, "".join("%d\n" % t for t in lists.get(k, [])).encode()) for k, _ in seqs])
        sym = cc.symmetrise(ll)
        want = cc.connected_component(sym, m)
        rule, holds = cc.order_free(sym, m)
        q = np.array([i for i, l in enumerate(ll) for _ in l], np.int64); t = np.array([e for l in ll for e in l], np.int64)
        got = _numpy_rule(len(ll), q, t)
        assert list(got) == rule, seed                      # the two statements of the rule agree everywhere
        if holds:
            assert rule == want, seed
        else:
            excluded += 1
    assert excluded <= 0.2 * cc_cases.N_RANDOM, excluded


def test_command_lines_in_dry_run(fixture):
    rc, out = _cli("clust-connected", "db", "res", "clu", *CLUST, level="2")
    assert rc == 96 and "clust-connected accepted (3 positional arguments" in out
    assert _cli("clust-connected", "db", "res", "clu", "--cluster-mode", "1")[0] == 96
    for res in ("cc/mixed7_res", "cc/mixed14_res", "cc/mixed5_res"):
        assert _cli("clust-connected", os.path.join(fixture, "cc/mixed7"), os.path.join(fixture, res), "clu", "--cluster-mode", "1")[0] == 96
    for extra in (["--cluster-mode", "0"], ["--cluster-mode", "2"], ["--cluster-mode", "3"], [], ["--cluster-mode", "1", "--compressed", "1"]):
        rc, out = _cli("clust-connected", "db", "res", "clu", *extra)
        assert rc == 95 and "nothing was written" in out, extra
    rc, out = _cli("clust-connected", os.path.join(fixture, "cc/mixed7"), os.path.join(fixture, "cc/ref/mixed7/out"), "clu", "--cluster-mode", "1")     # a cluster DB as result DB
    assert rc == 95 and "result DB of type 6" in out
    assert _cli("clust-connected", "db", "res", "clu", "--cluster-mode", "1", "--no-such-flag", "1")[0] == 1
    assert _cli("clust-connected", "db", "res", "clu", "--cluster-mode", "1", "-k", "14")[0] == 1                      # kmermatcher's flag
    rc, out = _cli("clust-connected", "db", "res", "clu", "--cluster-mode", "1", "--max-iterations", "0")               # Parameters.cpp:91: ^[1-9]{1}[0-9]*$
    assert rc == 1 and "Error in argument --max-iterations" in out
    # the drivers take mode 1 now and keep their other answers
    for kind, driver in (("NUCL", "linclust-ungapped"), ("PROT", "linclust-ungapped-prot")):
        lin, thr = open(os.path.join(fixture, "cc", "LINCLUST_" + kind)).read().splitlines()
        lin = lin.split()
        lin = [a for i, a in enumerate(lin) if a not in ("--alignment-mode", "--remove-tmp-files") and lin[i - 1] not in ("--alignment-mode", "--remove-tmp-files")]
        assert "--cluster-mode" in lin and lin[lin.index("--cluster-mode") + 1] == "1"
        assert _cli(driver, "db", "clu", *lin, "--score-per-col-thr", thr)[0] == 96
        assert _cli(driver, "db", "clu", *lin, "--score-per-col-thr", thr, "--max-iterations", "5", "--rep-out", "rep")[0] == 96
        assert _cli(driver, "db", "clu", *lin, "--score-per-col-thr", thr, "--max-iterations", "0")[0] == 1
        other = [a for i, a in enumerate(lin) if a != "--cluster-mode" and lin[i - 1] != "--cluster-mode"]
        for mode, want in (("0", 95), ("2", 96), ("3", 96), ("4", 95)):
            assert _cli(driver, "db", "clu", *other, "--score-per-col-thr", thr, "--cluster-mode", mode)[0] == want, (driver, mode)
        assert _cli(driver, "db", "clu", *other, "--score-per-col-thr", thr)[0] == 95                                 # the module's default is set cover
    # the previously pinned answers: mode 1 stays refused where it is not built
    for args in (["clust-greedy", "db", "res", "clu", "--cluster-mode", "1"], ["linclust-pre", "db", "a", "b", "--cluster-mode", "1"], ["clust", "db", "res", "clu", "--cluster-mode", "1"]):
        rc, out = _cli(*args)
        assert rc == 95 and "nothing was written" in out, args
    assert _cli("clust-greedy", "db", "res", "clu", "--cluster-mode", "3", "--max-iterations", "0")[0] == 96            # read by connected component only


def test_wrapper_routes_only_when_asked(tmp_path):
    ref = tmp_path / "ref"
    ref.write_text("#!/bin/bash\necho \"REF argv0=$0 args=$*\"\n")
    ref.chmod(0o755)
    log = tmp_path / "log"
    base = dict(os.environ, PLASSHIP_CLI_DRYRUN="1", PLASS_REF_BIN=str(ref), PLASS_WRAPPER_LOG=str(log))
    for v in ("PLASS_GPU_CLUST", "PLASS_GPU_CC", "PLASS_GPU_HAMMING", "PLASS_GPU_LOCAL", "PLASS_GPU_SUBST", "PLASS_GPU_REPSEQ"):
        base.pop(v, None)
    call = ["clust", "db", "res", "clu"] + CLUST
    greedy = [a if a != "1" or call[i - 1] != "--cluster-mode" else "3" for i, a in enumerate(call)]

    def run(args, **env):
        return subprocess.run([WRAPPER] + args, env=dict(base, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)

    out = run(call, PLASS_GPU_CC="1")
    assert out.returncode == 0 and "clust-connected accepted" in out.stdout and "args=clust db res clu --cluster-mode 1" in out.stdout
    out = run(greedy, PLASS_GPU_CC="1")                     # 95: the reference runs
    assert out.returncode == 0 and "accepted" not in out.stdout and "REF" in out.stdout
    out = run(call + ["--no-such-flag", "1"], PLASS_GPU_CC="1")
    assert out.returncode == 1 and "REF" not in out.stdout
    out = run(greedy, PLASS_GPU_CC="1", PLASS_GPU_CLUST="1")   # both: what clust-connected refuses goes on to clust-greedy
    assert out.returncode == 0 and "clust-greedy accepted" in out.stdout and "REF" in out.stdout
    # not opted in, or opted into something else: unchanged
    for env in ({}, {"PLASS_GPU_CC": "0"}, {"PLASS_GPU_LOCAL": "1"}, {"PLASS_GPU_CLUST": "1"}):
        out = run(call, **env)
        assert out.returncode == 0 and "accepted" not in out.stdout and "REF" in out.stdout, env
    out = run(greedy, PLASS_GPU_CLUST="1")
    assert out.returncode == 0 and "clust-greedy accepted" in out.stdout and "clust-connected" not in out.stdout
    lines = log.read_text().splitlines()
    assert lines[0].startswith("GPU path   (dry run: clust-connected accepted, the reference computes) : clust db")
    assert lines[1].startswith("reference  <- plass-hip exit 95 (outside the GPU path) : clust db")
    assert lines[2].startswith("GPU path   clust-connected exit 1 : clust")
    assert lines[3].startswith("reference  <- plass-hip exit 95") and lines[4].startswith("GPU path   (dry run: clust-greedy accepted")
    assert all(l.startswith("reference  (not a hot-path module) : clust") for l in lines[5:8])
    assert lines[8].startswith("reference  <- plass-hip exit 95") and lines[9].startswith("GPU path   (dry run: clust-greedy accepted") and len(lines) == 10


def test_library_exports_the_new_entries():
    import plass_amd
    from plass_amd import _lib

    def exports(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
        return {l.split()[-1] for l in out.splitlines() if l.split()[-1].startswith("plasship_") and l.split()[-2] == "T"}

    new = {"plasship_clust_connected_cands", "plasship_clust_connected_alns"}
    assert exports(plass_amd.cc_lib_path()) == {s[0] for s in _lib.CC_SYMBOLS} == new
    # the other four libraries' sets stay what their headers declare
    assert exports(plass_amd.lib_path()) == {s[0] for s in _lib.SYMBOLS + _lib.SYNTH_SYMBOLS + _lib.RCCL_SYMBOLS}
    assert exports(plass_amd.clust_lib_path()) == {s[0] for s in _lib.CLUST_SYMBOLS}
    assert exports(plass_amd.linclust_lib_path()) == {s[0] for s in _lib.LINCLUST_SYMBOLS}
    assert exports(plass_amd.subst_lib_path()) == {s[0] for s in _lib.SUBST_SYMBOLS}
    lib = plass_amd.load_library()
    ext = _lib.load_cc_library()
    assert ext is lib.cc and all(hasattr(ext, s) for s in new)
    header = open(os.path.join(ROOT, "include", "plasship_ext", "cc.h")).read()
    assert all("int %s(" % s in header for s in new)
    assert hasattr(plass_amd.Context, "clust_connected") and plass_amd.CcStats is _lib.CcStats
