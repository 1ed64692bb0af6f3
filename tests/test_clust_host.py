"""clust-greedy and linclust-pre without a GPU: the sequential Python restatement (tests/tools/clust_check.py) against the DBs the unmodified
reference wrote (tests/golden/clust.tar.gz, make_clust.sh: a reference pin, `clust --cluster-mode 3 | 2` and linclust's createsubdb / filterdb
subset), the new command lines in dry run, the wrapper's opt-in routing, the exported symbols."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import clust_check as cc  # noqa: E402

EXE = os.path.join(ROOT, "plass_amd", "plass-hip")
WRAPPER = os.path.join(ROOT, "plass_amd", "plass-gpu-wrapper")
# linclust's clust call as `penguin guided_nuclassemble` makes it (Linclust.cpp:67-76 picks GREEDY_MEM for --cov-mode 1; Parameters.cpp:415-420)
CLUST = ["--cluster-mode", "3", "--max-iterations", "1000", "--similarity-type", "2", "--threads", "4", "--compressed", "0", "-v", "3"]
KMER = ["--sub-mat", "nucl:nucleotide.out,aa:blosum62.out", "--alph-size", "nucl:5,aa:13", "--min-seq-id", "0.97", "--kmer-per-seq", "60", "--spaced-kmer-mode", "0",
        "--kmer-per-seq-scale", "0.100", "--adjust-kmer-len", "0", "--mask", "0", "--mask-lower-case", "0", "--cov-mode", "1", "-k", "22", "-c", "0.99",
        "--max-seq-len", "200000", "--hash-shift", "67", "--split-memory-limit", "0", "--include-only-extendable", "0", "--ignore-multi-kmer", "1"]
HAMMING = ["--rescore-mode", "0", "--wrapped-scoring", "1", "--filter-hits", "0", "-e", "0.001", "-a", "0", "--min-aln-len", "0", "--seq-id-mode", "0",
           "--add-self-matches", "0", "--sort-results", "0", "--db-load-mode", "0"]


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return cc.extract_fixtures(tmp_path_factory.mktemp("clust"))


def _runs(root):
    return [l.split("\t") for l in open(os.path.join(root, "clust", "RUNS")).read().splitlines()]


def _subsets(root):
    return [l.split("\t") for l in open(os.path.join(root, "clust", "SUBSETS")).read().splitlines()]


def test_restatement_equals_the_reference_byte_for_byte(root):
    runs = _runs(root)
    assert len(runs) == 10
    seen = set()
    for name, db, res, flags in runs:
        assert cc.parse_cluster_mode(flags) in (2, 3), name
        ent = cc.clust(os.path.join(root, db), os.path.join(root, res))
        data, index = cc.cluster_db_files(ent)
        ref = os.path.join(root, "clust", "ref", name, "out")
        assert open(ref, "rb").read() == data, name
        assert open(ref + ".index", "rb").read() == index, name
        assert cc.read_db(ref)[1] == 6, name                                 # DBTYPE_CLUSTER_RES
        seen.add((cc.read_db(os.path.join(root, res))[1], cc.read_db(os.path.join(root, db))[1], cc.parse_cluster_mode(flags)))
    # prefilter DBs with and without strands and an alignment DB, nucleotides and proteins, both greedy modes
    assert seen >= {(7, 1, 3), (7, 1, 2), (14, 1, 3), (5, 1, 3), (7, 0, 3)}
    subsets = _subsets(root)
    assert len(subsets) == 2
    for name, db, pref, clu in subsets:
        reps = [k for k, _ in cc.read_db(os.path.join(root, "clust", "ref", clu, "out"))[0]]
        mine = cc.subset_rule(cc.read_db(os.path.join(root, pref))[0], reps)
        ref, ref_type = cc.read_db(os.path.join(root, "clust", "ref", name, "pref_filter2"))
        assert ref_type == cc.read_db(os.path.join(root, pref))[1], name
        assert dict(mine) == dict(ref) and len(mine) == len(ref), name
        assert any(e != dict(cc.read_db(os.path.join(root, pref))[0])[k] for k, e in ref), name      # the filter dropped a line somewhere


def test_fixture_holds_the_cases_that_are_easy_to_get_wrong(root):
    """read off the REFERENCE's files alone"""
    key = {}
    for l in open(os.path.join(root, "clust", "NAMES")):
        db, k, label, n = l.split("\t")
        key[(db, label)] = (int(k), int(n))
    K = lambda label: key[("cases", label)][0]

    def clusters(run):
        return {k: [int(x) for x in e.split()] for k, e in cc.read_db(os.path.join(root, "clust", "ref", run, "out"))[0]}

    for run in ("cases7_m3", "cases7_m2", "cases14_m3", "cases5_m3"):
        c = clusters(run)
        # the chain c -> b -> x -> y with falling lengths: the correction pass promotes b and x, y stays with x
        assert c[K("c")] == [K("c")] and c[K("b")] == [K("b")] and c[K("x")] == [K("x"), K("y")]
        # e is left with d by pass 1, named by m and promoted; d is named by e and was its own representative all along
        assert c[K("e")] == [K("e"), K("m")] and c[K("d")] == [K("d")]
        # an entry listed by nobody with no line of its own, one that lists itself, one that lists a longer target (twice)
        assert c[K("lone")] == [K("lone")] and c[K("selfonly")] == [K("selfonly")] and c[K("short")] == [K("short")]
        assert sum(len(v) for v in c.values()) == 10
    # keys with gaps, and a key order that is not the length order
    lens = [n for (db, _), (k, n) in sorted(key.items(), key=lambda kv: kv[1][0]) if db == "cases"]
    assert lens != sorted(lens, reverse=True) and sorted(k for (db, _), (k, _) in key.items() if db == "cases") != list(range(10))
    # the star: the longest sequence lists all others; its entry starts with its own key, the members follow ascending
    s = clusters("star7_m3")
    assert s == {4: [4, 1, 2, 3, 5, 6]}
    # all lengths equal: the lower key wins
    assert len({n for (db, _), (_, n) in key.items() if db == "equal"}) == 1
    # (3 and 8 list each other: 8 goes to 3; 20 lists 12 and 21 lists 20: a later key never takes an earlier one)
    assert clusters("equal7_m3") == {3: [3, 8], 12: [12], 20: [20], 21: [21]}
    # the Hamming outputs: clusters of more than one member and singletons
    h = clusters("ham_nucl14_linclust_m3")
    assert any(len(v) > 1 for v in h.values()) and any(len(v) == 1 for v in h.values())


def test_restatement_refuses_what_the_reference_refuses(root):
    seq = cc.read_index(os.path.join(root, "clust", "cases"))
    res = cc.read_db(os.path.join(root, "clust", "cases7"))[0]
    with pytest.raises(ValueError, match="Sequence db size != result db size"):
        cc.greedy_low_mem(seq, res[:-1])
    with pytest.raises(ValueError, match="not contained in the sequence database"):
        cc.greedy_low_mem(seq, res[:-1] + [(res[-1][0], b"12345\t0\t0\n")])


def _cli(*args, level="1"):
    p = subprocess.run([EXE] + [str(a) for a in args], env=dict(os.environ, PLASSHIP_CLI_DRYRUN=level), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return p.returncode, p.stdout


def test_command_lines_in_dry_run(root):
    rc, out = _cli("clust-greedy", "db", "pref_rescore1", "pre_clust", *CLUST)
    assert rc == 96 and "clust-greedy accepted (3 positional arguments, 6 flags)" in out
    assert _cli("clust-greedy", "db", "res", "clu", "--cluster-mode", "2")[0] == 96
    # set cover, connected component, the module's default (set cover) and a compressed output are the reference's: 95 before the dry-run exit
    for extra in (["--cluster-mode", "0"], ["--cluster-mode", "1"], [], ["--cluster-mode", "3", "--compressed", "1"]):
        rc, out = _cli("clust-greedy", "db", "res", "clu", *extra)
        assert rc == 95 and "nothing was written" in out, extra
    # the result DB is taken by its dbtype: 7, 14 and 5 run, anything else is the reference's
    for res, want in (("clust/cases7", 96), ("clust/cases14", 96), ("clust/cases5", 96), ("clust/cases", 95), ("clust/ref/cases7_m3/out", 95)):
        assert _cli("clust-greedy", os.path.join(root, "clust", "cases"), os.path.join(root, res), "clu", "--cluster-mode", "3")[0] == want, res
    rc, out = _cli("clust-greedy", "db", "res", "clu", "--cluster-mode", "3", "--no-such-flag", "1")
    assert rc == 1 and "Unrecognized parameter" in out
    assert _cli("clust-greedy", "db", "res", "clu", "--cluster-mode", "3", "-k", "22")[0] == 1           # kmermatcher's flag
    # linclust-pre: the union of the three steps' flags
    rc, out = _cli("linclust-pre", "db", "pre_clust", "pref_filter2", *KMER, *HAMMING, *CLUST, level="2")
    assert rc == 96 and "linclust-pre accepted (3 positional arguments" in out
    flags = dict(l.split(" ", 1) for l in out.splitlines() if l.startswith("flag."))
    assert (flags["flag.k"], flags["flag.kps"], flags["flag.rescoreMode"], flags["flag.wrapped"], flags["flag.covMode"], flags["flag.hashShift"]) == ("22", "60", "0", "1", "1", "67")
    assert abs(float(flags["flag.seqIdThr"]) - 0.97) < 1e-6 and abs(float(flags["flag.covThr"]) - 0.99) < 1e-6 and abs(float(flags["flag.scaleNucl"]) - 0.1) < 1e-6
    base = ["linclust-pre", "db", "pre_clust", "pref_filter2", "-k", "22", "--kmer-per-seq", "60"]
    assert _cli(*base, "--cluster-mode", "2")[0] == 96
    for extra in (["--cluster-mode", "0"], ["--cluster-mode", "1"], [], ["--cluster-mode", "3", "--compressed", "1"], ["--cluster-mode", "3", "--rescore-mode", "3"],
                  ["--cluster-mode", "3", "--spaced-kmer-mode", "1"]):
        assert _cli(*base, *extra)[0] == 95, extra
    assert _cli("linclust-pre", "db", "a", "b", "--cluster-mode", "3")[0] == 95                          # -k and --kmer-per-seq must be given, as for kmermatcher
    assert _cli(*base, "--cluster-mode", "3", "--keep-target", "1")[0] == 1                             # assembleresults' flag
    # the reference's names keep their answer
    for mod in ("clust", "linclust"):
        rc, out = _cli(mod, "a", "b", "c")
        assert rc == 95 and "is not part of the GPU hot path" in out
        assert _cli(mod, "a", "b", "c", *CLUST)[0] == 95


def test_wrapper_routes_clust_only_when_asked(tmp_path):
    ref = tmp_path / "ref"
    ref.write_text("#!/bin/bash\necho \"REF argv0=$0 args=$*\"\n")
    ref.chmod(0o755)
    log = tmp_path / "log"
    base = dict(os.environ, PLASSHIP_CLI_DRYRUN="1", PLASS_REF_BIN=str(ref), PLASS_WRAPPER_LOG=str(log))
    for v in ("PLASS_GPU_CLUST", "PLASS_GPU_HAMMING"):
        base.pop(v, None)
    call = ["clust", "db", "pref_rescore1", "pre_clust"] + CLUST

    def run(args, **env):
        return subprocess.run([WRAPPER] + args, env=dict(base, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)

    # opted in: linclust's call goes to the new command (a dry run: accepted, then the reference computes)
    out = run(call, PLASS_GPU_CLUST="1")
    assert out.returncode == 0 and "clust-greedy accepted" in out.stdout and "args=clust db pref_rescore1 pre_clust --cluster-mode 3" in out.stdout
    # ... what the new command refuses falls back to the reference (set cover: exit 95)
    out = run(["clust", "db", "aln", "clu", "--cluster-mode", "0"], PLASS_GPU_CLUST="1")
    assert out.returncode == 0 and "accepted" not in out.stdout and "args=clust db aln clu --cluster-mode 0" in out.stdout
    # ... an error of the command line is the call's exit code, the reference is not started
    out = run(["clust", "db", "aln", "clu", "--cluster-mode", "3", "--no-such-flag", "1"], PLASS_GPU_CLUST="1")
    assert out.returncode == 1 and "REF" not in out.stdout
    # ... and other modules go where they went
    out = run(["kmermatcher", "db", "pref", "-k", "22", "--kmer-per-seq", "60"], PLASS_GPU_CLUST="1")
    assert "dry run: kmermatcher accepted" in out.stdout
    # not opted in (unset, or anything but 1): clust is not a hot-path module, the reference runs
    for env in ({}, {"PLASS_GPU_CLUST": "0"}, {"PLASS_GPU_HAMMING": "1"}):
        out = run(call, **env)
        assert out.returncode == 0 and "accepted" not in out.stdout and "plass-hip" not in out.stdout and "args=clust db pref_rescore1 pre_clust" in out.stdout
    lines = log.read_text().splitlines()
    assert lines[0].startswith("GPU path   (dry run: clust-greedy accepted, the reference computes) : clust db")
    assert lines[1].startswith("reference  <- plass-hip exit 95 (outside the GPU path) : clust db aln clu")
    assert lines[2].startswith("GPU path   clust-greedy exit 1 : clust")
    assert lines[3].startswith("GPU path   (dry run: accepted, the reference computes) : kmermatcher")
    assert lines[4:] == ["reference  (not a hot-path module) : clust"] * 3


def test_library_exports_the_new_entries():
    import plass_amd
    from plass_amd import _lib
    """the entry points live in the extension library beside libplasship.so, whose own exported set stays what its headers declare"""
    out = subprocess.run(["nm", "-D", "--defined-only", plass_amd.clust_lib_path()], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.split()[-1].startswith("plasship_") and l.split()[-2] == "T"}
    bound = {s[0] for s in _lib.CLUST_SYMBOLS}
    new = {"plasship_clust_greedy_cands", "plasship_clust_greedy_alns", "plasship_clusters_count", "plasship_clusters_download", "plasship_clusters_write",
           "plasship_clusters_free", "plasship_cands_filter"}
    assert exported == bound == new
    lib = plass_amd.load_library()
    assert all(hasattr(lib.clust, s) for s in new)
    assert hasattr(plass_amd.Context, "clust_greedy") and hasattr(plass_amd.Context, "filter_cands") and hasattr(plass_amd, "Clusters")
    header = open(os.path.join(ROOT, "include", "plasship_ext", "clust.h")).read()
    assert all(("int %s(" % s in header) or ("void %s(" % s in header) for s in new)
