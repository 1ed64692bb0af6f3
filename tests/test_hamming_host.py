"""rescorediagonal-hamming without a GPU: the Python restatement (tests/tools/hamming_check.py) against the DBs the unmodified reference
wrote (tests/golden/hamming.tar.gz, make_hamming.sh), the new command line in dry run, the wrapper's opt-in routing, the exported symbol."""
import os
import subprocess
import sys
import tarfile

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import hamming_check as hc  # noqa: E402

EXE = os.path.join(ROOT, "plass_amd", "plass-hip")
WRAPPER = os.path.join(ROOT, "plass_amd", "plass-gpu-wrapper")
# linclust's Hamming pre-clustering call as `penguin guided_nuclassemble` makes it (profiles/r05_workflow_dropin/*.routing.log)
LINCLUST = ["--sub-mat", "nucl:nucleotide.out,aa:blosum62.out", "--rescore-mode", "0", "--wrapped-scoring", "1", "--filter-hits", "0", "-e", "0.001",
            "-c", "0.99", "-a", "0", "--cov-mode", "1", "--min-seq-id", "0.97", "--min-aln-len", "0", "--seq-id-mode", "0", "--add-self-matches", "0",
            "--sort-results", "0", "--db-load-mode", "0", "--threads", "4", "--compressed", "0", "-v", "3"]


@pytest.fixture(scope="module")
def fixture_root(tmp_path_factory):
    d = tmp_path_factory.mktemp("hamming")
    with tarfile.open(os.path.join(ROOT, "tests", "golden", "hamming.tar.gz")) as t:
        t.extractall(d)
    return os.path.join(str(d), "hamming")


def test_restatement_equals_the_reference_and_every_filter_has_both_outcomes(fixture_root):
    runs = open(os.path.join(fixture_root, "RUNS")).read().splitlines()
    assert len(runs) == 10
    counts, seen = {}, set()
    for line in runs:
        mine, ref, ref_type, pref_type, par = hc.run_fixture_case(fixture_root, line, counts)
        name = line.split("\t")[0]
        assert ref_type == pref_type, name                       # the output keeps the prefilter dbtype (7 or 14)
        assert mine.keys() == ref.keys(), name
        bad = [k for k in ref if mine[k] != ref[k]]
        assert not bad, "%s: %d entries differ, first key %d:\n%r\n%r" % (name, len(bad), bad[0], mine[bad[0]], ref[bad[0]])
        assert any(e == b"" for e in ref.values()) and any(e for e in ref.values()), name     # an empty entry stays an empty entry
        seen.add((line.split("\t")[1], pref_type, par["wrapped"], par["min_seq_id"]))
    # both flag sets, wrapped and not, nucleotide (with and without strands) and protein
    assert seen == {("nucl", 7, 0, 0.97), ("nucl", 7, 1, 0.97), ("nucl", 7, 0, 0.5), ("nucl", 7, 1, 0.5), ("nucl", 14, 0, 0.97), ("nucl", 14, 1, 0.97),
                    ("nucl", 14, 0, 0.5), ("nucl", 14, 1, 0.5), ("prot", 7, 0, 0.97), ("prot", 7, 0, 0.5)}
    # a property of the inputs: every filter lets at least one line pass and drops at least one
    for f in hc.FILTERS:
        assert counts[f][0] >= 1 and counts[f][1] >= 1, (f, counts)


def test_fixture_holds_the_cases_that_are_easy_to_get_wrong(fixture_root):
    """read off the REFERENCE's files alone: the tie between two aliases, the second and third alias, the reverse strand's letters,
    the skipped longer target, the identity pair that fails every threshold"""
    names = {}
    for l in open(os.path.join(fixture_root, "NAMES")):
        db, key, name, n = l.split("\t")
        names[(db, name)] = int(key)
    K = lambda n: names[("nucl", n)]

    def lines(run, q):
        ent, _ = hc.read_db(os.path.join(fixture_root, "ref", run, "out"))
        return [tuple(int(x) for x in l.split()) for l in dict(ent)[K(q)].decode().splitlines()]

    w = "pref_nucl14_linclust_w1"
    # 300 residues planted at two aliases of diagonal 65300 of the 70 000-residue query, 65300 and 70000 - 65536 + 65300 = 69764: both score
    # 300, the first loop's alias is tried first and wins: 69764 & 0xFFFF = 4228 (the second loop's would be printed as 65300 - 65536)
    assert (K("ttie"), 100, 4228) in lines(w, "q70")
    # the second alias of diagonal 1000 (66536 -> printed as 1000) and the third of 500 and 700 (131572, 131772)
    assert (K("t70"), 98, 1000) in lines(w, "q70") and (K("t70rc"), -99, 1000) in lines(w, "q70")
    assert (K("t140"), 99, 500) in lines(w, "q140") and (K("t140s"), 100, 700) in lines(w, "q140")
    # lower case, N and IUPAC codes: the reverse strand is what num2aa[reverseResidue(aa2num[c])] makes of them, not the biological complement
    assert (K("rt_table"), -100, 97 - 11) in lines(w, "rq") and all(t != K("rt_bio") for t, _, _ in lines(w, "rq"))
    # a target one residue longer than the query: no line, in either wrapped run
    for run in (w, "pref_nucl14_loose_w1"):
        assert all(t != K("a17") for t, _, _ in lines(run, "a16"))
    # the identity pair on diagonal 3 of a 17-residue sequence: below every threshold and kept
    for run in ("pref_nucl14_linclust_w0", "pref_nucl14_loose_w0", w):
        (t, score, diag), = lines(run, "a17")
        assert t == K("a17") and score < 50 and diag == 3


def _cli(*args, level="1"):
    p = subprocess.run([EXE] + [str(a) for a in args], env=dict(os.environ, PLASSHIP_CLI_DRYRUN=level), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return p.returncode, p.stdout


def test_command_line_in_dry_run():
    rc, out = _cli("rescorediagonal-hamming", "db", "db", "pref", "pref_rescore1", *LINCLUST, level="2")
    assert rc == 96 and "rescorediagonal-hamming accepted (4 positional arguments" in out
    flags = dict(l.split(" ", 1) for l in out.splitlines() if l.startswith("flag."))
    assert (flags["flag.rescoreMode"], flags["flag.wrapped"], flags["flag.covMode"], flags["flag.minAlnLen"], flags["flag.seqIdMode"]) == ("0", "1", "1", "0", "0")
    assert abs(float(flags["flag.seqIdThr"]) - 0.97) < 1e-6 and abs(float(flags["flag.covThr"]) - 0.99) < 1e-6 and float(flags["flag.evalThr"]) == 0.001
    # the reference's defaults: --rescore-mode 0, no wrapping
    rc, out = _cli("rescorediagonal-hamming", "db", "db", "pref", "out", level="2")
    assert rc == 96 and "flag.rescoreMode 0\n" in out and "flag.wrapped 0\n" in out
    assert _cli("rescorediagonal-hamming", "db", "db", "pref", "out", "--wrapped-scoring", "0")[0] == 96
    # outside the GPU path: exit 95 before the dry-run exit
    assert _cli("rescorediagonal-hamming", "db", "db", "pref", "out", "--rescore-mode", "3")[0] == 95
    assert _cli("rescorediagonal-hamming", "db", "db", "pref", "out", "--rescore-mode", "1")[0] == 95
    assert _cli("rescorediagonal-hamming", "db", "db", "pref", "out", "--filter-hits", "1")[0] == 95
    assert _cli("rescorediagonal-hamming", "db", "db", "pref", "out", "--sort-results", "1")[0] == 95
    assert _cli("rescorediagonal-hamming", "qdb", "tdb", "pref", "out", *LINCLUST)[0] == 95
    rc, out = _cli("rescorediagonal-hamming", "db", "db", "pref", "out", "--no-such-flag", "1")
    assert rc == 1 and "Unrecognized parameter" in out
    assert _cli("rescorediagonal-hamming", "db", "db", "pref", "out", "-k", "22")[0] == 1           # kmermatcher's flag
    # the existing row keeps its answer for the same call
    assert _cli("rescorediagonal", "db", "db", "pref", "out", *LINCLUST)[0] == 95


def test_wrapper_routes_the_hamming_call_only_when_asked(tmp_path):
    ref = tmp_path / "ref"
    ref.write_text("#!/bin/bash\necho \"REF argv0=$0 args=$*\"\n")
    ref.chmod(0o755)
    log = tmp_path / "log"
    base = dict(os.environ, PLASSHIP_CLI_DRYRUN="1", PLASS_REF_BIN=str(ref), PLASS_WRAPPER_LOG=str(log))
    base.pop("PLASS_GPU_HAMMING", None)
    call = ["rescorediagonal", "db", "db", "pref", "pref_rescore1"] + LINCLUST

    def run(args, **env):
        return subprocess.run([WRAPPER] + args, env=dict(base, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)

    # opted in: linclust's call goes to the new command (a dry run: accepted, then the reference computes)
    out = run(call, PLASS_GPU_HAMMING="1")
    assert out.returncode == 0 and "rescorediagonal-hamming accepted" in out.stdout and "args=rescorediagonal db db pref pref_rescore1 --sub-mat" in out.stdout
    # ... a --rescore-mode 3 call still goes to rescorediagonal
    out = run(["rescorediagonal", "db", "db", "pref", "aln", "--rescore-mode", "3", "-e", "1e-5"], PLASS_GPU_HAMMING="1")
    assert "dry run: rescorediagonal accepted" in out.stdout
    # ... and what the new command refuses falls back to the reference (separate DBs: exit 95)
    out = run(["rescorediagonal", "q", "t", "pref", "o", "--rescore-mode", "0"], PLASS_GPU_HAMMING="1")
    assert out.returncode == 0 and "args=rescorediagonal q t pref o --rescore-mode 0" in out.stdout
    # not opted in (unset, or anything but 1): as today, plass-hip rescorediagonal answers 95 and the reference runs
    for env in ({}, {"PLASS_GPU_HAMMING": "0"}):
        out = run(call, **env)
        assert out.returncode == 0 and "accepted" not in out.stdout and "args=rescorediagonal db db pref pref_rescore1" in out.stdout
    lines = log.read_text().splitlines()
    assert lines[0].startswith("GPU path   (dry run: rescorediagonal-hamming accepted")
    assert lines[1].startswith("GPU path   (dry run: accepted, the reference computes) : rescorediagonal")
    assert all(l.startswith("reference  <- plass-hip exit 95 (outside the GPU path) : rescorediagonal") for l in lines[2:]) and len(lines) == 5


def test_library_exports_the_new_entry():
    import plass_amd
    from plass_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", plass_amd.lib_path()], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.split()[-1].startswith("plasship_") and l.split()[-2] == "T"}
    bound = {s[0] for s in _lib.SYMBOLS + _lib.SYNTH_SYMBOLS + _lib.RCCL_SYMBOLS}
    assert "plasship_rescore_hamming" in exported
    assert exported == bound and len(exported) == 56          # the 55 of before and this one
    assert hasattr(plass_amd.Context, "rescore_hamming")
