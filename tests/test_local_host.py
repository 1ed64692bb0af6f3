"""rescorediagonal-local without a GPU: the sequential Python restatement of `rescorediagonal --rescore-mode 2` (tests/tools/local_check.py)
against the CPU oracle's restatement of the same reference code on hand-made pairs at the kernel's edges (tests/tools/local_cases.py), what
those pairs are meant to show read off the restatement's records, the new command line in dry run, the wrapper's opt-in routing and the
exported symbols of the new extension library."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT, read_db, run_oracle

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import local_cases as cs  # noqa: E402
import local_check as lc  # noqa: E402

EXE = os.path.join(ROOT, "plass_amd", "plass-hip")
WRAPPER = os.path.join(ROOT, "plass_amd", "plass-gpu-wrapper")
LOCAL = ["--rescore-mode", "2", "--filter-hits", "0", "-e", "0.001", "-c", "0.99", "-a", "0", "--cov-mode", "1", "--min-seq-id", "0.97", "--min-aln-len", "0",
         "--seq-id-mode", "0", "--add-self-matches", "0", "--sort-results", "0", "--db-load-mode", "0", "--threads", "4", "--compressed", "0", "-v", "3"]


@pytest.fixture(scope="module")
def root(tmp_path_factory, oracle_bin):
    d = str(tmp_path_factory.mktemp("local"))
    return d, cs.write_all(d)


@pytest.fixture(scope="module")
def expected(root):
    d, _ = root
    return {(db, pref, name): cs.expected(d, db, pref, flags, thr) for db, pref in cs.COMBOS for name, flags, thr in cs.RUNS}


def test_restatement_equals_the_oracle_byte_for_byte(root, expected, oracle_bin, tmp_path):
    d, _ = root
    n = 0
    for db, pref in cs.COMBOS:
        for name, flags, thr in cs.RUNS:
            if thr is not None:
                continue                                   # (--filter-hits: the oracle does not have it)
            out = str(tmp_path / ("%s_%s" % (pref, name)))
            run_oracle(oracle_bin, ["rescorediagonal", os.path.join(d, db), os.path.join(d, db), os.path.join(d, pref), out] + flags.split())
            dbtype, ent = read_db(out)
            assert dbtype == 5 and ent == expected[(db, pref, name)][0], (pref, name)
            n += 1
    assert n == 12


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("local_golden"))
    return (d,) + cs.unpack_fixture(d)


def test_fixture_holds_the_hand_made_cases(root, fixture):
    """the reference ran on exactly the DBs the other tests make (make_local_inputs.py writes them with local_cases.write_all)"""
    d, _ = root
    for name in ("nucl", "prot", "pref_nucl14", "pref_nucl7", "pref_prot7"):
        assert read_db(os.path.join(d, name)) == read_db(os.path.join(fixture[0], "local", name)), name


def test_restatement_equals_the_reference_byte_for_byte(fixture, oracle_bin):
    """every `rescorediagonal --rescore-mode 2` DB the unmodified reference wrote: --filter-hits 0 and 1 (the threshold it read from its
    table, and the (seqid, cov) without a row: threshold 0), -a 0 and 1, --cov-mode 0 and 1, --seq-id-mode 0, 1 and 2, with and without strands"""
    d, runs, _ = fixture
    assert len(runs) == 21 and sum(thr is not None for *_, thr in runs) == 9 and sum(thr == 0.0 for *_, thr in runs) == 3
    kept_by_filter = 0
    for name, db, pref, flags, thr in runs:
        seqs, dbtype = lc.read_seqdb(os.path.join(d, db))
        ent, pref_type = lc.read_db(os.path.join(d, pref))
        par = lc.parse_flags(flags)
        assert par["rescore_mode"] == 2 and par["filter_hits"] == (thr is not None), name
        par["thr"] = thr
        out, recs = lc.rescore_local(seqs, dbtype == 1, ent, pref_type, par)
        want_type, want = read_db(os.path.join(d, "local", "ref", name, "out"))
        assert want_type == 5 and {k: e + b"\0" for k, e in out} == want, name
        if thr is not None:
            par["thr"] = None
            kept_by_filter += len(recs) - len(lc.rescore_local(seqs, dbtype == 1, ent, pref_type, par)[1])
    assert kept_by_filter > 0                                  # hasToFilter decided records of the reference


def test_merge_restatement_equals_the_reference_byte_for_byte(fixture):
    """mergeclusters on a clustering and a second one the reference's `clust` made on the subset DB of its representatives"""
    d, _, merges = fixture
    assert len(merges) == 2
    for name, db, first, second in merges:
        keys = [k for k, _ in lc.read_db(os.path.join(d, db))[0]]
        f, s = lc.read_db(os.path.join(d, first))[0], lc.read_db(os.path.join(d, second))[0]
        want_type, want = read_db(os.path.join(d, "local", "ref", name, "merged"))
        got = lc.merge_clusters(keys, f, s)
        assert want_type == 6 and {k: e + b"\0" for k, e in got} == want, name
        # the merge does something: fewer entries than the first clustering has, none of them empty, every sequence listed once
        assert len(got) == len(s) <= len(f) and sorted(int(l) for _, e in got for l in e.split()) == sorted(keys), name
    assert any(len(lc.read_db(os.path.join(d, m[3]))[0]) < len(lc.read_db(os.path.join(d, m[2]))[0]) for m in merges)


def test_restatement_equals_the_reference_linclust_run(fixture):
    """the reference's `linclust --alignment-mode 4` on the hand-made nucleotide DB, its intermediate DBs kept: the alignment step on the
    subset DB of pre_clust's representatives (mode 2 with --filter-hits 1 and the table's threshold, LINCLUST's second line; the E-value
    counts the subset's residues) and mergeclusters of pre_clust and clust, restated from the DBs before them"""
    d = fixture[0]
    ref = os.path.join(d, "local", "ref", "linclust")
    flags, thr = open(os.path.join(d, "local", "LINCLUST")).read().splitlines()
    seqs, dbtype = lc.read_seqdb(os.path.join(d, "local", "nucl"))
    reps = [int(l) for l in open(os.path.join(ref, "order_redundancy")).read().split()]
    assert dbtype == 1 and 0 < len(reps) < len(seqs)
    ent, pref_type = lc.read_db(os.path.join(ref, "pref_filter2"))
    assert pref_type == 14 and [k for k, _ in ent] == sorted(reps)
    par = lc.parse_flags(flags)
    par.update(rescore_mode=2, thr=float(thr))
    out, _ = lc.rescore_local({k: seqs[k] for k in reps}, True, ent, pref_type, par)
    assert read_db(os.path.join(ref, "aln")) == (5, {k: e + b"\0" for k, e in out})
    first, second = lc.read_db(os.path.join(ref, "pre_clust"))[0], lc.read_db(os.path.join(ref, "clust"))[0]
    got = lc.merge_clusters(list(seqs), first, second)
    assert read_db(os.path.join(ref, "clu")) == (6, {k: e + b"\0" for k, e in got})
    assert len(second) < len(first) < len(seqs)               # both steps joined something


def _rec(expected, cases, run, label, pref="pref_nucl14"):
    q, t = cases.label[label + ".q"], cases.label[label + ".t"]
    return [r for r in expected[("nucl", pref, run)][1] if r["query"] == q and r["target"] == t]


def test_cases_show_what_they_are_meant_to(root, expected):
    _, all_cases = root
    c = all_cases["nucl"]
    one = lambda run, label, pref="pref_nucl14": (lambda l: (l[0] if len(l) == 1 else pytest.fail("%s %s: %d records" % (run, label, len(l)))))(_rec(expected, c, run, label, pref))
    # the overlap lengths around a lane's 16 residues and a step's 1024: the whole overlap is the segment (substitutions inside)
    for n in (15, 16, 17, 1023, 1024, 1025, 2049):
        r = one("lax", "len%d" % n)
        assert (r["q_start"], r["q_end"], r["aln_len"]) == (0, n - 1, n), n
    assert one("filter0", "len1")["raw_score"] == 2 and not _rec(expected, c, "lax", "len1")      # (one column never passes -e)
    # position 0, the last position, across the boundaries
    assert (one("default", "first")["q_start"], one("default", "first")["q_end"]) == (0, 39)
    assert (one("default", "last")["q_start"], one("default", "last")["q_end"]) == (1460, 1499)
    assert (one("default", "step")["q_start"], one("default", "step")["q_end"]) == (1000, 1049)
    assert (one("filter0", "lane")["q_start"], one("filter0", "lane")["q_end"]) == (10, 21)
    # two equal maxima: the earlier one
    for label in ("tie_lane", "tie_wave", "tie_step"):
        r = one("filter0", label)
        assert (r["q_start"], r["q_end"], r["raw_score"]) == (5, 14, 20), label
    # zero-sum prefixes: the start is behind the LAST return to zero
    for label, reps in (("zeros_lane", 2), ("zeros_wave", 30), ("zeros_step", 300)):
        r = one("filter0", label)
        assert (r["q_start"], r["q_end"], r["raw_score"]) == (5 * reps, 5 * reps + 19, 40), label
    # nothing scores: the default constructor's -1 .. -1, alnLen 1; the identity pair is written, the ordinary pair never
    k = c.label["allneg.self"]
    for run, _, _ in cs.RUNS:
        recs = [r for r in expected[("nucl", "pref_nucl14", run)][1] if r["query"] == k]
        assert len(recs) == 1 and (recs[0]["raw_score"], recs[0]["q_start"], recs[0]["q_end"], recs[0]["db_start"], recs[0]["db_end"], recs[0]["aln_len"]) == (0, -1, -1, -1, -1, 1)
        assert not _rec(expected, c, run, "allneg.pair") and not _rec(expected, c, run, "miss")
    assert b"\t-1\t-1\t80\t-1\t-1\t80\t1M\n" in expected[("nucl", "pref_nucl14", "lax")][0][k]
    # both signs of the diagonal
    r = one("default", "neg")
    assert (r["diagonal"], r["q_start"], r["db_start"], r["q_end"], r["db_end"]) == (-77, 0, 77, 199, 276)
    r = one("default", "pos")
    assert (r["diagonal"], r["q_start"], r["db_start"], r["q_end"], r["db_end"]) == (31, 31, 0, 230, 199)
    # the wraps of diagonal 100 on 70 000 residues: a tie goes to the first wrap tried, a strictly better third one wins
    r = one("default", "wrap_tie")
    assert (r["diagonal"], r["raw_score"], r["q_start"], r["db_start"]) == (100 - 65536, 100, 200, 65636)
    q, t = (lc.np.frombuffer(c.seqs[c.label["wrap_tie." + x]], dtype=lc.np.uint8) for x in "qt")
    assert lc._by_diagonal(q, t, 100, lc.sub_mat(True))[0] == 100
    r = one("default", "wrap_third")
    assert (r["diagonal"], r["raw_score"], r["q_start"], r["db_start"]) == (65636, 160, 66636, 1000)
    # the reverse strand: positions come back flipped (start > end), and only a prefilter DB with strands has one
    r = one("default", "rev")
    assert r["reversed"] == 1 and r["q_start"] > r["q_end"] and r["aln_len"] == 250
    assert not _rec(expected, c, "default", "rev", "pref_nucl7")
    assert one("default", "rev_lower")["seq_id"] == 1.0 and one("default", "rev_long")["aln_len"] in (400, 401)       # (the planted 400 columns; a random neighbour may match)
    # lower case scores and counts like upper case; N never matches
    r = one("default", "case")
    assert (r["q_start"], r["q_end"], r["raw_score"]) == (0, 119, 2 * 110 - 3 * 10) and r["seq_id"] == lc.F32(110) / lc.F32(120)
    # the gates of run "linclust", each met with equality and missed by one
    for label in ("seqid", "cov", "alnlen", "cancover"):
        assert len(_rec(expected, c, "linclust", label + "_eq")) == 1 and not _rec(expected, c, "linclust", label + "_below"), label
    assert one("linclust", "seqid_eq")["seq_id"] == lc.F32(99) / lc.F32(100)
    # the E-value: the ladder is cut between two of its rungs
    kept = [m for m in range(10, 36) if _rec(expected, c, "default", "evalue%d" % m)]
    assert kept and kept == list(range(kept[0], 36)) and kept[0] > 10
    # --filter-hits: the score per column on the threshold is kept although its gates fail, one column less is not; threshold 0 keeps what scored
    assert not _rec(expected, c, "linclust", "percol_eq")
    assert one("filter1", "percol_eq")["per_col"] == 1.0 and not _rec(expected, c, "filter1", "percol_below")
    assert len(_rec(expected, c, "filter0", "percol_below")) == 1 and not _rec(expected, c, "filter0", "allneg.pair")


def _cli(*args, level="1"):
    p = subprocess.run([EXE] + [str(a) for a in args], env=dict(os.environ, PLASSHIP_CLI_DRYRUN=level), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return p.returncode, p.stdout


def test_command_lines_in_dry_run():
    rc, out = _cli("rescorediagonal-local", "db", "db", "pref_filter2", "aln", *LOCAL, level="2")
    assert rc == 96 and "rescorediagonal-local accepted (4 positional arguments" in out
    flags = dict(l.split(" ", 1) for l in out.splitlines() if l.startswith("flag."))
    assert (flags["flag.rescoreMode"], flags["flag.covMode"], flags["flag.filterHits"], flags["flag.addBt"]) == ("2", "1", "0", "0")
    base = ["rescorediagonal-local", "db", "db", "pref", "aln"]
    assert _cli(*base, "--rescore-mode", "2", "-a", "1")[0] == 96
    assert _cli(*base, "--rescore-mode", "2", "--filter-hits", "1", "--score-per-col-thr", "0.75")[0] == 96
    assert _cli(*base, "--rescore-mode", "2", "--filter-hits", "1", "--score-per-col-thr", "0")[0] == 96
    for extra in (["--rescore-mode", "0"], ["--rescore-mode", "1"], ["--rescore-mode", "3"], ["--rescore-mode", "4"], [], ["--rescore-mode", "2", "--wrapped-scoring", "1"],
                  ["--rescore-mode", "2", "--sort-results", "1"], ["--rescore-mode", "2", "--filter-hits", "1"], ["--rescore-mode", "2", "--compressed", "1"]):
        rc, out = _cli(*base, *extra)
        assert rc == 95 and "nothing was written" in out, extra
    rc, out = _cli("rescorediagonal-local", "q", "t", "pref", "aln", "--rescore-mode", "2")
    assert rc == 95 and "separate query and target DBs" in out
    rc, out = _cli(*base, "--rescore-mode", "2", "--no-such-flag", "1")
    assert rc == 1 and "Unrecognized parameter" in out
    assert _cli(*base, "--rescore-mode", "2", "-k", "22")[0] == 1                                   # kmermatcher's flag
    assert _cli(*base, "--rescore-mode", "2", "-e")[0] == 1                                         # a value is missing
    # our own flag belongs to the new module alone
    for mod in ("rescorediagonal", "rescorediagonal-hamming"):
        assert _cli(mod, "db", "db", "pref", "aln", "--score-per-col-thr", "1")[0] == 1, mod
    # the reference's names keep their answers
    rc, out = _cli("rescorediagonal", "db", "db", "pref", "aln", *LOCAL)
    assert rc == 95 and "--rescore-mode 2 is not part of the GPU path" in out
    for mod in ("mergeclusters", "linclust"):
        rc, out = _cli(mod, "a", "b", "c", "d")
        assert rc == 95 and "is not part of the GPU hot path" in out, mod


def test_merge_and_driver_command_lines_in_dry_run(fixture):
    d = fixture[0]
    assert _cli("mergeclusters-greedy", "db", "out", "clu1", "clu2", "--threads", "4", "--compressed", "0", "-v", "3")[0] == 96
    for clusterings in (["clu1"], ["clu1", "clu2", "clu3"], ["clu1", "clu2", "clu3", "clu4"]):      # the reference merges any number; linclust passes two
        rc, out = _cli("mergeclusters-greedy", "db", "out", *clusterings)
        assert rc == 95 and "nothing was written" in out, clusterings
    assert _cli("mergeclusters-greedy", "db", "out", "clu1", "clu2", "--compressed", "1")[0] == 95
    assert _cli("mergeclusters-greedy", "db", "out", "clu1", "clu2", "--cluster-mode", "3")[0] == 1   # clust's flag
    lin = open(os.path.join(d, "local", "LINCLUST")).read().splitlines()[0].split()
    lin = [a for i, a in enumerate(lin) if a not in ("--alignment-mode", "--remove-tmp-files") and lin[i - 1] not in ("--alignment-mode", "--remove-tmp-files")]
    base = ["linclust-ungapped", "db", "clu"] + lin
    rc, out = _cli(*base, "--score-per-col-thr", "4.5", level="2")
    assert rc == 96 and "linclust-ungapped accepted (2 positional arguments" in out
    flags = dict(l.split(" ", 1) for l in out.splitlines() if l.startswith("flag."))
    assert (flags["flag.k"], flags["flag.kps"], flags["flag.covMode"], flags["flag.filterHits"], flags["flag.ignoreMulti"]) == ("22", "60", "1", "1", "1")
    # the union of linclust-pre's flags and rescorediagonal-local's
    assert _cli(*base, "--score-per-col-thr", "0", "-a", "1", "--seq-id-mode", "1", "--min-aln-len", "10", "--rescore-mode", "2", "--include-only-extendable", "0")[0] == 96
    assert _cli(*base, "--filter-hits", "0")[0] == 96
    for extra in ([], ["--score-per-col-thr", "4.5", "--wrapped-scoring", "1"], ["--score-per-col-thr", "4.5", "--sort-results", "1"], ["--score-per-col-thr", "4.5", "--rescore-mode", "3"],
                  ["--score-per-col-thr", "4.5", "--cluster-mode", "0"], ["--score-per-col-thr", "4.5", "--spaced-kmer-mode", "1"], ["--score-per-col-thr", "4.5", "--compressed", "1"]):
        rc, out = _cli(*base, *extra)
        assert rc == 95 and "nothing was written" in out, extra
    assert _cli("linclust-ungapped", "db", "clu", "--cluster-mode", "3", "--filter-hits", "0")[0] == 95   # -k and --kmer-per-seq must be given, as for kmermatcher
    # a protein DB: the workflow has a filter step more there
    rc, out = _cli("linclust-ungapped", os.path.join(d, "local", "prot"), "clu", *lin, "--score-per-col-thr", "4.5")
    assert rc == 95 and "protein DB" in out
    assert _cli("linclust-ungapped", os.path.join(d, "local", "nucl"), "clu", *lin, "--score-per-col-thr", "4.5")[0] == 96
    assert _cli(*base, "--score-per-col-thr", "4.5", "--keep-target", "1")[0] == 1                      # assembleresults' flag
    for mod in ("mergeclusters", "linclust"):
        assert _cli(mod, "a", "b", "c", "d")[0] == 95, mod


def test_wrapper_routes_mode_2_only_when_asked(tmp_path):
    ref = tmp_path / "ref"
    ref.write_text("#!/bin/bash\necho \"REF argv0=$0 args=$*\"\n")
    ref.chmod(0o755)
    log = tmp_path / "log"
    base = dict(os.environ, PLASSHIP_CLI_DRYRUN="1", PLASS_REF_BIN=str(ref), PLASS_WRAPPER_LOG=str(log))
    for v in ("PLASS_GPU_CLUST", "PLASS_GPU_HAMMING", "PLASS_GPU_LOCAL"):
        base.pop(v, None)
    call = ["rescorediagonal", "db", "db", "pref_filter2", "aln"] + LOCAL

    def run(args, **env):
        return subprocess.run([WRAPPER] + args, env=dict(base, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)

    out = run(call, PLASS_GPU_LOCAL="1")
    assert out.returncode == 0 and "rescorediagonal-local accepted" in out.stdout and "args=rescorediagonal db db pref_filter2 aln --rescore-mode 2" in out.stdout
    # what the new command refuses falls back to the reference: the reference's own --filter-hits 1 carries no threshold
    refused = [a if a != "0" or call[i - 1] != "--filter-hits" else "1" for i, a in enumerate(call)]
    out = run(refused, PLASS_GPU_LOCAL="1")
    assert out.returncode == 0 and "accepted" not in out.stdout and "--filter-hits 1" in out.stdout and "REF" in out.stdout
    # an error of the command line is the call's exit code, the reference is not started
    out = run(call + ["--no-such-flag", "1"], PLASS_GPU_LOCAL="1")
    assert out.returncode == 1 and "REF" not in out.stdout
    # mode 3 goes where it went, mode 0 is not this switch's
    out = run(["rescorediagonal", "db", "db", "pref", "aln", "--rescore-mode", "3"], PLASS_GPU_LOCAL="1")
    assert "dry run: rescorediagonal accepted" in out.stdout
    out = run(["rescorediagonal", "db", "db", "pref", "aln", "--rescore-mode", "0"], PLASS_GPU_LOCAL="1")
    assert "accepted" not in out.stdout and "REF" in out.stdout
    # not opted in: plass-hip rescorediagonal refuses mode 2, the reference runs
    for env in ({}, {"PLASS_GPU_LOCAL": "0"}, {"PLASS_GPU_HAMMING": "1"}):
        out = run(call, **env)
        assert out.returncode == 0 and "accepted" not in out.stdout and "REF" in out.stdout
    lines = log.read_text().splitlines()
    assert lines[0].startswith("GPU path   (dry run: rescorediagonal-local accepted, the reference computes) : rescorediagonal db")
    assert lines[1].startswith("reference  <- plass-hip exit 95 (outside the GPU path) : rescorediagonal db")
    assert lines[2].startswith("GPU path   rescorediagonal-local exit 1 : rescorediagonal")
    assert lines[3].startswith("GPU path   (dry run: accepted, the reference computes) : rescorediagonal")
    assert all(l.startswith("reference  <- plass-hip exit 95 (outside the GPU path) : rescorediagonal") for l in lines[4:]) and len(lines) == 8


def test_library_exports_the_new_entries():
    import plass_amd
    from plass_amd import _lib

    def exports(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
        return {l.split()[-1] for l in out.splitlines() if l.split()[-1].startswith("plasship_") and l.split()[-2] == "T"}

    new = {"plasship_rescore_local", "plasship_rescore_local_subset", "plasship_clusters_merge", "plasship_merged_count", "plasship_merged_download", "plasship_merged_write",
           "plasship_merged_free", "plasship_clusters_read"}
    assert exports(plass_amd.linclust_lib_path()) == {s[0] for s in _lib.LINCLUST_SYMBOLS} == new
    # the other two libraries' sets stay what their headers declare
    assert exports(plass_amd.lib_path()) == {s[0] for s in _lib.SYMBOLS + _lib.SYNTH_SYMBOLS + _lib.RCCL_SYMBOLS}
    assert exports(plass_amd.clust_lib_path()) == {s[0] for s in _lib.CLUST_SYMBOLS}
    lib = plass_amd.load_library()
    ext = _lib.load_linclust_library()
    assert ext is lib.linclust and all(hasattr(ext, s) for s in new) and hasattr(plass_amd.Context, "rescore_local")
    header = open(os.path.join(ROOT, "include", "plasship_ext", "linclust.h")).read()
    assert all("int %s(" % s in header or "void %s(" % s in header for s in new)
    assert all(hasattr(plass_amd.Context, m) for m in ("merge_clusters", "read_clusters"))
