"""rescorediagonal-subst, linclust-ungapped-prot and clust-repseq without a GPU: the sequential Python restatement of `rescorediagonal
--rescore-mode 1` and of `result2repseq` (tests/tools/subst_check.py) against every DB the unmodified reference wrote (tests/golden/subst.tar.gz),
what the hand-made pairs (tests/tools/subst_cases.py) are meant to show read off the restatement's records, the new command lines in dry run,
the wrapper's opt-in routing and the exported symbols of the new extension library."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, read_db

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import local_cases as lcs  # noqa: E402
import subst_cases as cs  # noqa: E402
import subst_check as sc  # noqa: E402

EXE = os.path.join(ROOT, "plass_amd", "plass-hip")
WRAPPER = os.path.join(ROOT, "plass_amd", "plass-gpu-wrapper")
SUBST = ["--rescore-mode", "1", "--filter-hits", "0", "-e", "0.001", "-c", "0.8", "-a", "0", "--cov-mode", "1", "--min-seq-id", "0.9", "--min-aln-len", "0",
         "--seq-id-mode", "0", "--add-self-matches", "0", "--sort-results", "0", "--db-load-mode", "0", "--threads", "4", "--compressed", "0", "-v", "3"]


@pytest.fixture(scope="module")
def fixture(tmp_path_factory, oracle_bin):
    d = str(tmp_path_factory.mktemp("subst_golden"))
    return d, cs.unpack_fixture(d)


@pytest.fixture(scope="module")
def records(fixture):
    """the restatement on every run of the fixture, computed once: name -> (entries, records)"""
    d, runs = fixture
    return {name: cs.expected(d, db, pref, flags, thr) for name, db, pref, flags, thr in runs}


def test_fixture_holds_the_hand_made_cases(fixture, tmp_path):
    """the reference ran on exactly the DBs the other tests make (make_subst_inputs.py writes them with subst_cases.write_all)"""
    cs.write_all(str(tmp_path))
    cs.write_family(str(tmp_path))
    for name in ("prot", "pref_prot7", "nuclx", "pref_nuclx14", "pref_nuclx7", "fam"):
        assert read_db(tmp_path / "subst" / name) == read_db(os.path.join(fixture[0], "subst", name)), name


def test_restatement_equals_the_reference_byte_for_byte(fixture, records):
    """every `rescorediagonal --rescore-mode 1` DB the unmodified reference wrote: proteins and nucleotides, with and without strands,
    --filter-hits 0 and 1 (the threshold it read from its table, and the (seqid, cov) without a row: threshold 0)"""
    d, runs = fixture
    assert len(runs) == len(cs.RUNS) * len(cs.COMBOS) == 40 and sum(thr is not None for *_, thr in runs) == 20 and sum(thr == 0.0 for *_, thr in runs) == 5
    by_filter = by_gates = 0
    for name, db, pref, flags, thr in runs:
        par = sc.parse_flags(flags)
        assert par["rescore_mode"] == 1 and par["filter_hits"] == (thr is not None), name
        want_type, want = read_db(os.path.join(d, "subst", "ref", name, "out"))
        assert want_type == sc.read_db(os.path.join(d, pref))[1] and records[name][0] == want, name
        by_filter += sum(r["by_filter"] and not r["by_gates"] and not r["identity"] for r in records[name][1])
        by_gates += sum(r["by_gates"] and not r["by_filter"] and not r["identity"] for r in records[name][1])
    assert by_filter > 0 and by_gates > 0                     # hasToFilter alone and the third clause alone decided lines of the reference


def test_restatement_equals_the_reference_linclust_run(fixture):
    """the reference's `linclust --alignment-mode 4` on the protein DB, its intermediate DBs kept: the filter step on the subset DB of pre_clust's
    representatives (mode 1 with --filter-hits 1 and the table's threshold, LINCLUST's second line; the E-value counts the subset's residues),
    the alignment step on what it kept, mergeclusters, and result2repseq of the merged clustering"""
    d = fixture[0]
    ref = os.path.join(d, "subst", "ref", "linclust_prot")
    flags, thr = open(os.path.join(d, "subst", "LINCLUST")).read().splitlines()
    seqs, dbtype = sc.read_seqdb(os.path.join(d, "subst", "fam"))
    reps = [int(l) for l in open(os.path.join(ref, "order_redundancy")).read().split()]
    assert dbtype == 0 and 0 < len(reps) < len(seqs)
    ent, pref_type = sc.read_db(os.path.join(ref, "pref_filter2"))
    assert pref_type == 7 and [k for k, _ in ent] == sorted(reps)
    par = sc.parse_flags(flags)
    par.update(rescore_mode=1, thr=float(thr))
    sub = {k: seqs[k] for k in reps}
    out, recs = sc.rescore_subst(sub, False, ent, pref_type, par)
    assert read_db(os.path.join(ref, "pref_rescore2")) == (7, {k: e + b"\0" for k, e in out})
    n_in = sum(e.count(b"\n") for _, e in ent)
    assert 0 < len(recs) < n_in and any(not r["identity"] for r in recs)      # the filter dropped pairs and kept pairs
    par.update(rescore_mode=2)
    aln, _ = sc.lc.rescore_local(sub, False, out, pref_type, par)
    assert read_db(os.path.join(ref, "aln")) == (5, {k: e + b"\0" for k, e in aln})
    first, second = sc.read_db(os.path.join(ref, "pre_clust"))[0], sc.read_db(os.path.join(ref, "clust"))[0]
    merged = sc.lc.merge_clusters(list(seqs), first, second)
    assert read_db(os.path.join(ref, "clu")) == (6, {k: e + b"\0" for k, e in merged})
    assert len(second) < len(first) < len(seqs)               # both steps joined something
    assert read_db(os.path.join(ref, "rep")) == (0, sc.repseqs(dict(sc.read_db(os.path.join(d, "subst", "fam"))[0]), merged))


def test_repseq_restatement_equals_the_reference_on_the_nucleotide_run(fixture):
    d = fixture[0]
    clu = sc.read_db(os.path.join(d, "local", "ref", "linclust", "clu"))[0]
    want = read_db(os.path.join(d, "subst", "ref", "rep_nucl", "rep"))
    assert want == (1, sc.repseqs(dict(sc.read_db(os.path.join(d, "local", "nucl"))[0]), clu)) and len(want[1]) == len(clu)
    # the file set: the sequence DBs of the fixture have no header, lookup or source file, so the reference linked nothing
    assert open(os.path.join(d, "subst", "REPFILES")).read().split() == ["linclust_prot/rep", "linclust_prot/rep.dbtype", "linclust_prot/rep.index",
                                                                         "rep_nucl/rep", "rep_nucl/rep.dbtype", "rep_nucl/rep.index"]
    # an empty entry gives no output entry; the first key of the list is taken, not the entry's
    assert sc.repseqs({1: b"AA\n", 2: b"CC\n"}, [(1, b""), (2, b"1\n2\n")]) == {2: b"AA\n\0"}


def _rec(records, cases, run, label):
    q, t = cases.label[label + ".q"], cases.label[label + ".t"]
    return [r for r in records[run][1] if r["query"] == q and r["target"] == t]


def test_cases_show_what_they_are_meant_to(records):
    p, x, n = cs.prot_cases(), cs.nuclx_cases(), lcs.nucl_cases()
    one = lambda run, c, label: (lambda l: (l[0] if len(l) == 1 else pytest.fail("%s %s: %d records" % (run, label, len(l)))))(_rec(records, c, run, label))
    # the overlap lengths on both sides of every width: lane (16), group step (128), wavefront step and hand-over (1024)
    for length in (1, 15, 16, 17, 127, 128, 129, 300, 1023, 1024, 1025, 2049):
        assert one("pref_prot7_fh_norow", p, "len%d" % length)["diag_len"] == length
    for length in (127, 128, 129):
        assert one("pref_nuclx14_lax", x, "len%d" % length)["diag_len"] == length
    for length in (1, 15, 16, 17, 1023, 1024, 1025, 2049):
        assert one("pref_nucl14_fh_norow", n, "len%d" % length)["diag_len"] == length
    # each tier is met: pairs whose shorter sequence is at most GROUP_MAX and pairs beyond it, proteins and nucleotides, either strand
    tier = lambda c, label: min(len(c.seqs[c.label[label + ".q"]]), len(c.seqs[c.label[label + ".t"]])) > cs.GROUP_MAX
    assert [tier(p, "len%d" % l) for l in (1023, 1024, 1025)] == [False, False, True] and not tier(p, "mixed_tier")
    assert all(tier(p, "wave_ov%d" % o) and one("pref_prot7_fh_norow", p, "wave_ov%d" % o)["diag_len"] == o for o in (1, 17, 129))
    assert not tier(x, "rev333") and tier(x, "rev1301") and tier(x, "rev_shift") and all(one("pref_nuclx14_lax", x, l)["reversed"] for l in ("rev333", "rev1301", "rev_shift"))
    assert not _rec(records, x, "pref_nuclx7_lax", "rev1301")          # (without strands the pair scores nothing worth keeping)
    # the best segment wherever it lies scores the same; reached twice it is still that score
    s = one("pref_prot7_lax", p, "first")["raw_score"]
    assert s > 100 and all(one("pref_prot7_lax", p, l)["raw_score"] == s for l in ("last", "gstep", "wstep", "twice", "twice_wave"))
    # a running score that falls to exactly 0 and recovers (+6 -6 repeated, then 20 matches)
    assert all(one("pref_nuclx14_lax", x, l)["raw_score"] == 40 for l in ("zeros_lane", "zeros_group", "zeros_steps"))
    # nothing scores: diagonal 0 whatever the candidate's, NaN per column; kept only as an identity pair, by every run
    k = p.label["allneg.self"]
    for name, _ in cs.RUNS:
        recs = [r for r in records["pref_prot7_" + name][1] if r["query"] == k]
        assert len(recs) == 1 and (recs[0]["raw_score"], recs[0]["diagonal"], recs[0]["diag_len"]) == (0, 0, 0) and np.isnan(recs[0]["per_col"])
        assert not _rec(records, p, "pref_prot7_" + name, "allneg.pair") and not _rec(records, p, "pref_prot7_" + name, "miss")
        assert records["pref_prot7_" + name][0][k] == b"%d\t%d\t0\n\0" % (k, recs[0]["bit_score"])      # (the candidate's diagonal was 1)
    # the third clause alone keeps a pair with --min-seq-id 0 --min-aln-len 0; --min-aln-len 1 drops it (alnLen is 0 in mode 1): identity pairs stay
    r = one("pref_prot7_lax", p, "len300")
    assert r["by_gates"] and not r["by_filter"] and not _rec(records, p, "pref_prot7_alnlen1", "len300")
    assert records["pref_prot7_alnlen1"][1] and all(r["identity"] for r in records["pref_prot7_alnlen1"][1])
    # canBeCovered on its threshold, before anything is scored (0.9 and 0.8)
    assert _rec(records, p, "pref_prot7_fh_target", "cancover_eq") and not _rec(records, p, "pref_prot7_fh_target", "cancover_below")
    assert _rec(records, p, "pref_prot7_fh_lin", "cancover8_eq") and not _rec(records, p, "pref_prot7_fh_lin", "cancover8_below")
    # coverage is the diagonal's length over the sequence length
    assert one("pref_prot7_cov", p, "cov_eq")["diag_len"] == 50 and not _rec(records, p, "pref_prot7_cov", "cov_below") and _rec(records, p, "pref_prot7_lax", "cov_below")
    # the E-value: the ladder is cut between two of its rungs
    kept = [m for m in range(2, 24, 2) if _rec(records, p, "pref_prot7_default", "evalue%d" % m)]
    assert kept and kept == list(range(kept[0], 24, 2)) and kept[0] > 2
    # `*` and `X` score what the matrix says, lower case what upper case does: the whole overlap is the segment, its score the sum of its columns
    mat = sc.sub_mat(False)
    q, t = (np.frombuffer(p.seqs[p.label["xstar." + s]], dtype=np.uint8) for s in "qt")
    assert one("pref_prot7_lax", p, "xstar")["raw_score"] == int(mat[q, t].sum()) == int(mat[q, np.frombuffer(p.seqs[p.label["xstar.t"]].upper(), dtype=np.uint8)].sum())
    assert mat[ord("X"), ord("A")] < 0 and (mat[ord("*")] == mat[ord("X")]).all()      # (the reference maps `*` onto X)
    # the reverse strand has a negative score column
    e = records["pref_nuclx14_lax"][0][x.label["rev333.q"]]
    assert e.split(b"\t")[1].startswith(b"-")
    # the wraps of diagonal 100 on 70 000 residues: the tie goes to the first wrap tried (the short overlap of -65436: coverage fails),
    # a strictly better third one wins (65636); the printed diagonal is the 16-bit truncation either way
    r = one("pref_nucl14_lax", n, "wrap_tie")
    assert (r["diagonal"], r["raw_score"], r["diag_len"]) == (100 - 65536, 100, 70000 - 65436) and not _rec(records, n, "pref_nucl14_cov", "wrap_tie")
    r = one("pref_nucl14_lax", n, "wrap_third")
    assert (r["diagonal"], r["raw_score"], r["diag_len"]) == (65636, 160, 70000 - 65636)
    for label in ("wrap_tie", "wrap_third"):
        assert records["pref_nucl14_lax"][0][n.label[label + ".q"]].endswith(b"\t100\n\0")


def test_threshold_and_evalue_gates_met_with_equality(fixture):
    """the score per column equal to the threshold is kept, the next float above it as threshold drops the pair; -e equal to the pair's E-value
    keeps it, the next double below drops it (thresholds the reference's table does not hold: the restatement, pinned above, decides)"""
    d = fixture[0]
    p = cs.prot_cases()
    seqs, _ = sc.read_seqdb(os.path.join(d, "subst", "prot"))
    q, t = p.label["len300.q"], p.label["len300.t"]
    pref = [(q, b"%d\t17\t0\n" % t)]
    par = sc.parse_flags("--rescore-mode 1 -e 10 --min-seq-id 0.9 -c 0 --cov-mode 0 --min-aln-len 0 --filter-hits 1")
    par["thr"] = None
    assert not sc.rescore_subst(seqs, False, pref, 7, par)[1]
    par["min_seq_id"] = 0.0
    r = sc.rescore_subst(seqs, False, pref, 7, par)[1][0]
    per_col, evalue = r["per_col"], r["evalue"]
    assert per_col == np.float32(r["raw_score"]) / np.float32(300)
    par["min_seq_id"] = 0.9
    par["thr"] = float(per_col)
    assert len(sc.rescore_subst(seqs, False, pref, 7, par)[1]) == 1
    par["thr"] = float(np.nextafter(per_col, np.float32(np.inf)))
    assert not sc.rescore_subst(seqs, False, pref, 7, par)[1]
    par.update(thr=None, min_seq_id=0.0, e=evalue)
    assert len(sc.rescore_subst(seqs, False, pref, 7, par)[1]) == 1
    par["e"] = float(np.nextafter(evalue, 0.0))
    assert not sc.rescore_subst(seqs, False, pref, 7, par)[1]


def _cli(*args, level="1"):
    p = subprocess.run([EXE] + [str(a) for a in args], env=dict(os.environ, PLASSHIP_CLI_DRYRUN=level), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return p.returncode, p.stdout


def test_command_lines_in_dry_run(fixture):
    d = fixture[0]
    rc, out = _cli("rescorediagonal-subst", "db", "db", "pref_filter2", "pref_rescore2", *SUBST, level="2")
    assert rc == 96 and "rescorediagonal-subst accepted (4 positional arguments" in out
    flags = dict(l.split(" ", 1) for l in out.splitlines() if l.startswith("flag."))
    assert (flags["flag.rescoreMode"], flags["flag.covMode"], flags["flag.filterHits"]) == ("1", "1", "0")
    base = ["rescorediagonal-subst", "db", "db", "pref", "out"]
    assert _cli(*base, "--rescore-mode", "1", "--filter-hits", "1", "--score-per-col-thr", "2.4")[0] == 96
    assert _cli(*base, "--rescore-mode", "1", "--filter-hits", "1", "--score-per-col-thr", "0")[0] == 96
    for extra in (["--rescore-mode", "0"], ["--rescore-mode", "2"], ["--rescore-mode", "3"], ["--rescore-mode", "4"], [], ["--rescore-mode", "1", "--wrapped-scoring", "1"],
                  ["--rescore-mode", "1", "--sort-results", "1"], ["--rescore-mode", "1", "--filter-hits", "1"], ["--rescore-mode", "1", "--compressed", "1"],
                  ["--rescore-mode", "0", "--filter-hits", "1"], ["--rescore-mode", "0", "--filter-hits", "1", "--score-per-col-thr", "2.4"]):
        rc, out = _cli(*base, *extra)
        assert rc == 95 and "nothing was written" in out, extra
    rc, out = _cli("rescorediagonal-subst", "q", "t", "pref", "out", "--rescore-mode", "1")
    assert rc == 95 and "separate query and target DBs" in out
    assert _cli(*base, "--rescore-mode", "1", "--no-such-flag", "1")[0] == 1
    assert _cli(*base, "--rescore-mode", "1", "-k", "14")[0] == 1                                    # kmermatcher's flag
    # the driver: linclust-ungapped's flags
    lin = open(os.path.join(d, "subst", "LINCLUST")).read().splitlines()[0].split()
    lin = [a for i, a in enumerate(lin) if a not in ("--alignment-mode", "--remove-tmp-files") and lin[i - 1] not in ("--alignment-mode", "--remove-tmp-files")]
    base = ["linclust-ungapped-prot", "db", "clu"] + lin
    rc, out = _cli(*base, "--score-per-col-thr", "2.4", level="2")
    assert rc == 96 and "linclust-ungapped-prot accepted (2 positional arguments" in out
    flags = dict(l.split(" ", 1) for l in out.splitlines() if l.startswith("flag."))
    assert (flags["flag.k"], flags["flag.kps"], flags["flag.covMode"], flags["flag.filterHits"]) == ("14", "60", "1", "1")
    assert _cli(*base, "--score-per-col-thr", "2.4", "--rep-out", os.path.join(d, "no_such_rep"))[0] == 96
    assert _cli(*base, "--filter-hits", "0")[0] == 96
    for extra in ([], ["--score-per-col-thr", "2.4", "--wrapped-scoring", "1"], ["--score-per-col-thr", "2.4", "--sort-results", "1"], ["--score-per-col-thr", "2.4", "--rescore-mode", "1"],
                  ["--score-per-col-thr", "2.4", "--cluster-mode", "0"], ["--score-per-col-thr", "2.4", "--compressed", "1"]):
        rc, out = _cli(*base, *extra)
        assert rc == 95 and "nothing was written" in out, extra
    rc, out = _cli("linclust-ungapped-prot", os.path.join(d, "local", "nucl"), "clu", *lin, "--score-per-col-thr", "2.4")
    assert rc == 95 and "linclust-ungapped)" in out
    assert _cli("linclust-ungapped-prot", os.path.join(d, "subst", "fam"), "clu", *lin, "--score-per-col-thr", "2.4")[0] == 96
    rc, out = _cli(*base, "--score-per-col-thr", "2.4", "--rep-out", os.path.join(d, "subst", "fam"))      # an output that exists already
    assert rc == 1 and "exists already" in out
    # --rep-out on the nucleotide driver as well; a protein DB there keeps its answer and names the new driver
    nlin = open(os.path.join(d, "local", "LINCLUST")).read().splitlines()[0].split()
    nlin = [a for i, a in enumerate(nlin) if a not in ("--alignment-mode", "--remove-tmp-files") and nlin[i - 1] not in ("--alignment-mode", "--remove-tmp-files")]
    assert _cli("linclust-ungapped", "db", "clu", *nlin, "--score-per-col-thr", "4.5", "--rep-out", "rep")[0] == 96
    rc, out = _cli("linclust-ungapped", os.path.join(d, "subst", "fam"), "clu", *nlin, "--score-per-col-thr", "4.5")
    assert rc == 95 and "protein DB" in out and "linclust-ungapped-prot" in out
    assert _cli("linclust-pre", "db", "a", "b", "--rep-out", "rep")[0] == 1 and _cli("rescorediagonal-local", "db", "db", "p", "o", "--rep-out", "rep")[0] == 1
    # result2repseq under its own name, with that module's flags
    assert _cli("clust-repseq", "db", "clu", "rep", "--db-load-mode", "0", "--compressed", "0", "--threads", "4", "-v", "3")[0] == 96
    assert _cli("clust-repseq", "db", "clu", "rep", "--compressed", "1")[0] == 95
    assert _cli("clust-repseq", "db", "clu", "rep", "--cluster-mode", "2")[0] == 1
    # the previously pinned answers
    for args in (["rescorediagonal", "db", "db", "p", "o", "--rescore-mode", "1"], ["rescorediagonal-hamming", "db", "db", "p", "o", "--rescore-mode", "1"],
                 ["rescorediagonal-local", "db", "db", "p", "o", "--rescore-mode", "1"], ["result2repseq", "a", "b", "c"], ["linclust", "a", "b", "c"]):
        rc, out = _cli(*args)
        assert rc == 95 and "nothing was written" in out, args


def test_wrapper_routes_only_when_asked(tmp_path):
    ref = tmp_path / "ref"
    ref.write_text("#!/bin/bash\necho \"REF argv0=$0 args=$*\"\n")
    ref.chmod(0o755)
    log = tmp_path / "log"
    base = dict(os.environ, PLASSHIP_CLI_DRYRUN="1", PLASS_REF_BIN=str(ref), PLASS_WRAPPER_LOG=str(log))
    for v in ("PLASS_GPU_CLUST", "PLASS_GPU_HAMMING", "PLASS_GPU_LOCAL", "PLASS_GPU_SUBST", "PLASS_GPU_REPSEQ"):
        base.pop(v, None)
    call = ["rescorediagonal", "db", "db", "pref_filter2", "pref_rescore2"] + SUBST
    rep = ["result2repseq", "db", "clu", "rep", "--threads", "4"]

    def run(args, **env):
        return subprocess.run([WRAPPER] + args, env=dict(base, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)

    out = run(call, PLASS_GPU_SUBST="1")
    assert out.returncode == 0 and "rescorediagonal-subst accepted" in out.stdout and "args=rescorediagonal db db pref_filter2 pref_rescore2 --rescore-mode 1" in out.stdout
    # the workflow's own call carries --filter-hits 1 and no threshold: 95, the reference runs
    refused = [a if a != "0" or call[i - 1] != "--filter-hits" else "1" for i, a in enumerate(call)]
    out = run(refused, PLASS_GPU_SUBST="1")
    assert out.returncode == 0 and "accepted" not in out.stdout and "REF" in out.stdout
    out = run(call + ["--no-such-flag", "1"], PLASS_GPU_SUBST="1")
    assert out.returncode == 1 and "REF" not in out.stdout
    out = run(rep, PLASS_GPU_REPSEQ="1")
    assert out.returncode == 0 and "clust-repseq accepted" in out.stdout and "args=result2repseq db clu rep" in out.stdout
    # not opted in, or opted into something else: the reference runs
    for env in ({}, {"PLASS_GPU_SUBST": "0"}, {"PLASS_GPU_LOCAL": "1"}, {"PLASS_GPU_REPSEQ": "1"}):
        out = run(call, **env)
        assert out.returncode == 0 and "accepted" not in out.stdout and "REF" in out.stdout, env
    for env in ({}, {"PLASS_GPU_SUBST": "1"}):
        out = run(rep, **env)
        assert out.returncode == 0 and "accepted" not in out.stdout and "REF" in out.stdout, env
    lines = log.read_text().splitlines()
    assert lines[0].startswith("GPU path   (dry run: rescorediagonal-subst accepted, the reference computes) : rescorediagonal db")
    assert lines[1].startswith("reference  <- plass-hip exit 95 (outside the GPU path) : rescorediagonal db")
    assert lines[2].startswith("GPU path   rescorediagonal-subst exit 1 : rescorediagonal")
    assert lines[3].startswith("GPU path   (dry run: clust-repseq accepted, the reference computes) : result2repseq db")
    assert all(l.startswith("reference  <- plass-hip exit 95 (outside the GPU path) : rescorediagonal") for l in lines[4:8])
    assert all(l.startswith("reference  (not a hot-path module) : result2repseq") for l in lines[8:]) and len(lines) == 10


def test_library_exports_the_new_entries():
    import plass_amd
    from plass_amd import _lib

    def exports(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
        return {l.split()[-1] for l in out.splitlines() if l.split()[-1].startswith("plasship_") and l.split()[-2] == "T"}

    new = {"plasship_rescore_subst", "plasship_rescore_subst_subset", "plasship_clusters_repseqs", "plasship_merged_repseqs"}
    assert exports(plass_amd.subst_lib_path()) == {s[0] for s in _lib.SUBST_SYMBOLS} == new
    # the other three libraries' sets stay what their headers declare
    assert exports(plass_amd.lib_path()) == {s[0] for s in _lib.SYMBOLS + _lib.SYNTH_SYMBOLS + _lib.RCCL_SYMBOLS}
    assert exports(plass_amd.clust_lib_path()) == {s[0] for s in _lib.CLUST_SYMBOLS}
    assert exports(plass_amd.linclust_lib_path()) == {s[0] for s in _lib.LINCLUST_SYMBOLS}
    lib = plass_amd.load_library()
    ext = _lib.load_subst_library()
    assert ext is lib.subst and all(hasattr(ext, s) for s in new)
    header = open(os.path.join(ROOT, "include", "plasship_ext", "subst.h")).read()
    assert all("int %s(" % s in header for s in new)
    assert all(hasattr(plass_amd.Context, m) for m in ("rescore_subst", "repseqs"))
