"""plasship_rescore on hand-made candidate pairs at every kernel edge (run with `-m gpu` on an MI355X).

Each case of tests/tools/rescore_ladder.py is read_seqdb, read_prefdb, rescorediagonal, write; the alignment DB must equal the CPU oracle's
byte for byte over ALL keys, RescoreStats.n_scored the number of prefilter lines and n_accepted the number of oracle lines, and with
PLASSHIP_TUNE_LAZY_SELF=2 overlap_residues the restatement's sum of the winning diagonalLen over the pairs that pass canBeCovered.  That
the oracle writes what the reference's text says, and that every ladder reaches its edges, is tests/test_rescore_ladder_host.py (CPU).

The ladders: min(qLen, tLen) of 767-770 (the hand-over at RS_SHORT_MAX = 768) with overlaps of 1-257 columns and the whole sequence on
both signs of the diagonal, sequences of 1-40 residues, a diagonal that misses; '*' at either end, alone, twice and in the middle; the
reverse strand with overlaps that end 1-15 stored residues from the query's start and every IUPAC letter in both cases; sequences up to
140 000 residues with the true diagonal on every +-65536 wrap, a tie between two wraps and a later wrap that is better; --cov-mode 0-5,
--seq-id-mode 0-2, --min-aln-len and -a 1 on their thresholds; the E-value gate on the minimum score and one below it for six query
lengths, two DB sizes and three -e; identity pairs as stubs (the same DB object), as ordinary pairs and under --add-self-matches (two DB
objects), and a queue of 71 alignments through assembleresults.

Defects found: none, on either side: the oracle, the restatement and the kernels write the same bytes in every case.  (The restatement
reads fastSeqIdToBuffer / resultToBuffer as writing "1.00" for an identity of 1, Util.cpp:279-290 with Matcher.cpp:329-330; so does the
oracle.)

Mutations tried on scratch copies of rescore.hip (none committed), each through this module on an MI355X:
  - the tail mask's `nb` shifted by one column: all 64 tests fail;
  - `s.score > bScore` changed to `>=`: 15 fail (the wrap ladders' tie and their pairs with two scoring wraps, both strands);
  - one `minScore` entry (query length 100) off by one: 12 fail (every E-gate case);
  - `rem >= 16` changed to `rem > 16` in fetchQ: nothing fails, and nothing should: the byte-wise branch assembles the same 16 bytes;
  - `nNeg` computed with 65536: nothing fails, and nothing can (below);
  - `last > 0` changed to `last >= 0`: not run on a GPU, because `last` then wraps to 2^32 - 1 on a one-column '*' overlap and the
    kernel would read out of bounds; the same change in the CPU oracle's copy of the expression crashes it on `star_aa_strict`
    (tests/test_rescore_ladder_host.py), as does `>=` for the tie (4 wrap cases differ) while `nNeg` with 65536 changes none of the 57.
Moving RS_SHORT_MAX itself changes no output: both kernels compute the same record, the ladder only makes sure that each of them sees
every geometry.  `nNeg` computed with 65536 instead of 32768 changes no output: the k-th negative wrap
meets the target only if k * 65536 - d16 < tLen, so k <= (tLen + 65534) / 65536 <= 1 + tLen / 65536; the reference's count is generous."""
import os
import shutil
import sys

import pytest

from conftest import ROOT, assert_same_db, read_db, run_oracle, AA_AS

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import rescore_ladder as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import plass_amd
    c = plass_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _no_tunes(monkeypatch):
    monkeypatch.delenv("PLASSHIP_TUNE_LAZY_SELF", raising=False)


class _Oracle:
    """the oracle's rescorediagonal on a ladder, run once per (DB, flags) and shared by the tests of this module"""

    def __init__(self, oracle_bin, d):
        self.bin, self.dir, self.runs = oracle_bin, str(d), {}

    def run(self, name, lad, par, keep=None, copy=False):
        if name not in self.runs:
            qp, tp, pp = lad.write(self.dir, keep, tag="_" + name)
            if copy:
                tp = qp + "_copy"
                for ext in ("", ".index", ".dbtype"):
                    shutil.copy(qp + ext, tp + ext)
            out = os.path.join(self.dir, name + "_o_aln")
            run_oracle(self.bin, ["rescorediagonal", qp, tp, pp, out] + R.oracle_flags(par))
            self.runs[name] = (qp, tp, pp, out)
        return self.runs[name]


@pytest.fixture(scope="module")
def oracle(oracle_bin, tmp_path_factory):
    return _Oracle(oracle_bin, tmp_path_factory.mktemp("rescore_ladder"))


def _oracle_lines(path):
    return sum(e.count(b"\n") for e in read_db(path)[1].values())


def _rescore(ctx, paths, par, tmp_path, what, same_object):
    import plass_amd
    qp, tp, pp, out = paths
    qdb = ctx.read_seqdb(qp)
    tdb = qdb if same_object else ctx.read_seqdb(tp)
    cands = ctx.read_prefdb(qdb, tdb, pp)
    alns, st = ctx.rescorediagonal(qdb, tdb, cands, plass_amd.RescoreParams(**R.param_kwargs(par)))
    alns.write(tmp_path / "g_aln")
    print("%s: scored %d, accepted %d (oracle %d), overlap residues %d, %.3f ms" % (what, st.n_scored, st.n_accepted, _oracle_lines(out), st.overlap_residues, st.ms_kernel))
    assert_same_db(out, tmp_path / "g_aln", "rescore ladder, " + what)
    return qdb, alns, st


@pytest.mark.parametrize("name", list(R.CASES))
def test_ladder_rescorediagonal_vs_oracle(ctx, oracle, tmp_path, monkeypatch, name):
    lad, par, keep, _, pairs = R.case_restated(name)
    paths = oracle.run(name, lad, par, keep)
    monkeypatch.setenv("PLASSHIP_TUNE_LAZY_SELF", "2")            # no stubs (there is no identity pair here): overlap_residues is complete
    _, alns, st = _rescore(ctx, paths, par, tmp_path, name, False)
    assert st.n_scored == lad.n_lines(keep) == len(pairs)
    assert st.n_accepted == _oracle_lines(paths[3]) == sum(p["accepted"] for p in pairs)
    assert st.overlap_residues == sum(p["diag_len"] for p in pairs if p["canBeCovered"])
    alns.free()


@pytest.mark.parametrize("name,nucl,copy,add_self", [("self_aa_same", 0, False, 0), ("self_nucl_same", 1, False, 0), ("self_aa_copy_self0", 0, True, 0),
                                                     ("self_aa_copy_self1", 0, True, 1), ("self_aa_same_self1", 0, False, 1)])
def test_identity_pairs_lazy_and_eager(ctx, oracle, tmp_path, monkeypatch, name, nucl, copy, add_self):
    """identity pairs left as stubs and finished on write (the default) and scored at once (PLASSHIP_TUNE_LAZY_SELF=2): the same bytes, the
    oracle's; self pairs above RS_SHORT_MAX take stub -> long list -> the 16-lane kernel"""
    lad = R.identity(nucl)
    par = R._flags(add_self=add_self)
    _, pairs = lad.restate(R.numeric(par), same=not copy)
    paths = oracle.run(name, lad, par, None, copy)
    for lazy in (None, "2"):
        if lazy:
            monkeypatch.setenv("PLASSHIP_TUNE_LAZY_SELF", lazy)
        _, alns, st = _rescore(ctx, paths, par, tmp_path, "%s, LAZY_SELF=%s" % (name, lazy or "default"), not copy)
        assert st.n_scored == lad.n_lines() and st.n_accepted == _oracle_lines(paths[3]) == sum(p["accepted"] for p in pairs)
        if lazy:
            assert st.overlap_residues == sum(p["diag_len"] for p in pairs if p["canBeCovered"])
        alns.free()


@pytest.mark.parametrize("lazy", [None, "2"])
def test_queue_beyond_64_alignments_through_assembleresults(ctx, oracle, tmp_path, monkeypatch, lazy):
    """a query of 800 residues with 70 overlapping targets and its own line: the stub of a queue beyond 64 alignments is finished for the
    extension kernel (mode 2) on the 16-lane kernel; the assembled DB equals the oracle's"""
    import plass_amd
    lad = R.identity(0)
    par = R._flags()
    qp, _, pp, oaln = oracle.run("self_aa_same", lad, par)
    if lazy:
        monkeypatch.setenv("PLASSHIP_TUNE_LAZY_SELF", lazy)
    qdb = ctx.read_seqdb(qp)
    cands = ctx.read_prefdb(qdb, qdb, pp)
    alns, _ = ctx.rescorediagonal(qdb, qdb, cands, plass_amd.RescoreParams(**R.param_kwargs(par)))
    out, ast = ctx.assembleresults(qdb, alns, plass_amd.AssembleParams(min_seq_id=0.9))          # BEFORE any write: the stubs are still pending
    out.write(tmp_path / "g_out")
    run_oracle(oracle.bin, ["assembleresults", qp, oaln, tmp_path / "o_out"] + AA_AS)
    assert_same_db(tmp_path / "o_out", tmp_path / "g_out", "assembleresults on the identity ladder")
    assert ast.n_extended > 0
    alns.write(tmp_path / "g_aln")
    assert_same_db(oaln, tmp_path / "g_aln", "the alignment list after assembleresults")
