"""kmermatcher's extraction tiers at every hand-over length (run with `-m gpu` on an MI355X).

kmermatchImpl picks a kernel per sequence by window count, length and consideredRaw, and by record layout, alphabet, k, `allWork`,
--ignore-multi-kmer and the two caches (tests/tools/extract_ladder.py names the deciding lines).  The ladders put three sequences on every
edge and on its neighbours (-1, 0, +1, +2 windows), with overlap partners for each, and every case is one kmermatcher call compared with
the CPU oracle run with the same flags: the candidate DB byte for byte over ALL keys (no rung is left out of any comparison), and
KmermatchStats.n_kmer_records / n_grouped / n_candidates against the oracle's N_k / N_m / N_c, which also see a record that is dropped or
doubled at a position that matches nothing.

Before a GPU result is looked at, the oracle's output alone must show that the ladder reaches what it is for (a ladder that reaches nothing
fails): under the default flags at least ten sequences of every hand-over class take part in a candidate line with another sequence.

Paths a stat shows are asserted (n_scratch_sequences, n_cached_sequences, record_bytes); for the others the length itself is the argument.
The three-pass tier does not hand a sequence on for its LENGTH: beyond 8160 residues it re-stages the sequence in every pass (`resident`,
kmermatch_extract.hpp), so the protein rungs of 8161-9000 residues reach that non-resident path and n_scratch_sequences counts only the
sequences whose candidate set exceeds the last tier's CAP (kps 200, the length-scaled cases, nucleotide rungs from 9650 on).

Found by the ladder: with --ignore-multi-kmer 0 extractKernel sorted the candidates before the selection walk, which the reference does only
with --ignore-multi-kmer 1; a surplus in the threshold bin then kept other windows than the reference (nucleotide rungs of 3094 and 12000
residues under kps 20 / scale 0.3 / hash shift 3: N_m and N_c two short).  The cases `nucl_kps20_scale03_multi0_seed3` and
`multi0_kps10_scale05` hold hundreds of selected windows per rung, so such a surplus is the rule in them.

An edge that is moved DOWN changes no output (tried: `nWin >= 64 * REGS` in extractKernel passes every case): the next tier computes the
same records, and every tier checks its own limit again.  The ladder catches an edge moved UP (tried: `nWin > 64 * REGS + 1` fails ten
cases: the last window of the 257-, 1025- and 3073-window rungs is lost)."""
import os
import sys

import numpy as np
import pytest

from conftest import AA_AS, AA_RS, NUCL_AS, NUCL_RS, ROOT, assert_same_db, read_db, run_oracle

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import extract_ladder as X  # noqa: E402

pytestmark = pytest.mark.gpu

TUNES = ("PLASSHIP_TUNE_ROWTIER", "PLASSHIP_TUNE_FORCE_LONG", "PLASSHIP_TUNE_KMCACHE")


@pytest.fixture(scope="module")
def ctx():
    import plass_amd
    c = plass_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _no_tunes(monkeypatch):
    for t in TUNES:
        monkeypatch.delenv(t, raising=False)


class _Oracle:
    """the oracle's kmermatcher on a ladder, run once per (DB, flags) and shared by the tests of this module"""

    def __init__(self, oracle_bin, d):
        self.bin, self.dir, self.dbs, self.runs = oracle_bin, d, {}, {}

    def seq(self, tag, lad):
        if tag not in self.dbs:
            self.dbs[tag] = lad.write(self.dir / (tag + "_seq"))
        return self.dbs[tag]

    def kmermatcher(self, tag, lad, case):
        key = (tag, case["name"])
        if key not in self.runs:
            seq = self.seq(tag, lad)
            pref = str(self.dir / ("%s_%s_pref" % (tag, case["name"])))
            log = run_oracle(self.bin, ["kmermatcher", seq, pref] + X.oracle_flags(case))
            self.runs[key] = (seq, pref, log)
        return self.runs[key]


@pytest.fixture(scope="module")
def oracle(oracle_bin, tmp_path_factory):
    return _Oracle(oracle_bin, tmp_path_factory.mktemp("ladder"))


def _ladder_tag(case):
    return "%s_k%d_kps%d_s%g" % ("nucl" if case["nucl"] else "aa", case["k"], case["kps"], case["scale"])


def _params(case):
    import plass_amd
    return plass_amd.KmermatchParams(**X.param_kwargs(case))


def _compare(ctx, oracle, case, tmp_path, lad=None, tag=None, record_bytes=None):
    main = lad is None
    lad = lad if lad is not None else X.case_ladder(case)
    tag = tag or _ladder_tag(case)
    seq, opref, log = oracle.kmermatcher(tag, lad, case)
    X.check_conditions(lad, case, opref, log, main)
    db = ctx.read_seqdb(seq)
    cands, kst = ctx.kmermatcher(db, _params(case))
    cands.write(tmp_path / "g_pref")
    print("%s: GPU (N_k, N_m, N_c) = %r, oracle %r, scratch %d, cached %d, restarts %d, record bytes %d" % (
        case["name"], (kst.n_kmer_records, kst.n_grouped, kst.n_candidates), X.oracle_counts(log), kst.n_scratch_sequences, kst.n_cached_sequences,
        kst.n_restarts, kst.record_bytes))
    assert_same_db(opref, tmp_path / "g_pref", "ladder kmermatcher, " + case["name"])
    X.assert_counts(kst, log, case["name"])
    scratch = sum(X.goes_to_scratch(int(L), case["k"], case["kps"], case["scale"], case["nucl"]) for L in lad.lengths)
    assert kst.n_scratch_sequences >= scratch, "sequences whose candidate set exceeds every LDS tier did not take the HBM-scratch launch"
    if record_bytes is not None:
        assert kst.record_bytes == record_bytes
    return db, cands, kst


@pytest.mark.parametrize("name", [c["name"] for c in X.AA_CASES + X.NUCL_CASES])
def test_ladder_kmermatcher_vs_oracle(ctx, oracle, tmp_path, name):
    case = X.CASES[name]
    # nucleotide k > 23: the 24-byte layout on sequences that short (plasship_kmermatch)
    _, cands, kst = _compare(ctx, oracle, case, tmp_path, record_bytes=20 if (case["nucl"] and case["k"] > 23) else 16)
    if name in ("kps200", "kps10_scale05", "nucl_default"):
        assert kst.n_scratch_sequences > 0
    cands.free()


@pytest.mark.parametrize("name,env", [(n, e) for n in ("default", "k10") for e in ("ROWTIER=3", "ROWTIER=2", "FORCE_LONG=1")] + [("nucl_default", "FORCE_LONG=1")])
def test_ladder_under_a_forced_path(ctx, oracle, tmp_path, monkeypatch, name, env):
    """ROWTIER=3: the row kernels' bins (edges at 96 / 128 / 192 windows) and their fall-back queue in front of the 4-scores tier at this
    size; ROWTIER=2: the 4-scores tier takes the whole list; FORCE_LONG=1: the 24-byte layout on the whole ladder (both are read per call)"""
    var, val = env.split("=")
    monkeypatch.setenv("PLASSHIP_TUNE_" + var, val)
    _, cands, _ = _compare(ctx, oracle, X.CASES[name], tmp_path, record_bytes=20 if var == "FORCE_LONG" else 16)
    cands.free()


@pytest.mark.parametrize("L", [X.LAYOUT_SWITCH_L - 1, X.LAYOUT_SWITCH_L, 32766, 32767, 32768])
def test_layout_switch_lengths(ctx, oracle, tmp_path, L):
    """the SHRT_MAX switch of the record layout, decided by the longest ENTRY (L + 2 bytes): 16-byte records up to L = 32764, 24-byte
    ones from 32765; one DB per length, its longest entries a pair of rungs of that length"""
    lad = X.layout_switch_db(L)
    assert int(lad.lengths.max()) == L
    _, cands, _ = _compare(ctx, oracle, X.CASES["default"], tmp_path, lad=lad, tag="switch%d" % L, record_bytes=16 if L < X.LAYOUT_SWITCH_L else 20)
    cands.free()


@pytest.mark.parametrize("name", ["default", "nucl_default"])
def test_ladder_through_the_later_stages(ctx, oracle, tmp_path, name):
    """the long rungs' records mean the same downstream: rescorediagonal and (nucl)assembleresults on the ladder against the oracle"""
    import plass_amd
    case = X.CASES[name]
    nucl = case["nucl"]
    db, cands, _ = _compare(ctx, oracle, case, tmp_path)
    seq, opref, _ = oracle.kmermatcher(_ladder_tag(case), X.case_ladder(case), case)
    run_oracle(oracle.bin, ["rescorediagonal", seq, seq, opref, tmp_path / "o_aln"] + (NUCL_RS if nucl else AA_RS))
    run_oracle(oracle.bin, ["nuclassembleresults" if nucl else "assembleresults", seq, tmp_path / "o_aln", tmp_path / "o_out"] + (NUCL_AS if nucl else AA_AS))
    alns, rst = ctx.rescorediagonal(db, db, cands, plass_amd.RescoreParams(min_seq_id=0.99 if nucl else 0.9))
    alns.write(tmp_path / "g_aln")
    assert_same_db(tmp_path / "o_aln", tmp_path / "g_aln", "ladder rescorediagonal, " + name)
    out, ast = ctx.assembleresults(db, alns, plass_amd.AssembleParams(min_seq_id=0.99, max_seq_len=200000) if nucl else plass_amd.AssembleParams(min_seq_id=0.9))
    out.write(tmp_path / "g_out")
    assert_same_db(tmp_path / "o_out", tmp_path / "g_out", "ladder assembleresults, " + name)
    assert ast.n_extended > 0


SEED68 = dict(X.CASES["default"], name="default_seed68", hash_shift=68)


@pytest.mark.parametrize("name", ["default_seed68", "nucl_default"])
@pytest.mark.parametrize("kmcache", [1, 2])
def test_ladder_second_call_through_the_caches(oracle, tmp_path, monkeypatch, name, kmcache):
    """kmermatcher -> rescorediagonal -> assembleresults on the ladder, then kmermatcher again on the derived DB with the same flags
    (protein: hash shift 68 in both calls): unchanged sequences are served by the selected-window cache (extractCachedKernel) or, for
    nucleotides, the position cache (extractCachedPosKernel).  The second result equals the oracle's on the written derived DB and the
    cache has served sequences; with PLASSHIP_TUNE_KMCACHE=2 the result is the same and nothing is served.  Whether a call writes the
    cache depends on what the context has run before, so each case has a context of its own, with one call ahead of the chain."""
    import plass_amd
    case = SEED68 if name == "default_seed68" else X.CASES[name]
    nucl = case["nucl"]
    lad = X.case_ladder(case)
    seq, opref, log = oracle.kmermatcher(_ladder_tag(case), lad, case)
    X.check_conditions(lad, case, opref, log)
    if kmcache == 2:
        monkeypatch.setenv("PLASSHIP_TUNE_KMCACHE", "2")
    with plass_amd.Context(0) as c:
        db = c.read_seqdb(seq)
        warm, _ = c.kmermatcher(db, _params(case)); warm.free()
        cands, kst = c.kmermatcher(db, _params(case))
        cands.write(tmp_path / "g_pref")
        assert_same_db(opref, tmp_path / "g_pref", "first call, " + name)
        X.assert_counts(kst, log, name + ", first call")
        alns, _ = c.rescorediagonal(db, db, cands, plass_amd.RescoreParams(min_seq_id=0.99 if nucl else 0.9))
        db2, ast = c.assembleresults(db, alns, plass_amd.AssembleParams(min_seq_id=0.99, max_seq_len=200000) if nucl else plass_amd.AssembleParams(min_seq_id=0.9))
        assert ast.n_extended > 0
        db2.write(tmp_path / "seq_1")
        log2 = run_oracle(oracle.bin, ["kmermatcher", tmp_path / "seq_1", tmp_path / "o_pref_1"] + X.oracle_flags(case))
        assert X.oracle_counts(log2)[2] > 0
        cands2, kst2 = c.kmermatcher(db2, _params(case))
        cands2.write(tmp_path / "g_pref_1")
        print("%s, KMCACHE=%d: second call cached %d of %d sequences" % (name, kmcache, kst2.n_cached_sequences, len(lad.seqs)))
        assert_same_db(tmp_path / "o_pref_1", tmp_path / "g_pref_1", "second call on the derived DB, " + name)
        X.assert_counts(kst2, log2, name + ", second call")
        if kmcache == 1:
            assert kst2.n_cached_sequences > 0, "the cache served no sequence: the test does not reach the path it is for"
        else:
            assert kst2.n_cached_sequences == 0


def test_all_work_staged_and_unstaged_short_kernel(ctx, oracle, tmp_path):
    """only reads with nWin <= kps - 1: `allWork`, extractShortFastKernel<…, true, true> (records through LDS); the same reads plus one
    rung of 300 residues: the unstaged variant with the residency pad.  Both equal the oracle, and the reads' candidate lines among
    themselves are the same bytes in both"""
    case = X.CASES["default"]
    a, b = X.all_work_dbs(case["k"], case["kps"])
    assert int(X.windows(a.lengths, case["k"]).max()) <= case["kps"] - 1 and len(a.seqs) > 300
    assert int(b.lengths.max()) == 300 and len(b.seqs) == len(a.seqs) + 1
    reads = {int(k) for k in a.keys}
    among = []
    for tag, lad in (("allwork", a), ("allwork_plus_rung", b)):
        _, cands, kst = _compare(ctx, oracle, case, tmp_path, lad=lad, tag=tag, record_bytes=16)
        _, ent = read_db(tmp_path / "g_pref")
        among.append({k: [l for l in ent[k].split(b"\n") if l and l != b"\0" and int(l.split(b"\t", 1)[0]) in reads] for k in reads})
        cands.free()
    assert among[0] == among[1]
    assert sum(len(v) > 1 for v in among[0].values()) > 100         # (the first line of an entry is the query itself)
