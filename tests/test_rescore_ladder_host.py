"""The rescore ladder on the CPU (tests/tools/rescore_ladder.py): for every ladder and flag set the oracle's rescorediagonal must write what
the Python restatement of the reference's --rescore-mode 3 writes, line for line, and the restatement's booleans must show that every
ladder reaches what it is for (a ladder that reaches nothing fails).  tests/test_gpu_rescore_ladder.py runs the same cases on the GPU."""
import os
import shutil
import sys

import numpy as np
import pytest

from conftest import ROOT, read_db, run_oracle

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import rescore_ladder as R  # noqa: E402


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("rescore_ladder")


def _oracle_entries(oracle_bin, d, name, lad, par, keep, copy=False):
    qp, tp, pp = lad.write(d, keep, tag="_" + name)
    if copy:
        tp = qp + "_copy"
        for ext in ("", ".index", ".dbtype"):
            shutil.copy(qp + ext, tp + ext)
    out = os.path.join(str(d), name + "_o_aln")
    run_oracle(oracle_bin, ["rescorediagonal", qp, tp, pp, out] + R.oracle_flags(par))
    dbtype, ent = read_db(out)
    assert dbtype == R.DBTYPE_ALN
    return ent


@pytest.mark.parametrize("name", list(R.CASES))
def test_oracle_writes_what_the_restatement_writes(oracle_bin, workdir, name):
    lad, par, keep, ent, pairs = R.case_restated(name)
    assert len(pairs) == lad.n_lines(keep) > 0, "a pair was left out of the comparison"
    R.assert_same_entries(ent, _oracle_entries(oracle_bin, workdir, name, lad, par, keep), name)


@pytest.mark.parametrize("name,nucl,copy,add_self", [("self_aa_same", 0, False, 0), ("self_nucl_same", 1, False, 0), ("self_aa_copy_self0", 0, True, 0),
                                                     ("self_aa_copy_self1", 0, True, 1), ("self_aa_same_self1", 0, False, 1)])
def test_identity_pairs(oracle_bin, workdir, name, nucl, copy, add_self):
    """the same DB on both sides, and two copies of its files with --add-self-matches 0 / 1 (the reference decides sameQTDB by path)"""
    lad = R.identity(nucl)
    par = R._flags(add_self=add_self)
    ent, pairs = lad.restate(R.numeric(par), same=not copy)
    assert len(pairs) == lad.n_lines()
    selfs = [p for p in pairs if p["q"] == p["t"]]
    assert len(selfs) > 20 and all(p["identity"] == (not copy or bool(add_self)) for p in selfs)
    if not copy or add_self:
        assert all(p["accepted"] for p in selfs)
        assert any(p["score"] == 0 for p in selfs) and {p["cls"] for p in selfs} >= {"self/1thread", "self/16lanes", "self/X", "self/offdiag"}
    else:
        assert any(not p["accepted"] for p in selfs)                 # the X-only sequence against itself: an ordinary pair that scores 0
    assert any(p["accepted"] for p in pairs if p["q"] != p["t"]) and any(not p["accepted"] for p in pairs if p["q"] != p["t"])
    if not nucl:
        assert sum(p["accepted"] for p in pairs if p["q"] == lad.big_query_key) > 64
    R.assert_same_entries(ent, _oracle_entries(oracle_bin, workdir, name, lad, par, None, copy), name)


def _pairs(group):
    return [(n, p) for n in R.GROUPS[group] for p in R.case_restated(n)[4]]


@pytest.mark.parametrize("group", ["geometry", "stars", "reverse", "wraps"])
def test_every_class_has_an_accepted_and_a_rejected_line(group):
    acc, rej = set(), set()
    for _, p in _pairs(group):
        (acc if p["accepted"] else rej).add(p["cls"])
    classes = acc | rej
    never = {"miss"} | {c for c in classes if c.endswith(("/one", "/two"))}          # no diagonal scores above 0: never a line
    classes -= {"tie"}                                                               # (one pair, always a line; its own test below)
    assert (classes - never) - acc == set(), "classes without an accepted line: %s" % sorted((classes - never) - acc)
    assert classes - rej == set(), "classes without a rejected line: %s" % sorted(classes - rej)
    assert not (never & acc) and (group == "wraps" or never & classes)
    for side in ("1thread", "16lanes"):
        assert group == "wraps" or any(c.startswith(side) or ("/" + side + "/") in c for c in classes), side


def test_geometry_reaches_every_overlap_on_both_kernels():
    for nucl in (0, 1):
        lad = R.geometry(nucl)
        seen = set(lad.cls.values())
        for side in ("1thread", "16lanes"):
            for sign in ("pos", "neg"):
                for ov in R.OVERLAPS + ("all",):
                    assert "%s/%s/ov%s" % (side, sign, ov) in seen, (side, sign, ov)
        # the kernel a pair goes to, from its lengths
        for (qk, tk), cls in lad.cls.items():
            if cls[0] in "1":
                side = "1thread" if min(len(lad.q.seq(qk)), len(lad.t.seq(tk))) <= R.RS_SHORT_MAX else "16lanes"
                assert cls.startswith(side)


def test_stars_reach_every_kind():
    _, _, _, _, pairs = R.case_restated("star_aa_open")
    strict = R.case_restated("star_aa_strict")[4]
    for side in ("1thread", "16lanes"):
        for kind in R.STAR_KINDS:
            assert any(p["cls"] == "%s/%s" % (side, kind) for p in strict), (side, kind)
    # a '*' at an end is trimmed: the alignment is shorter than the diagonal
    assert sum(p["aln_len"] == p["diag_len"] - 1 for p in pairs) > 50 and sum(p["aln_len"] == p["diag_len"] - 2 for p in pairs) > 10
    assert all(p["score"] == 0 for p in strict if p["cls"].endswith(("/one", "/two")))


def test_reverse_strand_reaches_the_query_start_and_every_letter():
    lad = R.reverse_strand()
    pairs = R.case_restated("rev_nucl_open")[4]
    assert sum(p["reverse"] for p in pairs) > 1000 and any(not p["reverse"] for p in pairs)
    for side in ("1thread", "16lanes"):
        for k in range(1, 16):
            assert any(p["cls"] == "nearstart/%s/k%d" % (side, k) and p["accepted"] for p in pairs), (side, k)
    # every IUPAC letter, and its lower-case form, in an aligned column of a reverse-strand pair's stored query
    letters = set()
    for p in pairs:
        if p["reverse"] and p["accepted"]:
            q = lad.q.seq(p["q"])
            letters |= set(q.tobytes())
    for ch in R.IUPAC + R.IUPAC.lower():
        assert ch in letters, chr(ch)
    # the complement of every letter: the kernel's table against the reference's two-step mapping
    want = {"A": "T", "C": "G", "M": "G", "Y": "G", "H": "G", "T": "A", "U": "A", "W": "A", "G": "C", "K": "C", "B": "C", "D": "C", "V": "C", "R": "C", "S": "C", "N": "X"}
    tab = R.revcomp_table()
    for a, b in want.items():
        assert chr(tab[ord(a)]) == b and chr(tab[ord(a.lower())]) == b


def test_every_wrap_wins_and_ties_go_to_the_first():
    for name in ("wrap_fwd_strict", "wrap_rev_strict"):
        lad, _, _, _, pairs = R.case_restated(name)
        won = {}
        for p in pairs:
            q_len, t_len = len(lad.q.seq(p["q"])), len(lad.t.seq(p["t"]))
            won.setdefault((q_len, t_len), set()).add(p["wrap"])
            if p["cls"].startswith("wrap/"):
                assert p["wrap"] in (-1, int(p["cls"].rsplit("w", 1)[1])), p["cls"]           # (-1: an overlap of a few columns that scores 0)
        for q_len, t_len in R.WRAP_SIZES:
            possible = set()
            for d16 in range(0, 65536, 16):
                possible |= set(R.intersecting_wraps(q_len, t_len, d16))
            assert possible and possible <= won[(q_len, t_len)], "(%d, %d): wraps %s never win" % (q_len, t_len, sorted(possible - won[(q_len, t_len)]))
        tie = [p for p in pairs if p["cls"] == "tie"][0]
        assert tie["wrap"] == 0 and tie["accepted"] and tie["diag_len"] == 70000 - 32768
        mat = R.submat(True)
        q, t = lad.q.seq(tie["q"]), lad.t.seq(tie["t"])
        qa = R.reverse_query(q) if tie["reverse"] else q
        assert R.by_diagonal(mat, qa, t, -32768)[2] == R.by_diagonal(mat, qa, t, 32768)[2] == tie["score"] > 0
        later = [p for p in pairs if p["cls"] == "later-wrap-better"][0]
        q, t = lad.q.seq(later["q"]), lad.t.seq(later["t"])
        qa = R.reverse_query(q) if later["reverse"] else q
        assert later["wrap"] == 3 and 0 < R.by_diagonal(mat, qa, t, 1000 - 65536)[2] < later["score"]


def test_every_gate_is_the_only_failing_one_somewhere():
    only, passed = set(), set()
    for _, p in _pairs("gates"):
        g = R.only_failing_gate(p)
        if g:
            only.add(g)
        passed |= {g for g in R.GATES if p.get(g)}
    assert only == set(R.GATES) and passed == set(R.GATES), (only, passed)
    # per flag set of the gate ladder: the gate it is about decides, on the threshold and next to it
    def by(name):
        return R.case_restated("gates_" + name)[4]
    g = R.gates()
    # (the aligned columns of an ids/ pair, cut out for counting)
    lad_q = {qk: g.q.seq(qk)[R.overlap_of(len(g.q.seq(qk)), len(g.t.seq(tk)), {100: 10, 125: 40, 1000: 100}[len(g.t.seq(tk))])[0]:][:{100: 100, 125: 110, 1000: 1000}[len(g.t.seq(tk))]]
             for (qk, tk), c in g.cls.items() if c.startswith("ids/")}
    lad_t = {tk: g.t.seq(tk)[:{100: 100, 125: 110, 1000: 1000}[len(g.t.seq(tk))]] for (qk, tk), c in g.cls.items() if c.startswith("ids/")}
    for mode in range(6):
        for a, b, c in R.COV_RATIOS:
            ps = [p for p in by("cov%d_c%s" % (mode, c)) if p["cls"] == "len/%d:%d" % (a, b)]
            assert any(p["canBeCovered"] for p in ps) and any(not p["canBeCovered"] for p in ps), (mode, c)
            if mode < 3:
                ps = [p for p in by("cov%d_c%s" % (mode, c)) if p["cls"] == "cov/%d:%d" % (a, b) and p["canBeCovered"]]
                assert any(p["hasCov"] for p in ps) and any(R.only_failing_gate(p) == "hasCov" for p in ps), (mode, c)
    # the lowest accepted identity count is the one whose ratio the flag names, the next flag moves it by one
    for name, cls, lowest in (("idmode0_090", "ids/100", 90), ("idmode0_091", "ids/100", 91), ("idmode1_080", "ids/125", 100), ("idmode1_0808", "ids/125", 101),
                              ("idmode2_072", "ids/100", 90), ("idmode2_0728", "ids/100", 91), ("idmode0_090", "ids/1000", 900), ("idmode0_091", "ids/1000", 910)):
        ps = [p for p in by(name) if p["cls"] == cls]
        ids = {(p["q"], p["t"]): int(np.count_nonzero((lad_q[p["q"]] & 0xDF) == (lad_t[p["t"]] & 0xDF))) for p in ps}
        assert min(ids[(p["q"], p["t"])] for p in ps if p["accepted"]) == lowest, name
        assert max(ids[(p["q"], p["t"])] for p in ps if R.only_failing_gate(p) == "hasSeqId") == lowest - 1, name
    acc = {n: {p["cls"] for p in by(n) if p["accepted"] and p["cls"].startswith("alnlen/")} for n in ("alnlen100", "alnlen101")}
    assert acc["alnlen100"] == {"alnlen/100", "alnlen/101"} and acc["alnlen101"] == {"alnlen/101"}, acc
    assert all(e.count(b"M\n") == e.count(b"\n") for e in R.case_restated("gates_backtrace")[3].values())


@pytest.mark.parametrize("nucl", [0, 1])
@pytest.mark.parametrize("big", [0, 1])
def test_egate_scores_straddle_the_minimum_by_one(nucl, big):
    lad = R.egate(nucl, big)
    assert lad.t.residues() == R.E_DB_RESIDUES[big]
    for e in R.E_VALUES:
        pairs = R.case_restated("egate_%s_%d_e%g" % ("nucl" if nucl else "aa", big, e))[4]
        for q_len in R.E_QLENS:
            T0 = lad.thresholds[(q_len, e)]
            mine = [p for p in pairs if p["cls"].startswith("e/%d/%g/" % (q_len, e))]
            assert all(p["score"] == int(p["cls"].rsplit("/", 1)[1]) for p in mine), "a target does not score what it was built for"
            acc, rej = [p["score"] for p in mine if p["accepted"]], [p["score"] for p in mine if not p["accepted"]]
            assert acc and rej and min(acc) == T0 and max(rej) == T0 - 1, (q_len, e, T0, sorted(acc), sorted(rej))
            assert all(R.only_failing_gate(p) == "hasEvalue" for p in mine if not p["accepted"])
            long_side = q_len > R.RS_SHORT_MAX
            assert all((min(q_len, len(lad.t.seq(p["t"]))) > R.RS_SHORT_MAX) == long_side for p in mine)
    if big:
        assert lad.thresholds != R.egate(nucl, 0).thresholds


def test_score_table_entries_the_ladders_rely_on():
    aa, nt = R.submat(False), R.submat(True)
    o = ord
    assert aa[o("A"), o("A")] - aa[o("A"), o("S")] == 3 and aa[o("I"), o("I")] - aa[o("I"), o("V")] == 1 and aa[o("A"), o("A")] == aa[o("I"), o("I")] == 4
    assert aa[o("X"), o("X")] < 0 and aa[o("*"), o("*")] < 0 and (aa[o("a")] == aa[o("A")]).all()
    assert nt[o("A"), o("A")] == 2 and nt[o("A"), o("C")] == -3 and nt[o("N"), o("N")] == -3 and nt[o("u"), o("T")] == 2 and nt[o("k"), o("G")] == 2
    assert np.array_equal(aa, aa.T) and np.array_equal(nt, nt.T)
