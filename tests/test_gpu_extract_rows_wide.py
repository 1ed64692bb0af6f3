"""The 32- and 64-lane row kernels of kmermatcher's extraction (kmermatch_extract.hpp section 2e; run with `-m gpu` on an MI355X).

Protein sequences of 257-1024 windows are sorted by window count into three lists for extractRowKernel<10 / 12 / 16, 32> (two sequences per
wavefront; the lists end at 320, 384 and 512 windows) and one for extractRowKernel<16, 64>; a sequence with a surplus in the threshold bin or
a repeated k-mer among its selected windows is queued for the 16-scores tier.  Every case here is a small hand-made DB, one kmermatcher call
with PLASSHIP_TUNE_ROWTIER=3 (rows whatever the size) and one with PLASSHIP_TUNE_ROWTIER=2 (the wave tiers alone), both compared byte for
byte with the CPU oracle's candidate DB and its N_k / N_m / N_c.  The PLASSHIP_DEBUG_ROWTIER line of the first call must name the list sizes
and the number of fall-throughs this file works out on the host: plass_amd/csrc/xxh64_u64.hpp and the reduced alphabet of tables_data.h are
compiled with g++, so the score of every window, the threshold, the selected set, a surplus and a repeat are known before the GPU runs.

A sequence holding X residues does NOT fall through: its windows with an X are invalid (score 0xFFFFFFFF) and the row kernel finishes the
sequence like any other, as the 16-lane rows do.  The cases with X assert exactly that; the repeat among FEW valid windows (all selected,
so the repeat is selected whatever its score) is the X sequence that does reach the fallback."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import AA_AS, AA_RS, ROOT, assert_same_db, run_oracle

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import extract_ladder as X  # noqa: E402

pytestmark = pytest.mark.gpu

K, KPS, SEED = 14, 60, 67
CASE = X.CASES["default"]
assert (CASE["k"], CASE["kps"], CASE["hash_shift"], CASE["alph"], CASE["scale"]) == (K, KPS, SEED, 13, 0.0)
WIDE_BINS = (320, 384, 512)          # kmermatch.hip: ROW_WIDE_BINS; up to 1024 the 64-lane list
TUNES = ("PLASSHIP_TUNE_ROWTIER", "PLASSHIP_TUNE_FORCE_LONG", "PLASSHIP_TUNE_KMCACHE", "PLASSHIP_DEBUG_ROWTIER")
_LINE = re.compile(r"rowTier rows16 (\d+) (\d+) (\d+) (\d+) fell (\d+) rows32 (\d+) (\d+) (\d+) rows64 (\d+) fell (\d+) of (\d+) hist ([\d,]+)")


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


class _Scores:
    """score and k-mer index of every window of a protein sequence, as the kernels compute them"""

    def __init__(self, d):
        src, so = d / "s.cpp", d / "s.so"
        src.write_text('#include "xxh64_u64.hpp"\n#include "tables_data.h"\n'
                       'extern "C" void window_scores(const char *s, int L, int k, unsigned long long seed, unsigned *score, unsigned long long *kmer) {\n'
                       '    const unsigned char *m = PH_AA13_AA2NUM; const unsigned x = m[(int) \'X\'];\n'
                       '    for (int p = 0; p + k <= L; p++) {\n'
                       '        unsigned long long idx = 0, pw = 1; bool ok = true;\n'
                       '        for (int i = 0; i < k; i++) { const unsigned c = m[(unsigned char) s[p + i]]; ok = ok && c != x; idx += c * pw; pw *= 12; }\n'
                       '        kmer[p] = idx; score[p] = ok ? plasship::xxh64Score16(idx, seed) : 0xFFFFFFFFu;\n'
                       '    }\n}\n')
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-w", "-I", os.path.join(ROOT, "plass_amd", "csrc"), str(src), "-o", str(so)])
        self.lib = ctypes.CDLL(str(so))
        self.lib.window_scores.restype = None
        self.lib.window_scores.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_ulonglong, ctypes.c_void_p, ctypes.c_void_p]

    def windows(self, seq):
        n = len(seq) - K + 1
        sc, km = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64)
        self.lib.window_scores(seq.encode(), len(seq), K, SEED, sc.ctypes.data, km.ctypes.data)
        return sc, km

    def outcome(self, seq):
        """(valid windows, surplus in the threshold bin, repeated k-mer among the selected windows): kmermatcher.cpp:224-239 as the row
        kernels restate it — the threshold is the score of the `considered`-th valid window by score, every window at or below it is selected"""
        sc, km = self.windows(seq)
        valid = sc != 0xFFFFFFFF
        n = int(valid.sum())
        considered = min(KPS - 1, n)
        sel = valid if n <= considered else sc <= np.sort(sc[valid])[considered - 1]
        return n, int(sel.sum()) > considered, len(set(km[sel].tolist())) < int(sel.sum())


@pytest.fixture(scope="module")
def scores(tmp_path_factory):
    return _Scores(tmp_path_factory.mktemp("scores"))


def _rand(rng, L):
    return "".join(X.AA_LETTERS[i] for i in rng.integers(0, 20, L))


def _tiles(s):
    """reads of 60 residues over a sequence: its overlap partners (none over a run of X)"""
    return [s[p:p + 60] for p in range(0, len(s) - 59, 25) if s[p:p + 60].count("X") < 30]


def _clean(scores, rng, nw):
    """a random sequence of nw windows without an X that the row kernels finish"""
    while True:
        s = _rand(rng, nw + K - 1)
        n, surplus, repeat = scores.outcome(s)
        if n == nw and not surplus and not repeat:
            return s


def _with_repeat(scores, rng, nw):
    """a 14-mer whose score is low under the seed, twice in a random sequence: both copies are selected, nothing is at the threshold twice"""
    while True:
        w = _rand(rng, K)
        if scores.windows(w)[0][0] < 1500:
            break
    while True:
        s = list(_rand(rng, nw + K - 1))
        s[40:40 + K] = w; s[nw - 60:nw - 60 + K] = w
        s = "".join(s)
        sc, km = scores.windows(s)
        n, surplus, repeat = scores.outcome(s)
        if repeat and not surplus and sc[40] < np.sort(sc)[KPS - 2] and km[40] == km[nw - 60]:
            return s


def _with_surplus(scores, rng, nw):
    """two different k-mers share the threshold score: one window more at the threshold than places left"""
    for _ in range(100000):
        s = _rand(rng, nw + K - 1)
        n, surplus, repeat = scores.outcome(s)
        if surplus and not repeat:
            return s
    raise AssertionError("no sequence with a tie at the threshold found")


def _valid_stretch(scores, rng, nw, n_valid, repeat=False):
    """nw windows of which exactly n_valid hold no X: X everywhere but in one stretch of n_valid + 13 residues (with `repeat`, the stretch
    holds one 14-mer twice, 20 residues apart)"""
    while True:
        body = list(_rand(rng, n_valid + K - 1))
        if repeat:
            body[25:25 + K] = body[5:5 + K]
        s = "X" * 100 + "".join(body) + "X" * (nw + K - 1 - 100 - len(body))
        n, surplus, rep = scores.outcome(s)
        if n == n_valid and rep == repeat and not surplus:
            return s


class _DB(X.Ladder):
    def __init__(self, seqs, seed):
        X.Ladder.__init__(self, False, seqs, [len(s) > 128 for s in seqs], np.random.default_rng(seed))


def _expect(scores, db):
    """what the debug line must say: sizes of the three 32-lane lists, of the 64-lane list, of the 16-lane list of 193-256 windows, and the
    fall-throughs of the 32- and 64-lane launches"""
    nw = X.windows(db.lengths, K)
    lists = [int(((nw > lo) & (nw <= hi)).sum()) for lo, hi in zip((256,) + WIDE_BINS, WIDE_BINS + (1024,))]
    fell = 0
    for s in db.seqs:
        if 256 < len(s) - K + 1 <= 1024:
            _, surplus, repeat = scores.outcome(s)
            fell += surplus or repeat
    return dict(rows32=lists[:3], rows64=lists[3], fell=fell, last16=int(((nw > 192) & (nw <= 256)).sum()))


def _debug(err):
    m = _LINE.findall(err)
    assert m, "no PLASSHIP_DEBUG_ROWTIER line:\n%s" % err
    g = m[-1]
    v = [int(x) for x in g[:11]]
    return dict(rows16=v[0:4], fell16=v[4], rows32=v[5:8], rows64=v[8], fell=v[9], listed=v[10], hist=[int(x) for x in g[11].split(",")])


def _run(ctx, oracle_bin, tmp_path, monkeypatch, capfd, scores, db):
    """the DB through kmermatcher with the rows and with the wave tiers alone, both against the oracle; returns the rows' debug line"""
    import plass_amd
    seq = db.write(tmp_path / "seq")
    log = run_oracle(oracle_bin, ["kmermatcher", seq, str(tmp_path / "o_pref")] + X.oracle_flags(CASE))
    sdb = ctx.read_seqdb(seq)
    monkeypatch.setenv("PLASSHIP_DEBUG_ROWTIER", "1")
    out = {}
    for tier in ("3", "2"):
        monkeypatch.setenv("PLASSHIP_TUNE_ROWTIER", tier)
        capfd.readouterr()
        cands, kst = ctx.kmermatcher(sdb, plass_amd.KmermatchParams(**X.param_kwargs(CASE)))
        out[tier] = capfd.readouterr().err
        cands.write(tmp_path / ("g_pref" + tier))
        cands.free()
        assert_same_db(tmp_path / "o_pref", tmp_path / ("g_pref" + tier), "ROWTIER=" + tier)
        X.assert_counts(kst, log, "ROWTIER=" + tier)
    assert_same_db(tmp_path / "g_pref3", tmp_path / "g_pref2", "rows against the wave tiers")
    assert not _LINE.search(out["2"]), "PLASSHIP_TUNE_ROWTIER=2 ran the row kernels"
    d, want = _debug(out["3"]), _expect(scores, db)
    print("debug line:", d, "expected:", want)
    assert d["rows32"] == want["rows32"] and d["rows64"] == want["rows64"] and d["listed"] == sum(want["rows32"]) + want["rows64"]
    assert d["rows16"][3] == want["last16"]
    assert d["fell"] == want["fell"], "fall-throughs of the 32- and 64-lane launches"
    assert sum(d["hist"]) == d["listed"]
    return d, want


def test_every_edge_of_the_lists(ctx, oracle_bin, tmp_path, monkeypatch, capfd, scores):
    """three rungs on every edge and next to it: 256 / 257 (256 stays with the 16-lane rows), each end of a 32-lane list +- 1, 512 / 513,
    1024 / 1025 (1025 goes to the 48-scores tier: not listed); cut from one genome with reads tiled over it"""
    rng = np.random.default_rng(5)
    genome = X._genome(False, 3200, 31)
    seqs = X._partners(genome, False, rng)
    edges = [e + d for e in (256,) + WIDE_BINS + (1024,) for d in (-1, 0, 1, 2)]
    for nw in edges:
        for _ in range(3):
            p = int(rng.integers(0, len(genome) - (nw + K - 1) + 1))
            seqs.append(genome[p:p + nw + K - 1])
    db = _DB(seqs, 6)
    assert 200 < len(db.seqs) < 600
    d, want = _run(ctx, oracle_bin, tmp_path, monkeypatch, capfd, scores, db)
    assert want["rows32"] == [6 + 6, 6 + 6, 6 + 6] and want["rows64"] == 6 + 6 and want["last16"] == 6
    assert d["hist"][0] >= 6 and d["hist"][23] >= 6


def test_pairs_idle_half_and_fall_throughs(ctx, oracle_bin, tmp_path, monkeypatch, capfd, scores):
    """the first list holds exactly two sequences, of 257 and 320 windows: one wavefront whose halves differ by the full width of the list; the
    second holds an odd number (the last wavefront has an idle half); built to fall through: a repeated low-score 14-mer (32 and 64 lanes), a
    surplus in the threshold bin (32 and 64 lanes), a repeat among 40 valid windows of an X sequence.  Finished by the rows: X residues here
    and there, 40 valid windows (fewer than --kmer-per-seq), exactly 60 valid windows"""
    rng = np.random.default_rng(11)
    wide = [_clean(scores, rng, nw) for nw in (257, 320, 321, 350, 384, 385, 400, 512, 513, 777, 1024)]
    falls = [_with_repeat(scores, rng, 340), _with_repeat(scores, rng, 700), _with_surplus(scores, rng, 345), _with_surplus(scores, rng, 600),
             _valid_stretch(scores, rng, 450, 40, repeat=True)]
    few, sixty = _valid_stretch(scores, rng, 370, 40), _valid_stretch(scores, rng, 640, 60)
    xs = list(_clean(scores, rng, 360))
    for p in (30, 111, 200, 355):
        xs[p] = "X"
    xs = "".join(xs)
    assert scores.outcome(xs)[0] < 360 - 14 and scores.outcome(xs)[1:] == (False, False)
    assert scores.outcome(few) == (40, False, False) and scores.outcome(sixty) == (60, False, False)
    assert all(any(scores.outcome(s)[1:]) for s in falls)
    seqs = wide + falls + [few, sixty, xs]
    seqs = seqs + [t for s in seqs for t in _tiles(s)]
    db = _DB(seqs, 12)
    d, want = _run(ctx, oracle_bin, tmp_path, monkeypatch, capfd, scores, db)
    assert want["rows32"][0] == 2 and want["rows32"][1] % 2 == 1
    assert want["fell"] == len(falls) == 5, "only the sequences built to fall through do"


def test_second_call_reads_the_rows_cache_lines(oracle_bin, tmp_path, monkeypatch, capfd, scores):
    """kmermatcher -> rescorediagonal -> assembleresults -> kmermatcher with one seed: every sequence the thread-per-sequence kernel cannot
    hold has 257-1024 windows, so every selected-window cache line extractCachedKernel reads in the second call was written by the 32- and
    64-lane rows or by their fallback — and the fallback wrote fewer than the cache serves.  The second call equals the oracle's on the
    derived DB and a cold call on another context"""
    import plass_amd
    rng = np.random.default_rng(21)
    genome = X._genome(False, 2500, 32)
    seqs = [s for s in X._partners(genome, False, rng) if len(s) - K + 1 <= KPS - 1]
    for nw in (257, 300, 320, 340, 384, 400, 512, 513, 700, 1024) * 3:
        p = int(rng.integers(0, len(genome) - (nw + K - 1) + 1))
        seqs.append(genome[p:p + nw + K - 1])
    seqs += [_clean(scores, rng, nw) for nw in (280, 290, 330, 500, 600, 900)]       # no partner: nothing extends them
    db = _DB(seqs, 22)
    seq = db.write(tmp_path / "seq")
    monkeypatch.setenv("PLASSHIP_TUNE_ROWTIER", "3")
    monkeypatch.setenv("PLASSHIP_DEBUG_ROWTIER", "1")
    par = plass_amd.KmermatchParams(**X.param_kwargs(CASE))
    with plass_amd.Context(0) as c:
        sdb = c.read_seqdb(seq)
        warm, _ = c.kmermatcher(sdb, par); warm.free()
        capfd.readouterr()
        cands, _ = c.kmermatcher(sdb, par)
        d = _debug(capfd.readouterr().err)
        want = _expect(scores, db)
        assert d["rows32"] == want["rows32"] and d["rows64"] == want["rows64"] and d["fell"] == want["fell"] and d["rows16"][3] == 0
        alns, _ = c.rescorediagonal(sdb, sdb, cands, plass_amd.RescoreParams(min_seq_id=0.9))
        db2, ast = c.assembleresults(sdb, alns, plass_amd.AssembleParams(min_seq_id=0.9))
        assert ast.n_extended > 0
        db2.write(tmp_path / "seq_1")
        log2 = run_oracle(oracle_bin, ["kmermatcher", tmp_path / "seq_1", tmp_path / "o_pref_1"] + X.oracle_flags(CASE))
        cands2, kst2 = c.kmermatcher(db2, par)
        cands2.write(tmp_path / "g_pref_1")
        print("second call: %d sequences from the cache, %d of %d fell through in the first" % (kst2.n_cached_sequences, d["fell"], d["listed"]))
        assert_same_db(tmp_path / "o_pref_1", tmp_path / "g_pref_1", "second call on the derived DB")
        X.assert_counts(kst2, log2, "second call")
        assert kst2.n_cached_sequences > d["fell"] and kst2.n_cached_sequences >= 6
    with plass_amd.Context(0) as c:
        cold, kst3 = c.kmermatcher(c.read_seqdb(tmp_path / "seq_1"), par)
        cold.write(tmp_path / "g_pref_cold")
        assert kst3.n_cached_sequences == 0
        assert_same_db(tmp_path / "g_pref_cold", tmp_path / "g_pref_1", "cached call against a cold call")
