"""kmermatcher's group kernels on hand-made buckets at every edge (run with `-m gpu` on an MI355X).

groupLinesKernel<256, 2048, 3> ("narrow"), groupLinesKernel<512, 4096, 4> ("wide") and groupKernel<..., LONG, true> ("long",
PLASSHIP_TUNE_FORCE_LONG=1) are forced onto small DBs whose records are known exactly (tests/tools/group_ladder.py) by
PLASSHIP_TUNE_PART_BITS (bucket bits) and PLASSHIP_TUNE_GROUP_SHAPE.  Every case is one kmermatcher call: the candidate DB equals the CPU
oracle's byte for byte over all keys, n_kmer_records / n_grouped / n_candidates equal its N_k / N_m / N_c, and the fields of the
PLASSHIP_DEBUG_GROUPHIST line equal what the rung exists for (kernel, positions against the registers, distinct keys, sub-passes, neighbour
classes), so a rung that no longer reaches its branch fails.

Reached, by case:
  A  size[narrow|wide-i]      one bucket of C-24 .. C+40 and 3C-3 records (C = 2048 / 4096): `inRegs` on both sides of `n <= GL_RMAX * BLOCK`,
                              the recAt loops and fetch(b + 1, true) behind them
  B  distinct[kernel-i]       one bucket of M-1, M, M+1, 2M+1, 6M keys, each in two sequences (M = 1536 / 3072 / 1536): no retry at M, one at
                              M+1, two at 2M+1, three or more at 6M; the rewind of `written`, the alternating cursors.  These buckets are
                              beyond the registers (2 records per key); distinct_inregs[narrow|wide-i] holds the same M-1, M, M+1 keys in
                              exactly C records, so the retry runs on the register path (phase C of the last sub-pass with the prefetch)
  C  neighbours[bits-shape]   2^14 buckets, three per workgroup: empty>regs, regs>empty, empty>empty, regs>regs, regs>big, big>regs, a hot
                              bucket first and later in a workgroup's range; the same DB at 13 bits (two per workgroup) and at 11 bits (two
                              partition levels, one bucket per workgroup); "long" at 14 bits
  D  head_word[kernel]        equal-length tie (smaller id), the head holding the k-mer twice (smaller position), a head of 32 764 residues
                              against 32 763, head ids 66 000 / 131 200 and member ids up to 131 500, positions 300 and 32 750 (the last window)
  E  filter[kernel-flags]     diagonals queryLen - mLen, + 1, 0, -1 under --include-only-extendable 0 / 1; member lengths on both sides of the
                              coverage threshold of --cov-mode 0, 1 and 2
  golden[bits]                the golden protein and nucleotide kmermatcher cases of test_gpu_parity under PART_BITS 5 and 12
  B  distinct_nucl[kernel-i]  the same five key counts as nucleotide (k = 22): every k-mer in two copies of a 22-base sequence and two of its
                              reverse complement, the identity records of either strand; the NUCL instantiations, `kmer | BIT63` keys
  D  head_word_nucl[kernel]   a head on each strand against a member on each strand (sign of the score and diagonal as restated), and the
                              call's first run (`firstRunKey`, k-mer value 1) with a reverse-strand head and a member on each strand: its
                              forward member is NOT reversed, which any later run with such a head would do

Defects found: none.

Mutations, each built into a copy of the library and run against this file on an MI355X (the 66 protein cases; the nucleotide cases were
added afterwards).  Only what is compared or stored was changed; cases that failed:
  `n < GL_RMAX * BLOCK` for `inRegs`    none: at n == C the bucket takes the recAt loops and computes the same records, so no output can differ;
                                        the edge is pinned through the debug line alone (over_regs == 0 at max_pos == C in size[*-3], size[*-4],
                                        distinct_inregs[*])
  `hMulti` bit taken as `slot & 15`     (set and test) distinct_inregs[narrow|wide-0..2], head_word[narrow], filter[narrow|wide-0,2,3,4]: the
                                        cases that hold keys with ONE member, which a neighbour's bit turns into runs; where every key has two
                                        members (A, B, C) the bit is set anyway
  position ranked before id in the word (the two fields swapped in packing and unpacking alike, so that the decoded id stays an id)
                                        head_word[narrow], head_word[wide], golden[5], golden[12]
  length tie of groupKernel             `>=` for `==` is the same predicate (hLen is the final maximum when phase B reads it); with the length test
                                        taken out: head_word[long]
  `diagonal >= queryLen - mLen`         filter[narrow-1], filter[wide-1], filter[long-1], golden[5], golden[12]
Not run, because they move the index of a store (`out[arena + written + ...]`): no rewind of `written` on a retry (the first attempt's records
stay below the retry's: n_grouped grows in distinct[*-2..4], distinct_inregs[*-2]) and `par` not toggled (a slow wavefront adds a cursor that
sub-pass s + 1 has zeroed: its `written` falls behind, records overwrite each other and slots of the arena keep stale input: distinct[narrow|wide-2..4]).
`> MAXKEYS` against `>=` moves a retry, not an output; distinct[*-1] pins it through max_sub == 1 at exactly M keys."""
import os
import sys

import pytest

from conftest import ROOT, assert_same_db, run_oracle
import test_gpu_parity as P

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import group_ladder as G  # noqa: E402

pytestmark = pytest.mark.gpu

VARS = ("PLASSHIP_TUNE_PART_BITS", "PLASSHIP_TUNE_GROUP_SHAPE", "PLASSHIP_DEBUG_GROUPHIST", "PLASSHIP_TUNE_FORCE_LONG")
KERNEL_ENV = {"narrow": {"PLASSHIP_TUNE_GROUP_SHAPE": "1"}, "wide": {"PLASSHIP_TUNE_GROUP_SHAPE": "2"}, "long": {"PLASSHIP_TUNE_FORCE_LONG": "1"}}
PAIRS = ("empty>regs", "regs>empty", "empty>empty", "regs>regs", "regs>big", "big>regs")


@pytest.fixture(autouse=True)
def _clear(monkeypatch):
    for v in VARS:
        monkeypatch.delenv(v, raising=False)


@pytest.fixture(scope="module")
def ctx():
    import plass_amd
    c = plass_amd.Context(0)
    yield c
    c.close()


class _Oracle:
    """the oracle's kmermatcher, run once per (DB, flags) and shared by the cases of this module"""

    def __init__(self, oracle_bin, d):
        self.bin, self.dir, self.runs = oracle_bin, d, {}

    def run(self, tag, db, flags):
        key = (tag, tuple(sorted(flags.items())))
        if key not in self.runs:
            seq = str(self.dir / (tag + "_seq"))
            if not os.path.exists(seq):
                db.write(seq)
            pref = str(self.dir / ("%s_pref%d" % (tag, len(self.runs))))
            self.runs[key] = (seq, pref, run_oracle(self.bin, ["kmermatcher", seq, pref] + G.oracle_flags(**flags)))
        return self.runs[key]


@pytest.fixture(scope="module")
def oracle(oracle_bin, tmp_path_factory):
    return _Oracle(oracle_bin, tmp_path_factory.mktemp("group_ladder"))


def _case(ctx, oracle, tmp_path, monkeypatch, capfd, tag, db, kernel, bits=None, flags=None):
    """one kmermatcher call under the kernel's switches -> the groupHist line of the call"""
    import plass_amd
    flags = flags or {}
    seq, opref, log = oracle.run(tag, db, flags)
    for k, v in KERNEL_ENV[kernel].items():
        monkeypatch.setenv(k, v)
    if bits is not None:
        monkeypatch.setenv("PLASSHIP_TUNE_PART_BITS", str(bits))
    monkeypatch.setenv("PLASSHIP_DEBUG_GROUPHIST", "1")
    sdb = ctx.read_seqdb(seq)
    capfd.readouterr()
    cands, kst = ctx.kmermatcher(sdb, plass_amd.KmermatchParams(**G.param_kwargs(**flags)))
    err = capfd.readouterr().err
    cands.write(tmp_path / "g_pref")
    cands.free()
    hist = G.group_hist(err)
    print("%s %s bits %r: GPU (N_k, N_m, N_c) = %r, oracle %r\n%s" % (tag, kernel, bits, (kst.n_kmer_records, kst.n_grouped, kst.n_candidates), G.oracle_counts(log), err.strip()))
    assert_same_db(opref, tmp_path / "g_pref", "group ladder %s, %s" % (tag, kernel))
    assert (int(kst.n_kmer_records), int(kst.n_grouped), int(kst.n_candidates)) == G.oracle_counts(log)
    assert kst.record_bytes == (20 if kernel == "long" else 16)
    assert len(hist) == 1 + kst.n_restarts, err
    h = hist[-1]
    assert h["kernel"] == kernel and h["max_keys"] == G.MAX_KEYS[kernel] and h["reg_cap"] == G.REG_CAP.get(kernel, 0)
    assert h["records"] == G.oracle_counts(log)[0]
    if bits is not None:
        assert h["buckets"] == 1 << bits
    return h


# ---- A: size against the registers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(9))
@pytest.mark.parametrize("shape", ["narrow", "wide"])
def test_size(ctx, oracle, tmp_path, monkeypatch, capfd, shape, i):
    C = G.REG_CAP[shape]
    records = G.size_steps(C)[i]
    h = _case(ctx, oracle, tmp_path, monkeypatch, capfd, "size%d" % records, G.size_db(records), shape, bits=0)
    pos = (records + G.RPL - 1) // G.RPL * G.RPL                       # every record slot of these DBs is used: whole lines but the last
    assert h["max_pos"] == pos and h["over_regs"] == int(pos > C) and h["bpb"] == 1
    assert h["max_sub"] == 1 and h["multi_sub"] == 0 and h["max_distinct"] == G.size_db(records).distinct
    assert (C - 64 < pos <= C, C < pos <= C + 64, pos == 3 * C) == (i < 5, 5 <= i < 8, i == 8)


# ---- B: distinct keys against MAXKEYS -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(5))
@pytest.mark.parametrize("kernel", ["narrow", "wide", "long"])
def test_distinct(ctx, oracle, tmp_path, monkeypatch, capfd, kernel, i):
    M = G.MAX_KEYS[kernel]
    d = G.distinct_steps(M)[i]
    db = G.distinct_db(d)
    h = _case(ctx, oracle, tmp_path, monkeypatch, capfd, "distinct%d" % d, db, kernel, bits=0)
    sub = G.replay_sub_passes(db.keys, M)
    assert (sub == 1, sub == 2, sub >= 4, sub >= 8) == (i < 2, i == 2, i >= 3, i == 4)
    assert h["max_distinct"] == d and h["max_sub"] == sub and h["multi_sub"] == int(sub > 1)
    if kernel != "long":
        assert h["max_pos"] == (2 * d + G.RPL - 1) // G.RPL * G.RPL and h["over_regs"] == 1        # two records per key: beyond the registers at every step


@pytest.mark.parametrize("i", range(3))
@pytest.mark.parametrize("shape", ["narrow", "wide"])
def test_distinct_inregs(ctx, oracle, tmp_path, monkeypatch, capfd, shape, i):
    M, C = G.MAX_KEYS[shape], G.REG_CAP[shape]
    d = G.distinct_steps(M)[i]
    db = G.distinct_db(d, C)
    h = _case(ctx, oracle, tmp_path, monkeypatch, capfd, "inregs%d_%d" % (d, C), db, shape, bits=0)
    sub = G.replay_sub_passes(db.keys, M)
    assert sub == (2 if i == 2 else 1)
    assert h["max_distinct"] == d and h["max_sub"] == sub and h["multi_sub"] == int(sub > 1) and h["max_pos"] == C and h["over_regs"] == 0


@pytest.mark.parametrize("i", range(5))
@pytest.mark.parametrize("kernel", ["narrow", "wide", "long"])
def test_distinct_nucl(ctx, oracle, tmp_path, monkeypatch, capfd, kernel, i):
    """rung B as nucleotide (k = 22): every k-mer on both strands, the identity records of either strand; NUCL instantiations of the kernels"""
    M = G.MAX_KEYS[kernel]
    d = G.distinct_steps(M)[i]
    db = G.nucl_distinct_db(d)
    h = _case(ctx, oracle, tmp_path, monkeypatch, capfd, "nucl_distinct%d" % d, db, kernel, bits=0, flags=dict(nucl=True))
    sub = G.replay_sub_passes(db.keys, M)
    assert (sub == 1, sub == 2, sub >= 4, sub >= 8) == (i < 2, i == 2, i >= 3, i == 4)
    assert h["max_distinct"] == d and h["max_sub"] == sub and h["multi_sub"] == int(sub > 1) and h["records"] == db.records
    if kernel != "long":
        assert h["max_pos"] == (db.records + G.RPL - 1) // G.RPL * G.RPL and h["over_regs"] == int(db.records > G.REG_CAP[kernel])


@pytest.mark.parametrize("kernel", ["narrow", "wide", "long"])
def test_head_word_nucl(ctx, oracle, tmp_path, monkeypatch, capfd, kernel):
    """rung D as nucleotide: the strand bit of the head word on both strands of head and member, and `firstRunKey` on a run of three"""
    db = G.nucl_head_db()
    h = _case(ctx, oracle, tmp_path, monkeypatch, capfd, "nucl_head", db, kernel, flags=dict(nucl=True))
    assert h["buckets"] == 1 and h["max_distinct"] == db.distinct
    G.check_nucl_heads(db, G.read_pref_lines(tmp_path / "g_pref"))


# ---- C: neighbours inside a workgroup --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,bits", [(k, b) for b in (14, 13, 11) for k in ("narrow", "wide")] + [("long", 14)])
def test_neighbours(ctx, oracle, tmp_path, monkeypatch, capfd, kernel, bits):
    db = G.neighbours_db()
    h = _case(ctx, oracle, tmp_path, monkeypatch, capfd, "neighbours", db, kernel, bits=bits)
    per = {}
    for key in db.keys:
        per.setdefault(G.bucket_of(key, bits), set()).add(key)
    assert h["max_distinct"] == max(len(v) for v in per.values())
    assert h["max_sub"] == max(G.replay_sub_passes(v, G.MAX_KEYS[kernel]) for v in per.values()) == 1 and h["multi_sub"] == 0
    assert h["max_pos"] >= G.HOT_COPIES > G.REG_CAP["wide"]
    if kernel != "long":
        assert h["over_regs"] == 2 * len(db.hot) == h["big_first"] + h["big_later"]
    if bits == 11:                      # two levels (more than 10 bits), one bucket per workgroup: no neighbours
        assert h["bpb"] == 1 and not any(h["pairs"].values())
        return
    assert h["bpb"] >= 2
    want = [p for p in PAIRS if kernel != "long" or "big" not in p]
    if bits == 14:
        assert all(h["pairs"][p] >= 1 for p in want), h["pairs"]
        if kernel != "long":
            assert h["big_first"] >= 1 and h["big_later"] >= 1
    else:
        assert all(h["pairs"][p] >= 1 for p in want if "big" not in p), h["pairs"]


# ---- D: the run-head word ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["narrow", "wide", "long"])
def test_head_word(ctx, oracle, tmp_path, monkeypatch, capfd, kernel):
    db = G.head_word_db()
    h = _case(ctx, oracle, tmp_path, monkeypatch, capfd, "head_word", db, kernel, flags=dict(multi=0))
    assert h["buckets"] >= 64 and h["max_sub"] == 1
    pref = G.read_pref(tmp_path / "g_pref")
    G.check_heads(db, pref)
    assert pref[66000][5] == G.LAYOUT16_MAX_L - G.K and pref[300][400] == -5 and 131100 in pref[70001] and 200 in pref[131200]


# ---- E: the filter ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", range(len(G.FILTER_FLAGS)))
@pytest.mark.parametrize("kernel", ["narrow", "wide", "long"])
def test_filter(ctx, oracle, tmp_path, monkeypatch, capfd, kernel, f):
    db, flags = G.filter_db(), G.FILTER_FLAGS[f]
    h = _case(ctx, oracle, tmp_path, monkeypatch, capfd, "filter", db, kernel, flags=flags)
    assert h["buckets"] == 1 and h["max_distinct"] == db.distinct


# ---- the golden cases under other geometries ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [5, 12])
def test_golden_cases_under_part_bits(ctx, golden, tmp_path, monkeypatch, bits):
    """PART_BITS 5: the golden sets in 32 buckets; 12: two levels.  (With PART_BITS 0 the golden sets in one bucket take 51 s on an MI355X: the
    sub-passes of one bucket grow with the square of its records.  The one-bucket geometry is covered by rungs A, B, D (nucleotide) and E.)"""
    monkeypatch.setenv("PLASSHIP_TUNE_PART_BITS", str(bits))
    for it in (0, 1, 2):
        P.test_golden_aa_modules(ctx, golden, tmp_path, it)
    for it in (0, 1):
        P.test_golden_nucl_kmermatcher_rescore(ctx, golden, tmp_path, it)
