"""The line lists of the k-mer partition (tagScatterRunsKernel, tagSortRegionRunsKernel: linepart.hpp) at their edges (run with `-m gpu` on
an MI355X).

As in test_gpu_linepart_edges.py the DBs are 13-residue protein sequences (tests/tools/group_ladder.py): one sequence is one record, in id
order, and identical sequences share the bucket.  PLASSHIP_TUNE_PART_BITS fixes the geometry: up to 10 bits = one level (3 bits = 8 buckets,
the 512-thread partition kernel), 20 bits = two levels of 1024.  Every case is one kmermatcher call whose candidate DB equals the CPU oracle's
byte for byte with N_k / N_m / N_c equal.  Before that the case states on the host, from the restated hash and the restated piece geometry
(kmermatch.hip: pieceLinesFor, 256 CUs), that its DB has the edge it is named for, and afterwards the PLASSHIP_DEBUG_LINELIST line of the call
must name the same output lines, chunks, regions and largest bucket.

Every debug line names its caller: `hash` (the hash partition of the k-mer records) or `repsort` (the range partition of the grouped records).

The level-1 list kernel walks the partition's OUTPUT lines in chunks of CHUNK = 32 768; their number is pieces * (piece lines + buckets), so
not every count can be reached: CHUNK - 1 cannot (32 767 = 7 * 31 * 151 is no such product for any power-of-two bucket count at 256 CUs:
pieceLinesFor gives 8 * buckets lines per piece below 8192 * buckets input lines, hence multiples of 9 * buckets, and about 1000 pieces above),
the nearest below is CHUNK - 8.  Reached here: CHUNK - 8, CHUNK, CHUNK + 1 and 2 CHUNK + 56 (a tail smaller than a wavefront).  The list
kernels stage whole chunks, not rows; fine buckets of 7, 8, 9 and 40 lines stand where a row of 8 entries would have its edges.
The rep sort takes a second level from 2^18 grouped 24-byte records on: the nucleotide ladder DB of that size takes 2.2 s to build on the host
(measured), the case's kmermatcher call and oracle run come on top.
"""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, assert_same_db, run_oracle

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import group_ladder as G  # noqa: E402

pytestmark = pytest.mark.gpu

VARS = ("PLASSHIP_TUNE_PART_BITS", "PLASSHIP_TUNE_GROUP_SHAPE", "PLASSHIP_DEBUG_LINELIST", "PLASSHIP_TUNE_FORCE_LONG")
CHUNK, CUS, RPL = 32768, 256, G.RPL
_LINE = re.compile(r"lineList (\w+) level (\d) buckets (\d+) lines (\d+) listed (\d+) chunk (\d+) chunks (\d+) regions (\d+) maxBucket (\d+)(?: emptyRegions (\d+) maxRegion (\d+) pieces (\d+))?")


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


@pytest.fixture(scope="module")
def pool():
    """4096 distinct 13-residue words and their identity keys, shared by all cases"""
    words = G._words(np.random.default_rng(77), 4096, G.K - 1, set())
    return words, {w: G.identity_key(w) for w in words}


def make_db(seqs, keyof):
    db = G.GroupDb(seqs, [False] * len(seqs), windows_all=False)
    db.keys = [keyof[s] for s in seqs]
    db.records = len(seqs)
    return db


def geometry(records, nb):
    """level 1 of lineGeometry: (piece lines, pieces, output lines)"""
    lines = -(-records // RPL)
    want = -(-lines // (4 * CUS))
    pl = max(nb * 8, min(nb * 64, max(want, 1)))
    n_p = -(-lines // pl)
    return pl, n_p, n_p * (pl + nb)


def lines_of(keys, bits):
    """lines per final bucket when every level-1 bucket is one level-2 piece and the level-1 input is cut into pieces"""
    per = {}
    for k in keys:
        b = G.bucket_of(k, bits); per[b] = per.get(b, 0) + 1
    return per


def _run(ctx, oracle_bin, tmp_path, monkeypatch, capfd, db, bits, env=None, flags=None, record_bytes=16):
    import plass_amd
    flags = flags or {}
    seq = db.write(tmp_path / "seq")
    log = run_oracle(oracle_bin, ["kmermatcher", seq, str(tmp_path / "o_pref")] + G.oracle_flags(**flags))
    if bits is not None:
        monkeypatch.setenv("PLASSHIP_TUNE_PART_BITS", str(bits))
    monkeypatch.setenv("PLASSHIP_DEBUG_LINELIST", "1")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    sdb = ctx.read_seqdb(seq)
    capfd.readouterr()
    cands, kst = ctx.kmermatcher(sdb, plass_amd.KmermatchParams(**G.param_kwargs(**flags)))
    err = capfd.readouterr().err
    cands.write(tmp_path / "g_pref")
    cands.free()
    got, want = (int(kst.n_kmer_records), int(kst.n_grouped), int(kst.n_candidates)), G.oracle_counts(log)
    print("bits %r, %d records: GPU (N_k, N_m, N_c) = %r, oracle %r" % (bits, db.records, got, want))
    assert_same_db(str(tmp_path / "o_pref"), tmp_path / "g_pref", "line-list edges, %r bits, %d records" % (bits, db.records))
    assert got == want and want[0] == db.records
    assert kst.record_bytes == record_bytes
    out = []
    for m in _LINE.finditer(err):
        names = ("level", "buckets", "lines", "listed", "chunk", "chunks", "regions", "max_bucket", "empty_regions", "max_region", "pieces")
        d = {n: int(v) for n, v in zip(names, m.groups()[1:]) if v is not None}
        d["who"] = m.group(1)
        out.append(d)
    assert out and out[0]["who"] == "hash" and out[0]["level"] == 1 and out[0]["chunk"] == CHUNK, err
    print("debug lines: %r" % out)
    return out


def cycle(words, n):
    return [words[i % len(words)] for i in range(n)]


# output lines of level 1 around one and two chunks: (bits, records, output lines)
@pytest.mark.parametrize("bits,records,out_lines", [(3, 455 * 64 * RPL, CHUNK - 8), (1, 30720 * RPL, CHUNK), (0, 31776 * RPL, CHUNK + 1), (3, 117, 72)])
def test_chunk_counts(ctx, oracle_bin, tmp_path, monkeypatch, capfd, pool, bits, records, out_lines):
    """one chunk less a line (the nearest reachable: - 8), exactly one chunk, one chunk and a line, and an input of 15 lines: fewer than the
    workgroup has threads"""
    words, keyof = pool
    assert geometry(records, 1 << bits)[2] == out_lines
    d = _run(ctx, oracle_bin, tmp_path, monkeypatch, capfd, make_db(cycle(words[:512], records), keyof), bits)
    assert d[0]["lines"] == out_lines and d[0]["chunks"] == -(-out_lines // CHUNK) and d[0]["buckets"] == 1 << bits


def test_two_chunks_and_a_tail_bucket_edges(ctx, oracle_bin, tmp_path, monkeypatch, capfd, pool):
    """two chunks and 56 lines (a tail smaller than a wavefront); of the 8 buckets one has no line, one exactly one line, and the others'
    lines lie in all three chunks"""
    words, keyof = pool
    by = {}
    for w in words:
        by.setdefault(G.bucket_of(keyof[w], 3), []).append(w)
    assert len(by) == 8
    empty, single = 5, 2
    rest = [w for b in sorted(by) if b not in (empty, single) for w in by[b][:64]]
    records = 911 * 64 * RPL
    pl, n_p, out_lines = geometry(records, 8)
    assert (pl, out_lines) == (64, 2 * CHUNK + 56)
    seqs = cycle(rest, records); seqs[records // 2] = by[single][0]
    db = make_db(seqs, keyof)
    per = lines_of(db.keys, 3)
    assert empty not in per and per[single] == 1
    # a piece of 64 lines holds every other bucket (384 distinct words cycle through 512 records), so each has lines in every chunk
    assert all(len({G.bucket_of(k, 3) for k in db.keys[p * 512:(p + 1) * 512]} - {single}) == 6 for p in (0, 455, 910))
    d = _run(ctx, oracle_bin, tmp_path, monkeypatch, capfd, db, 3)
    assert d[0]["lines"] == out_lines and d[0]["chunks"] == 3 and d[0]["lines"] % CHUNK < 64


@pytest.mark.parametrize("behind", [False, True])
def test_hot_bucket_fills_a_chunk(ctx, oracle_bin, tmp_path, monkeypatch, capfd, pool, behind):
    """every tagged line of one whole chunk belongs to one bucket: all ranks of the chunk land on one counter and the bucket's run is the
    whole chunk; at the start of the input, and behind more than a chunk of other keys"""
    words, keyof = pool
    hot = words[0]; hb = G.bucket_of(keyof[hot], 3)
    others = [w for w in words[1:1024] if G.bucket_of(keyof[w], 3) != hb]
    n_hot, n_other = 460 * 64 * RPL, (455 * 64 * RPL if behind else 1000)      # 455 pieces of 72 output lines end 8 lines before the second chunk
    seqs = (cycle(others, n_other) + [hot] * n_hot) if behind else ([hot] * n_hot + cycle(others, n_other))
    db = make_db(seqs, keyof)
    pl, n_p, out_lines = geometry(db.records, 8)
    assert pl == 64
    hot_piece = [all(s == hot for s in seqs[p * pl * RPL:(p + 1) * pl * RPL]) for p in range(n_p)]
    full = [k for k in range(out_lines // CHUNK) if all(hot_piece[p] for p in range(k * CHUNK // (pl + 8), -(-(k + 1) * CHUNK // (pl + 8))))]
    assert full and (full[0] > 0) == behind, "no chunk whose pieces are all hot"
    d = _run(ctx, oracle_bin, tmp_path, monkeypatch, capfd, db, 3)
    # (a chunk of output lines is CHUNK * 64 / 72 hot input lines: every piece adds 8 unused lines)
    assert d[0]["lines"] == out_lines and d[0]["max_bucket"] >= n_hot // RPL >= CHUNK * pl // (pl + 8) + pl


def test_unused_tail_straddles_a_chunk(ctx, oracle_bin, tmp_path, monkeypatch, capfd, pool):
    """1024 buckets, four pieces of 8192 + 1024 output lines; the last piece uses fewer than 5120 of them, so the TAG_NONE lines at its end
    begin before output line 32 768 and end behind it"""
    words, keyof = pool
    records = (3 * 8192 + 4000) * RPL
    pl, n_p, out_lines = geometry(records, 1024)
    assert (pl, n_p, out_lines) == (8192, 4, 36864)
    assert 3 * 9216 + 4000 + 1024 < CHUNK < out_lines            # the last piece writes at most its input lines + one open line per bucket
    d = _run(ctx, oracle_bin, tmp_path, monkeypatch, capfd, make_db(cycle(words, records), keyof), 10)
    assert d[0]["lines"] == out_lines and d[0]["chunks"] == 2 and d[0]["listed"] <= 3 * 9216 + 5024


def two_level_db(pool, bits):
    """600 background words once each, and four words in 56, 64, 65 and 320 copies whose final buckets hold nothing else: 7, 8, 9 and 40 lines"""
    words, keyof = pool
    b1 = (bits + 1) // 2
    special, used = [], set()
    for w in words[600:]:
        b = G.bucket_of(keyof[w], bits)
        if b not in used and len(special) < 4:
            used.add(b); special.append(w)
    bg = [w for w in words[:600] if G.bucket_of(keyof[w], bits) not in used]
    seqs = list(bg)
    for w, c in zip(special, (56, 64, 65, 320)):
        seqs += [w] * c
    perm = np.random.default_rng(bits).permutation(len(seqs))
    db = make_db([seqs[i] for i in perm], keyof)
    per = lines_of(db.keys, bits)
    assert [per[G.bucket_of(keyof[w], bits)] for w in special] == [56, 64, 65, 320]
    level1 = lines_of(db.keys, b1)
    empty_regions = (1 << b1) - len(level1)
    one_line_regions = sum(1 for c in level1.values() if c == 1)
    assert empty_regions > 0 and one_line_regions > 0
    return db, empty_regions


def test_two_levels_regions_and_rows(ctx, oracle_bin, tmp_path, monkeypatch, capfd, pool):
    """level 2: regions without a line (level-1 buckets without records), regions of one line, fine buckets of 7, 8, 9 and 40 lines"""
    db, empty_regions = two_level_db(pool, 20)
    d = _run(ctx, oracle_bin, tmp_path, monkeypatch, capfd, db, 20)
    assert len(d) >= 2 and d[1]["who"] == "hash" and d[1]["level"] == 2 and d[1]["regions"] == 1024 and d[1]["buckets"] == 1024
    assert d[1]["empty_regions"] == empty_regions and d[1]["max_bucket"] == 40


def test_two_levels_long_records(ctx, oracle_bin, tmp_path, monkeypatch, capfd, pool):
    """24-byte records: 512 buckets per level"""
    db, empty_regions = two_level_db(pool, 18)
    d = _run(ctx, oracle_bin, tmp_path, monkeypatch, capfd, db, 18, env={"PLASSHIP_TUNE_FORCE_LONG": "1"}, record_bytes=20)      # (the reference's KmerPosition<int>; 24 bytes on the device)
    assert len(d) >= 2 and d[1]["who"] == "hash" and d[1]["level"] == 2 and d[1]["regions"] == 512 and d[1]["buckets"] == 512
    assert d[1]["empty_regions"] == empty_regions and d[1]["max_bucket"] == 40


def test_nucleotide_rep_sort_lists(ctx, oracle_bin, tmp_path, monkeypatch, capfd):
    """a nucleotide DB of the ladder: 8000 records in runs of four, whose rep sort partitions the grouped records by ranges of the
    representative (KEY_RANGE) into more than one bucket and builds their lists with the level-1 kernel"""
    db = G.nucl_distinct_db(3000)
    d = _run(ctx, oracle_bin, tmp_path, monkeypatch, capfd, db, None, flags=dict(nucl=True))
    rep = [x for x in d if x["who"] == "repsort"]
    assert len(rep) == 1 and rep[0]["level"] == 1 and rep[0]["buckets"] > 1 and rep[0]["listed"] > 0


def test_nucleotide_rep_sort_two_levels(ctx, oracle_bin, tmp_path, monkeypatch, capfd):
    """the rep sort's second level (KEY_RANGE; 24-byte records: 2^18 grouped records make 10 bucket bits = 32 regions of 32 buckets): a region
    is SEVERAL pieces here (a level-1 bucket is cut into pieces of 512 lines), so unused TAG_NONE lines lie inside the regions, not only at
    their end"""
    db = G.nucl_distinct_db(100002)
    assert db.records > 1 << 18
    d = _run(ctx, oracle_bin, tmp_path, monkeypatch, capfd, db, None, env={"PLASSHIP_TUNE_FORCE_LONG": "1"}, flags=dict(nucl=True), record_bytes=20)
    rep = [x for x in d if x["who"] == "repsort"]
    assert [x["level"] for x in rep] == [1, 2], d
    r2 = rep[1]
    assert r2["regions"] > 1 and r2["buckets"] > 1 and r2["listed"] * RPL >= db.records
    assert r2["pieces"] > r2["regions"] - r2["empty_regions"], "no region of several pieces"
    assert r2["lines"] - r2["listed"] > r2["buckets"], "no unused lines beyond one piece's"
