"""groupLinesKernel's register path on hand-made buckets that decide what a thread's records meet in the table (run with `-m gpu` on an MI355X).

A thread of groupLinesKernel holds up to GL_RMAX = 8 records of a bucket and probes the LDS table for them; these buckets pin what such a
group of probes can meet, whatever order the kernel issues them in.  Every case is one kmermatcher call built like those of
tests/test_gpu_group_ladder.py (its `_case`: the candidate DB equals the CPU oracle's byte for byte, N_k / N_m / N_c equal the oracle's, the
PLASSHIP_DEBUG_GROUPHIST line names the kernel and the branch), on both workgroup shapes ("narrow" 256 x 2048, "wide" 512 x 4096):

  same[shape-ext]       one bucket of exactly C = GL_RMAX * BLOCK records that all hold ONE k-mer (C copies of a 14-residue sequence; one bucket bit
                        parts its k-mer from its identity record): every record of every thread has the same key, so one probe claims the slot and
                        all others find it taken by their own k-mer, and the multi bit is set from within one thread
  collide[shape-ext]    eight distinct k-mers with ONE home slot under the kernels' multiplier 0xD6E8FEB86659FD93 (searched on the host; HT = 4096,
                        hence also 2048), six in three sequences and two in one: the first probe fails for all but one of them, the walk runs in
                        both phases, and the two single keys stand between runs
  size[shape-i]         a bucket of 1, 7, 8, 9, C - 1, C and C + 1 records: a lone record among seven sentinels, a partial and a full line, the
                        last register partly and wholly filled, and the hand-over to the record-by-record path at C + 1
  retry[shape-ext]      C records of glMaxKeys(HT) + 1 distinct k-mers: the sub-passes double on the register path, the arena cursor is rewound and
                        the output space is reserved again
  neighbours[shape]     2^14 buckets, three per workgroup: a bucket of 20 records followed by one of 1200, both in registers; the second bucket's
                        records take the registers while the first one's are still being written out
--include-only-extendable 0 and 1 (`ext`) where named."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_group_ladder import _case, _clear, ctx, oracle  # noqa: F401  (fixtures of the ladder, one context and one oracle cache per module)

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import group_ladder as G  # noqa: E402

pytestmark = pytest.mark.gpu

MUL, HT_WIDE = 0xD6E8FEB86659FD93, 4096
_DBS = {}


def _word(rng):
    return "".join(G.AA[i] for i in rng.integers(0, 20, size=G.K))


def home_slot(key, ht=HT_WIDE):
    return (((key * MUL) & G.M64) >> 32) & (ht - 1)


def same_db(C):
    """C copies of one 14-residue sequence whose k-mer and identity record fall into different buckets at one bucket bit"""
    if ("same", C) not in _DBS:
        rng = np.random.default_rng(77)
        while True:
            w = _word(rng)
            if G.bucket_of(G.kmer_index(w), 1) != G.bucket_of(G.identity_key(w), 1):
                break
        _DBS["same", C] = G.GroupDb([w] * C, [True] * C)
    return _DBS["same", C]


def collide_db():
    if "collide" not in _DBS:
        rng = np.random.default_rng(78)
        first = _word(rng); words, codes = [first], {G.kmer_index(first)}
        while len(words) < 8:
            w = _word(rng); k = G.kmer_index(w)
            if k not in codes and home_slot(k) == home_slot(G.kmer_index(first)):
                words.append(w); codes.add(k)
        seqs = [w for w in words[:6] for _ in range(3)] + words[6:]
        seqs = [seqs[i] for i in rng.permutation(len(seqs))]
        db = G.GroupDb(seqs, [True] * len(seqs))
        assert db.distinct == 16 and len({home_slot(G.kmer_index(w)) for w in words}) == 1 == len({home_slot(G.kmer_index(w), 2048) for w in words})
        _DBS["collide"] = db
    return _DBS["collide"]


def neighbours_db(small=10, big=600):
    """a k-mer of `small` sequences in the first bucket of a workgroup's three (14 bucket bits), one of `big` sequences in the next bucket"""
    if "neighbours" not in _DBS:
        rng = np.random.default_rng(79)
        while True:
            a = _word(rng); ba = G.bucket_of(G.kmer_index(a), G.C_BITS)
            if ba % G.C_BPB == 0:
                break
        while True:
            b = _word(rng)
            if G.bucket_of(G.kmer_index(b), G.C_BITS) == ba + 1:
                break
        keys = [G.kmer_index(a), G.identity_key(a), G.kmer_index(b), G.identity_key(b)]
        assert len({G.bucket_of(k, G.C_BITS) for k in keys}) == 4, "the identity records share a bucket: take another seed"
        seqs = [a] * small + [b] * big
        seqs = [seqs[i] for i in rng.permutation(len(seqs))]
        _DBS["neighbours"] = G.GroupDb(seqs, [True] * len(seqs))
    return _DBS["neighbours"]


@pytest.mark.parametrize("ext", [0, 1])
@pytest.mark.parametrize("shape", ["narrow", "wide"])
def test_same(ctx, oracle, tmp_path, monkeypatch, capfd, shape, ext):
    C = G.REG_CAP[shape]
    h = _case(ctx, oracle, tmp_path, monkeypatch, capfd, "same%d" % C, same_db(C), shape, bits=1, flags=dict(ext=ext))
    assert h["max_pos"] == C and h["over_regs"] == 0 and h["max_distinct"] == 1 and h["max_sub"] == 1


@pytest.mark.parametrize("ext", [0, 1])
@pytest.mark.parametrize("shape", ["narrow", "wide"])
def test_collide(ctx, oracle, tmp_path, monkeypatch, capfd, shape, ext):
    db = collide_db()
    h = _case(ctx, oracle, tmp_path, monkeypatch, capfd, "collide", db, shape, bits=0, flags=dict(ext=ext))
    assert h["over_regs"] == 0 and h["max_distinct"] == db.distinct and h["max_sub"] == 1


@pytest.mark.parametrize("i", range(7))
@pytest.mark.parametrize("shape", ["narrow", "wide"])
def test_size(ctx, oracle, tmp_path, monkeypatch, capfd, shape, i):
    C = G.REG_CAP[shape]
    records = [1, 7, 8, 9, C - 1, C, C + 1][i]
    h = _case(ctx, oracle, tmp_path, monkeypatch, capfd, "size%d" % records, G.size_db(records), shape, bits=0)
    assert h["max_pos"] == (records + G.RPL - 1) // G.RPL * G.RPL and h["over_regs"] == int(records > C) and h["max_sub"] == 1


@pytest.mark.parametrize("ext", [0, 1])
@pytest.mark.parametrize("shape", ["narrow", "wide"])
def test_retry(ctx, oracle, tmp_path, monkeypatch, capfd, shape, ext):
    M, C = G.MAX_KEYS[shape], G.REG_CAP[shape]
    db = G.distinct_db(M + 1, C)
    h = _case(ctx, oracle, tmp_path, monkeypatch, capfd, "inregs%d_%d" % (M + 1, C), db, shape, bits=0, flags=dict(ext=ext))
    assert G.replay_sub_passes(db.keys, M) == 2 == h["max_sub"] and h["max_pos"] == C and h["over_regs"] == 0 and h["max_distinct"] == M + 1


@pytest.mark.parametrize("shape", ["narrow", "wide"])
def test_neighbours(ctx, oracle, tmp_path, monkeypatch, capfd, shape):
    h = _case(ctx, oracle, tmp_path, monkeypatch, capfd, "batch_neighbours", neighbours_db(), shape, bits=G.C_BITS)
    assert h["bpb"] >= 2 and h["over_regs"] == 0 and h["pairs"]["regs>regs"] >= 1 and h["max_pos"] == 600
