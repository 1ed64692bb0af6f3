"""Hand-made buckets for kmermatcher's group kernels (tests/test_group_ladder_host.py, tests/test_gpu_group_ladder.py).

Stage K5 (plass_amd/csrc/kmermatch_group.hpp) groups the k-mer records of one hash bucket in an LDS table: groupLinesKernel<256, 2048, 3>
("narrow"), groupLinesKernel<512, 4096, 4> ("wide") and, in the 24-byte layout, groupKernel<..., LONG, true> ("long").  The branches a
bucket takes depend on
  its record POSITIONS (lines * 8, padding included) against C = GL_RMAX * BLOCK = 2048 / 4096: up to C the bucket lives in registers, beyond it
      is read from memory once per phase and sub-pass, and a following bucket beyond C gets no look-ahead;
  its DISTINCT keys against M = MAXKEYS = 1536 / 3072 (GR_MAXKEYS = 1536 in groupKernel): `sFlag[0] > MAXKEYS` doubles the sub-passes;
  its NEIGHBOURS inside one workgroup's range (empty, in registers, beyond them), which needs bucketsPerBlock > 1;
  the packed run-head word (0x7FFF - len) << 48 | id << 16 | (pos & 0x7FFF) << 1 | strand, and the filter behind it.
The builders below make small protein DBs whose records are known exactly: a sequence of 14 residues has one window, hence two records (its
k-mer and its identity record, kmermatcher.cpp:241-249), one of 13 residues has the identity record alone; every window of a sequence of at
most 72 residues is selected (59 windows).  Identical sequences share both keys.  PLASSHIP_TUNE_PART_BITS / GROUP_SHAPE / FORCE_LONG
(kmermatch.hip) put these records into the bucket geometry a rung needs, and the PLASSHIP_DEBUG_GROUPHIST line says what the kernel met.
The k-mer index, the identity hash, the partition hash and the sub-pass selector are restated here on the oracle's letter table and XXH64, so
that every key of a DB is known on the host: a collision in the reduced alphabet shows as a wrong distinct count, it is not assumed away.
The expectation of every comparison is the CPU oracle's kmermatcher with the same flags."""
import ctypes
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
AA = "ACDEFGHIKLMNPQRSTVWY"
K, ALPH, KPS, HASH_SHIFT = 14, 13, 60, 67
RPL = 8                                   # linepart.hpp: records per line
REG_CAP = {"narrow": 2048, "wide": 4096}  # GL_RMAX * BLOCK
MAX_KEYS = {"narrow": 1536, "wide": 3072, "long": 1536}       # HT / 4 * 3; GR_MAXKEYS
LAYOUT16_MAX_L = 32764                    # plasship_kmermatch: `!(db->maxEntryLen < SHRT_MAX)` takes the 24-byte layout; an entry is L + 2 bytes
M64 = (1 << 64) - 1


@functools.lru_cache(maxsize=None)
def _ora():
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "build", "liboracle.so"))
    lib.oracle_aa2num.restype = ctypes.POINTER(ctypes.c_ubyte); lib.oracle_aa2num.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.oracle_xxh64_u64.restype = ctypes.c_ulonglong; lib.oracle_xxh64_u64.argtypes = [ctypes.c_ulonglong, ctypes.c_ulonglong]
    return lib


@functools.lru_cache(maxsize=None)
def letter_codes():
    t = _ora().oracle_aa2num(0, ALPH)
    return np.array([t[ord(c)] for c in AA], dtype=np.uint64)


def xxh64(v, seed=HASH_SHIFT):
    return int(_ora().oracle_xxh64_u64(int(v) & M64, seed))


def kmer_index(word):
    """Indexer::int2index on the reduced alphabet: sum code[i] * (alph - 1)^i (kmermatcher.cpp:200 of the oracle)"""
    c = letter_codes(); idx = 0; p = 1
    for ch in word:
        idx += int(c[AA.index(ch)]) * p; p *= ALPH - 1
    return idx & M64


def identity_key(seq, seed=HASH_SHIFT):
    """the k-mer field of a sequence's identity record: XXH64 of Util::hash over the codes"""
    c = letter_codes(); h = 0
    for ch in seq:
        h = (h * 31 + int(c[AA.index(ch)])) & M64
    return xxh64(h, seed)


def window_score(word, seed=HASH_SHIFT):
    return xxh64(kmer_index(word), seed) & 0xFFFF


def sub_class(key, n_sub):
    """the kernels' sub-pass selector"""
    return (((key * 0xD6E8FEB86659FD93) & M64) >> 40) % n_sub


def replay_sub_passes(keys, max_keys):
    """the retry rule: the smallest power of two for which every class holds at most max_keys distinct keys"""
    keys = set(keys); n = 1
    while True:
        per = [0] * n
        for key in keys:
            per[sub_class(key, n)] += 1
        if max(per) <= max_keys:
            return n
        n *= 2


def bucket_of(key, bits):
    """linepart.hpp kmerMix: the final bucket is the top `bits` bits of the mixed key (level 1 takes the upper, level 2 the next ones)"""
    if bits == 0:
        return 0
    x = (key * 0x9E3779B97F4A7C15) & M64; x ^= x >> 29; x = (x * 0xBF58476D1CE4E5B9) & M64; x ^= x >> 32
    return x >> (64 - bits)


class GroupDb:
    """seqs in key order (key = index); rung[i]: the sequence must take part in a candidate line; keys: the k-mer field of every record"""

    def __init__(self, seqs, rung, windows_all=True):
        self.seqs, self.rung = list(seqs), np.asarray(rung, dtype=bool)
        self.nucl = False
        if windows_all:
            keys = []
            for s in self.seqs:
                keys.append(identity_key(s))
                keys.extend(kmer_index(s[p:p + K]) for p in range(len(s) - K + 1))
            self.keys = keys
            self.records, self.distinct = len(keys), len(set(keys))

    def write(self, path):
        path = str(path); off = 0
        with open(path, "wb") as f, open(path + ".index", "wb") as ix:
            for i, s in enumerate(self.seqs):
                e = s.encode() + b"\n\0"
                f.write(e); ix.write(b"%d\t%d\t%d\n" % (i, off, len(e))); off += len(e)
        with open(path + ".dbtype", "wb") as f:
            f.write((1 if self.nucl else 0).to_bytes(4, "little"))
        return path


def _words(rng, n, L, taken):
    """n words of L letters whose reduced-alphabet codes differ from one another and from every word in `taken` (a set of code tuples)"""
    c = letter_codes(); out = []
    while len(out) < n:
        w = rng.integers(0, 20, size=(n - len(out) + 8, L))
        for row in w:
            t = tuple(int(c[i]) for i in row)
            if t not in taken and len(out) < n:
                taken.add(t); out.append("".join(AA[i] for i in row))
    return out


def _from_groups(groups, seed):
    """groups: [(windows 0 | 1, copies)] -> a DB of `copies` identical sequences of 13 + windows residues per group, shuffled"""
    rng = np.random.default_rng(seed); taken = set()
    w1 = _words(rng, sum(1 for w, _ in groups if w), K, taken); w0 = _words(rng, sum(1 for w, _ in groups if not w), K - 1, taken)
    seqs, rung = [], []
    for w, copies in groups:
        s = (w1 if w else w0).pop()
        seqs += [s] * copies; rung += [copies >= 2] * copies
    perm = rng.permutation(len(seqs))
    db = GroupDb([seqs[i] for i in perm], [rung[i] for i in perm])
    assert db.records == sum((1 + w) * c for w, c in groups) and db.distinct == sum(1 + w for w, _ in groups), "a key collision: take another seed"
    return db


@functools.lru_cache(maxsize=None)
def size_db(records):
    """rung A: `records` records in runs of four members (few distinct keys: no retry), the remainder one run of 13-residue sequences"""
    groups = [(1, 4)] * (records // 8)
    if records % 8:
        groups.append((0, records % 8))
    return _from_groups(groups, 1000 + records)


def size_steps(C):
    return [C - 24, C - 9, C - 8, C - 1, C, C + 1, C + 8, C + 40, 3 * C - 3]


@functools.lru_cache(maxsize=None)
def distinct_db(distinct, records=None):
    """rung B: exactly `distinct` keys.  records None: every key in two sequences (2 * distinct records); else `records` <= 2 * distinct records,
    records - distinct keys in two sequences and the rest once (a bucket that still fits the registers)"""
    records = 2 * distinct if records is None else records
    assert distinct <= records <= 2 * distinct
    m, s = records - distinct, 2 * distinct - records
    groups = [(1, 2)] * (m // 2) + [(0, 2)] * (m % 2) + [(1, 1)] * (s // 2) + [(0, 1)] * (s % 2)
    return _from_groups(groups, 2000 + 7 * distinct + records)


def distinct_steps(M):
    return [M - 1, M, M + 1, 2 * M + 1, 6 * M]


# ---- rung C: neighbours inside a workgroup -----------------------------------------------------------------------------------------
HOT_COPIES = 4200           # more than the wide shape's 4096 positions
C_BITS, C_BPB = 14, 3       # 2^14 buckets over 256 CUs * 24 workgroups: three buckets per workgroup


@functools.lru_cache(maxsize=None)
def neighbours_db(seed=31):
    """12 500 k-mers in two sequences each (50 000 records) and four hot 14-residue sequences in HOT_COPIES copies: eight hot keys (k-mer and
    identity record).  The hot words are drawn until, at C_BITS bits, one hot k-mer's bucket is the FIRST of its workgroup's range with an
    occupied successor, one is a LATER one with occupied neighbours on both sides, and all eight hot keys have buckets of their own (also
    at 13 and 11 bits)."""
    rng = np.random.default_rng(seed); taken = set()
    bg = _words(rng, 12500, K, taken)
    occ = set()
    for w in bg:
        occ.add(bucket_of(kmer_index(w), C_BITS)); occ.add(bucket_of(identity_key(w), C_BITS))
    hot, want = [], ["first", "later", "any", "any"]
    while want:
        w = _words(rng, 1, K, taken)[0]
        keys = [kmer_index(w), identity_key(w)]
        all_keys = [k for h in hot for k in (kmer_index(h), identity_key(h))] + keys
        if any(len({bucket_of(k, b) for k in all_keys}) != len(all_keys) for b in (C_BITS, 13, 11)):
            continue
        if any(bucket_of(k, C_BITS) in occ for k in keys):
            continue                                           # a hot bucket holds hot records only: its class does not hang on the background
        b = bucket_of(keys[0], C_BITS)
        kind = "first" if (b % C_BPB == 0 and b + 1 in occ) else "later" if (b % C_BPB == 1 and b - 1 in occ and b + 1 in occ) else "any"
        if kind in want:
            want.remove(kind); hot.append(w)
        elif kind != "any" and "any" in want:
            want.remove("any"); hot.append(w)
    seqs = [w for w in bg for _ in range(2)] + [h for h in hot for _ in range(HOT_COPIES)]
    perm = rng.permutation(len(seqs))
    db = GroupDb([seqs[i] for i in perm], [True] * len(seqs))
    db.hot = hot
    assert db.distinct == 2 * (12500 + 4)
    return db


# ---- rungs D and E: hand-made runs ---------------------------------------------------------------------------------------------------
def head_rule(members):
    """kmermatcher.cpp:450-559 with sort #1's order (kmermatcher.h:56-96): the run's first record is the longest sequence's, then the
    smallest id's, then the smallest position's.  members: [(id, length, position)] -> the winning (id, length, position)"""
    return min(members, key=lambda m: (-m[1], m[0], m[2]))


def can_be_covered(thr, mode, q, t):
    """Util::canBeCovered in single precision"""
    thr, q, t = np.float32(thr), np.float32(q), np.float32(t)
    if mode == 0:
        return bool(q / t >= thr and t / q >= thr)
    if mode == 1:
        return bool(q / t >= thr)
    if mode == 2:
        return bool(t / q >= thr)
    raise ValueError(mode)


def kept(ext, thr, mode, rep, member):
    """does assignGroup keep `member` (id, length, position) of a run whose head is `rep`"""
    diagonal = rep[2] - member[2]
    extendable = diagonal < 0 or diagonal > rep[1] - member[1]
    return extendable if ext else can_be_covered(thr, mode, rep[1], member[1])


def _embed(rng, L, placed, flank=None):
    """a random sequence of L residues holding the words of `placed` {position: word}; flank: the letter on either side of a word (two
    sequences with different flanks share the word's window and not the overlapping ones)"""
    s = [AA[i] for i in rng.integers(0, 20, size=L)]
    for p, w in placed.items():
        assert 0 <= p and p + len(w) <= L
        s[p:p + len(w)] = list(w)
        if flank:
            for q in (p - 1, p + len(w)):
                if 0 <= q < L:
                    s[q] = flank
    return "".join(s)


def _low_score_words(rng, n, taken, limit=3):
    out = []
    while len(out) < n:
        w = _words(rng, 1, K, taken)[0]
        if window_score(w) <= limit:
            out.append(w)
    return out


class HandDb(GroupDb):
    """runs: {name: [(id, length, position), ...]} of the hand-made runs (one shared k-mer each)"""


@functools.lru_cache(maxsize=None)
def head_word_db(seed=5):
    """rung D.  131 600 sequences, all of 13 residues (an identity record each, no window) except the hand-made ones:
      tie      two longest members of 60 residues (ids 70001, 70005), a shorter one (id 100) and one with id 131100
      longer   a member of 40 residues with the smaller id (200) against one of 60 with id 131200: the longer is the head
      twice    the head (id 300, 70 residues) holds the k-mer at positions 5 and 40 (--ignore-multi-kmer 0 keeps both records)
      long     a head of LAYOUT16_MAX_L residues (id 66000) against one a residue shorter (id 131500): one shared k-mer at positions 300 / 290,
               one at the LAST window of either; `last` adds a 30-residue member (id 5) of the last-window k-mer: diagonal 32750
    The two k-mers of the long sequences have window scores of at most 3, so they are among the 59 selected of 32 751 windows."""
    rng = np.random.default_rng(seed); taken = set()
    N = 131600
    x = _words(rng, 3, K, taken); lo = _low_score_words(rng, 2, taken)
    runs = {"tie": [(70001, 60, 20), (70005, 60, 7), (100, 40, 3), (131100, 30, 0)],
            "longer": [(200, 40, 9), (131200, 60, 33)],
            "twice": [(300, 70, 5), (300, 70, 40), (400, 40, 10)],
            "long": [(66000, LAYOUT16_MAX_L, 300), (131500, LAYOUT16_MAX_L - 1, 290)],
            "last": [(66000, LAYOUT16_MAX_L, LAYOUT16_MAX_L - K), (131500, LAYOUT16_MAX_L - 1, LAYOUT16_MAX_L - 1 - K), (5, 30, 0)]}
    word = {"tie": x[0], "longer": x[1], "twice": x[2], "long": lo[0], "last": lo[1]}
    placed = {}
    for name, ms in runs.items():
        for i, L, p in ms:
            placed.setdefault(i, (L, {}))[1][p] = word[name]
    fill = _words(rng, N, K - 1, taken)
    seqs = [(_embed(rng, *placed[i]) if i in placed else fill[i]) for i in range(N)]
    db = HandDb(seqs, [i in placed for i in range(N)], windows_all=False)
    db.runs, db.word = runs, word
    return db


@functools.lru_cache(maxsize=None)
def filter_db(seed=9):
    """rung E: eight runs of a 60-residue head and one member; diagonals on both sides of the two edges of `canBeExtended`, and member lengths on
    both sides of the coverage thresholds of the sweep fixture (-c 0.8 --cov-mode 0; -c 0.9 --cov-mode 1 / 2)"""
    rng = np.random.default_rng(seed); taken = set()
    spec = [("diag_eq", 25, 40, 5), ("diag_gt", 25, 40, 4), ("diag_0", 10, 40, 10), ("diag_m1", 10, 40, 11),
            ("cov_08", 10, 48, 10), ("cov_08_below", 10, 47, 10), ("cov_09", 10, 54, 10), ("cov_09_below", 10, 53, 10)]
    words = _words(rng, len(spec), K, taken)
    seqs, runs, word = [], {}, {}
    for (name, rp, ml, mp), w in zip(spec, words):
        runs[name] = [(len(seqs), 60, rp), (len(seqs) + 1, ml, mp)]; word[name] = w
        seqs += [_embed(rng, 60, {rp: w}, "A"), _embed(rng, ml, {mp: w}, "C")]
    db = HandDb(seqs, [True] * len(seqs))
    db.runs, db.word = runs, word
    assert db.distinct == db.records - len(spec), "the runs share more than their k-mer: take another seed"
    return db


def expected_grouped(db, ext, thr, mode):
    """N_m of a hand-made DB whose only runs are db.runs"""
    n = 0
    for ms in db.runs.values():
        rep = head_rule(ms)
        n += sum(kept(ext, thr, mode, rep, m) for m in ms)
    return n


# ---- the nucleotide rungs (B and D) ------------------------------------------------------------------------------------------------------
# k = 22: a sequence of 22 bases has one window and two records, one of 21 bases its identity record alone.  A window's record carries the
# smaller of the k-mer and its reverse complement, bit 63 = "the k-mer itself was the smaller" (forward); the kernels group by kmer | bit 63.
NK, NSCALE, BIT63, NT = 22, 0.1, 1 << 63, "ACGT"
_COMP = str.maketrans("ACGT", "TGCA")


def revcomp(s):
    return s.translate(_COMP)[::-1]


@functools.lru_cache(maxsize=None)
def _nucl_codes():
    lib = _ora(); t = lib.oracle_aa2num(1, 5)
    lib.oracle_revcomp.restype = ctypes.c_ulonglong; lib.oracle_revcomp.argtypes = [ctypes.c_ulonglong, ctypes.c_int]
    return {ch: int(t[ord(ch)]) for ch in NT}


def nucl_window(word):
    """(canonical k-mer, forward) of one window; None for a k-mer that is its own reverse complement (kmermatcher.cpp:188-197 of the oracle)"""
    c = _nucl_codes(); f = 0
    for ch in word:
        f = (f << 2) | c[ch]
    r = int(_ora().oracle_revcomp(f, len(word)))
    return None if r == f else (min(f, r), f < r)


def nucl_identity_key(seq):
    c = _nucl_codes(); h = 0
    for ch in seq:
        h = (h * 31 + c[ch]) & M64
    return xxh64(h) | BIT63


class NuclDb(GroupDb):
    def __init__(self, seqs, rung):
        self.seqs, self.rung, self.nucl = list(seqs), np.asarray(rung, dtype=bool), True
        keys = []
        for s in self.seqs:
            keys.append(nucl_identity_key(s))
            ws = [nucl_window(s[p:p + NK]) for p in range(len(s) - NK + 1)]
            assert None not in ws and len({w[0] for w in ws}) == len(ws) <= KPS - 1, "a palindromic or repeated window: take another seed"
            keys.extend(w[0] | BIT63 for w in ws)
        self.keys = keys
        self.records, self.distinct = len(keys), len(set(keys))


def _nucl_words(rng, n, L, taken):
    out = []
    while len(out) < n:
        w = "".join(NT[i] for i in rng.integers(0, 4, size=L))
        key = min(w, revcomp(w))
        if key not in taken and (L < NK or nucl_window(w) is not None):
            taken.add(key); out.append(w)
    return out


@functools.lru_cache(maxsize=None)
def nucl_distinct_db(distinct):
    """rung B, nucleotide: exactly `distinct` keys, each in at least two sequences.  distinct // 3 k-mers, each in two copies of a 22-base
    sequence and two of its reverse complement (three keys: the k-mer with four members on both strands, and the identity records of either
    strand), and distinct % 3 pairs of identical 21-base sequences.  The run of the smallest k-mer is the call's first (`firstRunKey`): its
    head, the member with the smallest id, is given the forward strand, so that the never-refreshed `repIsReverse` of run 0 is what it would
    be anyway and no (rep, target, diagonal) triple holds both strands."""
    rng = np.random.default_rng(3000 + distinct); taken = set()
    w1 = _nucl_words(rng, distinct // 3, NK, taken); w0 = _nucl_words(rng, distinct % 3, NK - 1, taken)
    seqs = [x for w in w1 for x in (w, w, revcomp(w), revcomp(w))] + [w for w in w0 for _ in range(2)]
    seqs = [seqs[i] for i in rng.permutation(len(seqs))]
    first = min(w1, key=lambda w: nucl_window(w)[0])
    ids = [i for i, x in enumerate(seqs) if x in (first, revcomp(first))]
    fwd = [i for i in ids if nucl_window(seqs[i])[1]]
    if ids[0] not in fwd:
        seqs[ids[0]], seqs[fwd[0]] = seqs[fwd[0]], seqs[ids[0]]
    db = NuclDb(seqs, [True] * len(seqs))
    assert db.distinct == distinct and db.records == 8 * (distinct // 3) + 2 * (distinct % 3), "a key collision: take another seed"
    return db


def nucl_line(rep, m, first):
    """kmermatcher.cpp:450-559 for one member of a nucleotide run: rep, m = (id, length, record position, forward); first: the call's first run,
    whose `repIsReverse` is never refreshed (false) -> (sign of the score: -1 = the query is to be reversed, diagonal)"""
    rep_rev, m_rev = (not rep[3]) and not first, not m[3]
    if rep_rev == m_rev and not rep_rev or (rep_rev and not m_rev):
        qp, tp = rep[2], m[2]
    else:
        qp, tp = (rep[1] - 1) - rep[2], (m[1] - 1) - m[2]
    q_rev = rep_rev != m_rev
    return (-1 if q_rev else 1), qp - tp


@functools.lru_cache(maxsize=None)
def nucl_head_db():
    """rung D, nucleotide: a 60-base head on either strand against a 40-base member on either strand (four runs), and the call's first run
    (the k-mer A...AC, canonical value 1) with a head on the reverse strand and one member on each strand.  A sequence "on the reverse strand"
    holds the reverse complement of the run's canonical k-mer; its record position is L - p - k.
    runs: {name: [(id, length, record position, forward), ...]}, the head first"""
    for seed in range(50):
        rng = np.random.default_rng(700 + seed); taken = set()
        words = _nucl_words(rng, 4, NK, taken)
        words = [w if nucl_window(w)[1] else revcomp(w) for w in words] + ["A" * (NK - 1) + "C"]
        spec = [("ff", True, [True]), ("fr", True, [False]), ("rf", False, [True]), ("rr", False, [False]), ("first", False, [True, False])]
        seqs, runs = [], {}
        def put(L, p, w, fwd, j):
            # the k-mer with a flank letter of the sequence's own on either side (the windows next to it differ between the run's members)
            core = "CGT"[j] + w + "ACG"[j]
            s = [NT[i] for i in rng.integers(0, 4, size=L)]
            s[p - 1:p + NK + 1] = list(core if fwd else revcomp(core))
            seqs.append("".join(s))
            return (len(seqs) - 1, L, p if fwd else L - p - NK, fwd)
        for (name, rep_fwd, members), w in zip(spec, words):
            runs[name] = [put(60, 17, w, rep_fwd, 0)] + [put(40 + 4 * j, 3 + 5 * j, w, f, 1 + j) for j, f in enumerate(members)]
        # two identical 21-base sequences behind the runs: theirs is the last (rep, target) run of sort #2, the one the reference's scan continues
        # into the stale records behind the compaction point, so every hand-made line is a plain run
        seqs += _nucl_words(rng, 1, NK - 1, taken) * 2
        try:
            db = NuclDb(seqs, [True] * len(seqs))
        except AssertionError:
            continue
        if db.distinct == db.records - 1 - sum(len(ms) - 1 for ms in runs.values()) and min(db.keys) == (1 | BIT63):
            db.runs = runs
            return db
    raise AssertionError("no seed gives runs that share their k-mer alone")


def read_pref_lines(path):
    """{query: {target: (score, diagonal)}} of a prefilter DB, the query's own line left out"""
    path = str(path); data = open(path, "rb").read(); out = {}
    for line in open(path + ".index", "rb"):
        key, o, l = (int(v) for v in line.split()[:3])
        out[key] = {int(r.split(b"\t")[0]): (int(r.split(b"\t")[1]), int(r.split(b"\t")[2])) for r in data[o:o + l].rstrip(b"\0").split(b"\n") if r and int(r.split(b"\t")[0]) != key}
    return out


def check_nucl_heads(db, lines):
    """every hand-made nucleotide run: the longest member lists the others with the strand and the diagonal the restated rule gives"""
    for name, ms in db.runs.items():
        rep = min(ms, key=lambda m: (-m[1], m[0], m[2]))
        assert rep == ms[0]
        for m in ms[1:]:
            assert lines[rep[0]].get(m[0]) == nucl_line(rep, m, name == "first"), "run %s, member %d: %r, expected %r" % (name, m[0], lines[rep[0]].get(m[0]), nucl_line(rep, m, name == "first"))
            assert rep[0] not in lines[m[0]]


FILTER_FLAGS = [dict(ext=0, c=0.0, cov_mode=0), dict(ext=1, c=0.0, cov_mode=0), dict(ext=0, c=0.8, cov_mode=0), dict(ext=0, c=0.9, cov_mode=1),
                dict(ext=0, c=0.9, cov_mode=2)]


# ---- flags, the oracle's output, the debug line ----------------------------------------------------------------------------------------
def oracle_flags(ext=0, c=0.0, cov_mode=0, multi=1, nucl=False):
    if nucl:
        return ["--alph-size", "5", "--kmer-per-seq", str(KPS), "--kmer-per-seq-scale", "%.3f" % NSCALE, "-k", str(NK), "-c", "%g" % c, "--cov-mode", str(cov_mode),
                "--ignore-multi-kmer", str(multi), "--hash-shift", str(HASH_SHIFT), "--include-only-extendable", str(ext)]
    return ["--alph-size", str(ALPH), "--kmer-per-seq", str(KPS), "--kmer-per-seq-scale", "0.000", "-k", str(K), "-c", "%g" % c, "--cov-mode", str(cov_mode),
            "--ignore-multi-kmer", str(multi), "--hash-shift", str(HASH_SHIFT), "--include-only-extendable", str(ext)]


def param_kwargs(ext=0, c=0.0, cov_mode=0, multi=1, nucl=False):
    if nucl:
        return dict(k=NK, alph_size=5, kmer_per_seq=KPS, kmer_per_seq_scale=NSCALE, hash_shift=HASH_SHIFT, include_only_extendable=bool(ext),
                    ignore_multi_kmer=bool(multi), cov_mode=cov_mode, c=c)
    return dict(k=K, alph_size=ALPH, kmer_per_seq=KPS, kmer_per_seq_scale=0.0, hash_shift=HASH_SHIFT, include_only_extendable=bool(ext),
                ignore_multi_kmer=bool(multi), cov_mode=cov_mode, c=c)


_COUNTS = re.compile(r"oracle kmermatcher: \d+ seqs, N_k=(\d+) N_m=(\d+) N_c=(\d+)")


def oracle_counts(log):
    m = _COUNTS.search(log)
    assert m, "no N_k / N_m / N_c line in the oracle's output:\n%s" % log
    return tuple(int(v) for v in m.groups())


def read_pref(path):
    """{query: {target: diagonal}} of a prefilter DB, the query's own line left out"""
    path = str(path); data = open(path, "rb").read(); out = {}
    for line in open(path + ".index", "rb"):
        key, o, l = (int(v) for v in line.split()[:3])
        out[key] = {}
        for r in data[o:o + l].rstrip(b"\0").split(b"\n"):
            if r:
                t, _score, d = r.split(b"\t")
                if int(t) != key:
                    out[key][int(t)] = int(d)
    return out


def connected(pref):
    keys = set()
    for q, tg in pref.items():
        if tg:
            keys.add(q); keys.update(tg)
    return keys


def check_rungs_connected(db, pref):
    """every rung sequence takes part in a candidate line"""
    conn = connected(pref)
    lone = [i for i in np.nonzero(db.rung)[0] if int(i) not in conn]
    assert not lone, "%d rung sequences take part in no candidate line (first ids %r)" % (len(lone), lone[:10])


def check_heads(db, pref, ext=0):
    """rung D / E under --include-only-extendable 0, -c 0: the head the rule names lists every other member of its run, with the run's diagonal where
    the pair shares nothing else; no other member lists one"""
    for name, ms in db.runs.items():
        rep = head_rule(ms)
        others = {m[0]: m for m in ms if m[0] != rep[0]}
        for i, m in others.items():
            assert i in pref[rep[0]], "run %s: head %d does not list member %d" % (name, rep[0], i)
            assert rep[0] not in pref[i] and not (set(others) - {i}) & set(pref[i]), "run %s: member %d is a head" % (name, i)
            shared = sum(1 for o in db.runs.values() if {rep[0], i} <= {x[0] for x in o})
            if shared == 1:
                assert pref[rep[0]][i] == rep[2] - m[2], "run %s: member %d on diagonal %d, expected %d" % (name, i, pref[rep[0]][i], rep[2] - m[2])


_HIST = re.compile(r"groupHist call \d+ kernel (\w+) buckets (\d+) bpb (\d+) records (\d+) \| maxPos (\d+) regCap (\d+) overRegs (\d+) \(first (\d+), later (\d+)\) "
                   r"\| maxDistinct (\d+) maxKeys (\d+) \| maxSub (\d+) multiSub (\d+) \| pairs((?: \w+>\w+ \d+)+)")


def group_hist(err):
    """the PLASSHIP_DEBUG_GROUPHIST lines of a stderr text -> [dict]"""
    out = []
    for m in _HIST.finditer(err):
        names = ("buckets", "bpb", "records", "max_pos", "reg_cap", "over_regs", "big_first", "big_later", "max_distinct", "max_keys", "max_sub", "multi_sub")
        d = dict(kernel=m.group(1), **{n: int(m.group(2 + i)) for i, n in enumerate(names)})
        d["pairs"] = {p: int(c) for p, c in re.findall(r"(\w+>\w+) (\d+)", m.group(14))}
        out.append(d)
    return out
