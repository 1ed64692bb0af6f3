"""rescorediagonal --rescore-mode 3 on hand-made candidate pairs at every edge of plasship_rescore's kernels (plass_amd/csrc/rescore.hip).

Two parts, neither needs a GPU:

1. `restate`: a plain Python restatement of what the reference writes for --rescore-mode 3, read from the reference's text alone
   (lib/mmseqs/src; the line numbers are given at each function), in float32 where the reference computes in `float`.  Only the E-value,
   the bit score and the 123 x 123 ASCII score table come from liboracle.so (pinned on the reference's constants in
   tests/test_oracle_golden.py).  It returns the alignment DB's entries and, per candidate pair, the gate booleans, the winning wrap and
   its diagonalLen.  The CPU oracle's rescorediagonal must write the same bytes (tests/test_rescore_ladder_host.py).

2. Seeded builders of query DB / target DB / prefilter DB triples ("ladders"): a target is a copy of a region of its query, placed on the
   intended diagonal, about one column in ten substituted, with one more substitution forced at overlap column 0, 3, 4, 15, 16, 17,
   last - 1 or last (one per target), letters in lower case here and there, keys distinct and not in file order, and the diagonal written
   as signed 16-bit text.  The first entry of every data file is a sequence no pair uses: where no diagonal scores above 0 the reference's
   identity loop runs over index -1 of both strings (rescorediagonal.cpp:276-282 with startPos = endPos = -1), which is the NUL of the
   entry in front of it for every entry but the first.  For a pair that is no identity pair the ladders stay out of that case: the OPEN
   flag set (every score above 0 passes the E-value gate, so every line and its score, coordinates and identity count are visible) runs
   on the prefilter DB without the pairs the restatement scores 0; the STRICT flag set runs on all of them.
"""
import ctypes
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
F32 = np.float32
FLT_EPSILON = np.finfo(np.float32).eps
DBTYPE_AA, DBTYPE_NUCL, DBTYPE_ALN, DBTYPE_PREF, DBTYPE_PREF_REV = 0, 1, 5, 7, 14
RS_SHORT_MAX = 768          # rescore.hip: min(qLen, tLen) up to which one thread scores a pair
GATES = ("canBeCovered", "hasAlnLen", "hasCov", "hasSeqId", "hasEvalue")
STAR = 42


# ------------------------------------------------------------------------------------------------------------------ liboracle pieces
@functools.lru_cache(maxsize=None)
def _lib():
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "build", "liboracle.so"))
    lib.oracle_bitscore.restype = ctypes.c_double; lib.oracle_bitscore.argtypes = [ctypes.c_int, ctypes.c_double]
    lib.oracle_evalue.restype = ctypes.c_double; lib.oracle_evalue.argtypes = [ctypes.c_int, ctypes.c_ulonglong, ctypes.c_double, ctypes.c_double]
    lib.oracle_ascii_submat.restype = ctypes.POINTER(ctypes.c_byte); lib.oracle_ascii_submat.argtypes = [ctypes.c_int]
    return lib


@functools.lru_cache(maxsize=None)
def submat(nucl):
    """SubstitutionMatrix.h:56-73 (createAsciiSubMat): [123][123] scores indexed by the two ASCII letters"""
    p = _lib().oracle_ascii_submat(int(nucl))
    return np.ctypeslib.as_array(p, shape=(123 * 123,)).astype(np.int64).reshape(123, 123).copy()


def evalue(nucl, db_res, score, q_len):
    return _lib().oracle_evalue(int(nucl), int(db_res), float(score), float(q_len))


def bit_score(nucl, score):
    return int(_lib().oracle_bitscore(int(nucl), float(score)) + 0.5)          # rescorediagonal.cpp:252


def min_score_for(nucl, db_res, q_len, e):
    """the lowest raw score whose E-value passes -e for that query length (the E-value falls as the score grows)"""
    s = 0
    while evalue(nucl, db_res, s, q_len) > e:
        s += 1
    return s


# ------------------------------------------------------------------------------------------------------------------ the restatement
def _nucl_class(c):
    """NucleotideMatrix.cpp:17-61 (setupLetterMapping): the letter whose number an ASCII byte gets"""
    u = chr(c).upper()
    if u in "ATGC":
        return u
    if u in "UW":
        return "T"
    if u in "KBDVRS":
        return "G"
    if u in "MYH":
        return "C"
    return "X"


@functools.lru_cache(maxsize=None)
def revcomp_table():
    """rescorediagonal.cpp:175-178: num2aa[reverseResidue(aa2num[c])], reverseLookup of NucleotideMatrix.cpp:9-13"""
    rev = {"A": "T", "G": "C", "C": "G", "T": "A", "X": "X"}
    return np.array([ord(rev[_nucl_class(c)]) for c in range(256)], dtype=np.uint8)


def reverse_query(q):
    return revcomp_table()[q[::-1]]


def can_be_covered(thr, mode, q, t):
    """Util.cpp:533-550; COV_MODE_BIDIRECTIONAL 0, TARGET 1, QUERY 2, LENGTH_QUERY 3, LENGTH_TARGET 4, LENGTH_SHORTER 5 (Parameters.h)"""
    q, t = F32(q), F32(t)
    if mode == 0:
        return bool(q / t >= thr and t / q >= thr)
    if mode == 2:
        return bool(t / q >= thr)
    if mode == 1:
        return bool(q / t >= thr)
    if mode == 3:
        return bool(t / q >= thr and float(t / q) <= 1.0)
    if mode == 4:
        return bool(q / t >= thr and float(q / t) <= 1.0)
    if mode == 5:
        return bool(min(t, q) / max(t, q) >= thr)
    return True


def has_coverage(thr, mode, qc, tc):
    """Util.cpp:552-567"""
    if mode == 0:
        return bool(qc >= thr and tc >= thr)
    if mode == 2:
        return bool(qc >= thr)
    if mode == 1:
        return bool(tc >= thr)
    return True


def compute_cov(start, end, length):
    """StripedSmithWaterman.cpp:1055-1057, in unsigned 32-bit arithmetic"""
    s, e = start & 0xFFFFFFFF, end & 0xFFFFFFFF
    return F32((min(length, max(s, e)) - min(s, e) + 1) & 0xFFFFFFFF) / F32(length)


def compute_seq_id(mode, ids, q_len, t_len, aln_len):
    """Util.cpp:588-598"""
    if mode == 1:
        return F32(ids) / F32(min(q_len, t_len))
    if mode == 2:
        return F32(ids) / F32(max(q_len, t_len))
    if mode == 0:
        return F32(ids) / F32(aln_len)
    return F32(0.0)


def seq_id_text(seq_id):
    """Util.cpp:278-307 (fastSeqIdToBuffer) as Matcher.cpp:329-330 uses it: on the 1.0 branch the returned pointer stands ON the final
    NUL, not behind it, so the tab that resultToBuffer writes at [-1] replaces the third '0': "1.00"."""
    seq_id = F32(seq_id)
    if float(seq_id) == 1.0:
        return "1.00"
    s = "0."
    if float(seq_id) < 0.10:
        s += "0"
    if float(seq_id) < 0.01:
        s += "0"
    return s + "%d" % int(seq_id * F32(1000))


def by_diagonal(mat, q, t, diagonal):
    """DistanceCalculator.h:115-175 with computeGlobalSubstitutionStartEndDistance (204-220) -> (start, end, score, diagonalLen)"""
    dist = abs(diagonal)
    if diagonal >= 0 and dist < len(q):
        n = min(len(t), len(q) - dist)
        s1, s2 = q[dist:dist + n], t[:n]
    elif diagonal < 0 and dist < len(t):
        n = min(len(t) - dist, len(q))
        s1, s2 = q[:n], t[dist:dist + n]
    else:
        return -1, -1, 0, 0
    first = 1 if (s1[0] == STAR or s2[0] == STAR) else 0
    last = n - 1
    if last > 0 and (s1[n - 1] == STAR or s2[n - 1] == STAR):
        last -= 1
    score = int(mat[s1[first:last + 1], s2[first:last + 1]].sum()) if last >= first else 0
    return first, last, max(score, 0), n


def ungapped_alignment(mat, q, t, d16):
    """DistanceCalculator.h:93-113: every +-65536 wrap of the 16-bit diagonal; the strictly better score wins
    -> (start, end, score, diagonalLen, diagonal, distToDiagonal, index of the winning wrap or -1)"""
    best = (-1, -1, 0, 0, 0, 0, -1)
    wrap = 0
    for dev in range(1, 1 + len(t) // 32768 + 1):
        real = -dev * 65536 + d16
        s, e, sc, n = by_diagonal(mat, q, t, real)
        if sc > best[2]:
            best = (s, e, sc, n, real, abs(real), wrap)
        wrap += 1
    for dev in range(0, len(q) // 65536 + 1):
        real = dev * 65536 + d16
        s, e, sc, n = by_diagonal(mat, q, t, real)
        if sc > best[2]:
            best = (s, e, sc, n, real, abs(real), wrap)
        wrap += 1
    return best


def intersecting_wraps(q_len, t_len, d16):
    out, wrap = [], 0
    for dev in range(1, 1 + t_len // 32768 + 1):
        if abs(-dev * 65536 + d16) < t_len:
            out.append(wrap)
        wrap += 1
    for dev in range(0, q_len // 65536 + 1):
        if dev * 65536 + d16 < q_len:
            out.append(wrap)
        wrap += 1
    return out


def restate(qdb, tdb, same, pref, reverse_capable, par):
    """rescorediagonal.cpp:146-356 for RESCORE_MODE_END_TO_END_ALIGNMENT.  qdb / tdb: SeqDB; pref: [(query key, [(target key, prefScore,
    diagonal as signed 16-bit)])] -> ({query key: entry bytes}, [per pair dict])"""
    nucl = qdb.nucl
    mat = submat(nucl)
    cov_thr, seq_id_thr = F32(par["c"]), F32(par["min_seq_id"])
    db_res = tdb.residues()
    out, pairs = {}, []
    for qkey, lines in pref:
        text = b""
        if lines:
            q = qdb.seq(qkey)
            q_len = len(q)
            q_rev = reverse_query(q) if reverse_capable else None
        for tkey, pref_score, diag in lines:
            d16 = diag & 0xFFFF                                                  # QueryMatcher.h:88
            is_reverse = bool(reverse_capable and pref_score < 0)
            q_aln = q_rev if is_reverse else q
            is_identity = qdb.id_of(qkey) == tdb.id_of(tkey) and (par["add_self"] or same)
            t = tdb.seq(tkey)
            db_len = len(t)
            info = dict(q=qkey, t=tkey, canBeCovered=can_be_covered(cov_thr, par["cov_mode"], q_len, db_len), identity=is_identity,
                        accepted=False, wrap=-1, diag_len=0, score=0, reverse=is_reverse)
            pairs.append(info)
            if not info["canBeCovered"]:
                continue
            start, end, score, diag_len, diagonal, dist, wrap = ungapped_alignment(mat, q_aln, t, d16)
            ev = evalue(nucl, db_res, score, q_len)
            bits = bit_score(nucl, score)
            aln_len = end - start + 1
            if diagonal >= 0:
                qs, qe, ds, de = start + dist, end + dist, start, end
            else:
                qs, qe, ds, de = start, end, start + dist, end + dist
            seq_id = 0.0
            if ev <= par["e"] or is_identity:
                if start < 0:
                    # index -1 of both strings: the NUL that ends the entry in front (the ladders keep the first entry out of every pair)
                    if is_reverse or qdb.first_key == qkey or tdb.first_key == tkey:
                        raise ValueError("pair (%d, %d): the reference reads in front of a buffer here" % (qkey, tkey))
                    ids = 1
                else:
                    a, b = q_aln[qs:qe + 1] & 0xDF, t[ds:de + 1] & 0xDF
                    ids = int(np.count_nonzero(a == b))
                seq_id = float(compute_seq_id(par["seq_id_mode"], ids, q_len, db_len, aln_len))
            query_cov, target_cov = compute_cov(qs, qe, q_len), compute_cov(ds, de, db_len)
            if is_reverse:
                qs, qe = q_len - qs - 1, q_len - qe - 1
            info.update(hasCov=has_coverage(cov_thr, par["cov_mode"], query_cov, target_cov),
                        hasSeqId=bool(seq_id >= float(seq_id_thr - FLT_EPSILON)), hasEvalue=bool(ev <= par["e"]),
                        hasAlnLen=bool(aln_len >= par["min_aln_len"]), wrap=wrap, diag_len=diag_len, score=score, aln_len=aln_len)
            if is_identity or (info["hasAlnLen"] and info["hasCov"] and info["hasSeqId"] and info["hasEvalue"]):
                info["accepted"] = True
                line = "%d\t%d\t%s\t%.3E\t%d\t%d\t%d\t%d\t%d\t%d" % (tkey, bits, seq_id_text(seq_id), ev, qs, qe, q_len, ds, de, db_len)
                if par["a"]:
                    line += "\t%dM" % aln_len                                    # rescorediagonal.cpp:285-291
                text += line.encode() + b"\n"
        out[qkey] = text + b"\0"
    return out, pairs


def only_failing_gate(info):
    """the one gate that keeps a pair out, or None"""
    if not info["canBeCovered"]:
        return "canBeCovered"
    bad = [g for g in GATES[1:] if not info[g]]
    return bad[0] if len(bad) == 1 else None


# ------------------------------------------------------------------------------------------------------------------ DBs
class SeqDB:
    """sequences under distinct keys that are not in file order; the first entry of the data file takes part in no pair"""

    def __init__(self, nucl):
        self.nucl, self.seqs, self.keys = nucl, [], None

    def add(self, s):
        self.seqs.append(np.ascontiguousarray(s, dtype=np.uint8))
        return len(self.seqs) - 1

    def finish(self, rng):
        dummy = self.add(random_seq(rng, 17, self.nucl))
        n = len(self.seqs)
        self.keys = rng.choice(np.arange(1, 8 * n + 8), size=n, replace=False).astype(np.int64)
        order = [dummy] + [int(i) for i in rng.permutation(n) if i != dummy]
        self.file_order = order
        self.first_key = int(self.keys[dummy])
        self.by_key = {int(k): i for i, k in enumerate(self.keys)}
        self.rank = {int(k): r for r, k in enumerate(sorted(self.by_key))}
        return self

    def key(self, i):
        return int(self.keys[i])

    def seq(self, key):
        return self.seqs[self.by_key[key]]

    def id_of(self, key):
        return self.rank[key]

    def residues(self):
        return sum(len(s) for s in self.seqs)

    def write(self, path):
        from plass_amd.synth import write_db
        path = str(path)
        off, at, parts = {}, 0, []
        for i in self.file_order:
            off[i] = at
            parts.append(self.seqs[i].tobytes() + b"\n\0")
            at += len(self.seqs[i]) + 2
        idx = sorted(range(len(self.seqs)), key=self.key)
        write_db(path, b"".join(parts), [off[i] for i in idx], [len(self.seqs[i]) + 2 for i in idx], [self.key(i) for i in idx],
                 DBTYPE_NUCL if self.nucl else DBTYPE_AA)
        return path


def write_text_db(path, entries, dbtype):
    from plass_amd.synth import write_db
    keys = sorted(entries)
    off, at = [], 0
    for k in keys:
        off.append(at); at += len(entries[k])
    write_db(str(path), b"".join(entries[k] for k in keys), off, [len(entries[k]) for k in keys], keys, dbtype)
    return str(path)


AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
NT = np.frombuffer(b"ACGT", dtype=np.uint8)
IUPAC = b"ACGTUMYHWKBDVRSN"
EDGE_COLS = (0, 3, 4, 15, 16, 17, -2, -1)


def random_seq(rng, n, nucl):
    return rng.choice(NT if nucl else AA, size=n)


def _other_letter(rng, c, nucl):
    """a letter of another class than c (so the score and the identity count both move)"""
    alpha = NT if nucl else AA
    cls = ord(_nucl_class(int(c))) if nucl else (int(c) & 0xDF)
    while True:
        x = int(rng.choice(alpha))
        if x != cls:
            return x


def lower_some(rng, s, rate=0.12):
    s = s.copy()
    m = (rng.random(len(s)) < rate) & (s >= 65) & (s <= 90)
    s[m] |= 0x20
    return s


def alias_some(rng, s, rate=0.06):
    """nucleotides: a letter replaced by another one of the SAME number (T -> U or W, G -> K B D V R S, C -> M Y H): the score stays,
    the identity count does not"""
    s = s.copy()
    same = {"T": b"UW", "G": b"KBDVRS", "C": b"MYH"}
    for i in np.nonzero(rng.random(len(s)) < rate)[0]:
        ch = chr(int(s[i]))
        if ch in same:
            s[i] = int(rng.choice(np.frombuffer(same[ch], dtype=np.uint8)))
    return s


def overlap_of(q_len, t_len, d):
    """(query offset, target offset, columns) of diagonal d, or None"""
    if d >= 0 and d < q_len:
        return d, 0, min(t_len, q_len - d)
    if d < 0 and -d < t_len:
        return 0, -d, min(t_len + d, q_len)
    return None


def diag_for(q_len, t_len, ov, sign):
    """the diagonal of that sign on which the pair overlaps in `ov` columns, or None"""
    if sign > 0:
        d = q_len - ov if ov < t_len else (q_len - t_len if q_len >= t_len else None)
        if d is None or d < 0 or overlap_of(q_len, t_len, d)[2] != ov:
            return None
        return d
    d = -(t_len - ov) if ov < q_len else (-(t_len - q_len) if t_len > q_len else None)
    if d is None or d >= 0 or overlap_of(q_len, t_len, d)[2] != ov:
        return None
    return d


def plant(rng, q_aln, t_len, d, nucl, forced=None, rate=0.1, subs=None):
    """a target of t_len residues that copies q_aln on diagonal d; about one column in `1 / rate` substituted but none of EDGE_COLS,
    then column `forced` (an index into EDGE_COLS) substituted; subs: exactly these columns instead"""
    t = random_seq(rng, t_len, nucl)
    qo, to, n = overlap_of(len(q_aln), t_len, d)
    cols = q_aln[qo:qo + n].copy()
    cols[(cols >= 97) & (cols <= 122)] &= 0xDF
    edge = {c % n for c in EDGE_COLS if -n <= c < n}
    if subs is None:
        subs = [int(i) for i in np.nonzero(rng.random(n) < rate)[0] if int(i) not in edge]
        if forced is not None and -n <= EDGE_COLS[forced] < n:
            subs.append(EDGE_COLS[forced] % n)
    for i in subs:
        cols[i] = _other_letter(rng, cols[i], nucl)
    t[to:to + n] = cols
    return t


def d16_text(d):
    w = d & 0xFFFF
    return w - 65536 if w >= 32768 else w


class Ladder:
    """a query DB, a target DB (or the same one) and the candidate pairs with the class each belongs to"""

    def __init__(self, name, nucl, rev=False, same=False, seed=1):
        self.name, self.nucl, self.rev, self.same = name, nucl, rev, same
        self.rng = np.random.default_rng(seed)
        self.q = SeqDB(nucl)
        self.t = self.q if same else SeqDB(nucl)
        self.pairs = []                                # (query index, target index, prefScore, true diagonal, class)
        self.no_line = set()                           # queries that keep an empty entry

    def pair(self, qi, ti, d, cls, reverse=False):
        score = int(self.rng.integers(1, 1000))
        self.pairs.append((qi, ti, -score if reverse else score, d, cls))

    def finish(self, lower=True, alias=True):
        rng = self.rng
        for db in ({id(self.q): self.q, id(self.t): self.t}).values():
            for i, s in enumerate(db.seqs):
                if self.nucl and alias:
                    s = alias_some(rng, s)
                db.seqs[i] = lower_some(rng, s) if lower else s
            db.finish(rng)
        self.cls = {}
        per_q = {}
        order = rng.permutation(len(self.pairs))
        for j in order:
            qi, ti, sc, d, cls = self.pairs[int(j)]
            qk, tk = self.q.key(qi), self.t.key(ti)
            assert (qk, tk) not in self.cls, "a pair twice"
            self.cls[(qk, tk)] = cls
            per_q.setdefault(qk, []).append((tk, sc, d16_text(d)))
        self.pref = [(int(k), per_q.get(int(k), [])) for k in sorted(self.q.by_key)]     # an entry for every query, some of them empty
        return self

    def n_lines(self, keep=None):
        return sum(1 for _, lines in self.pref for l in lines if keep is None or keep(_, l[0]))

    def pref_entries(self, keep=None):
        return {qk: b"".join(b"%d\t%d\t%d\n" % l for l in lines if keep is None or keep(qk, l[0])) + b"\0" for qk, lines in self.pref}

    def write(self, d, keep=None, tag=""):
        """-> (query DB path, target DB path, prefilter DB path)"""
        d = str(d)
        qp = self.q.write(os.path.join(d, self.name + "_q"))
        tp = qp if self.same else self.t.write(os.path.join(d, self.name + "_t"))
        pp = write_text_db(os.path.join(d, self.name + "_pref" + tag), self.pref_entries(keep), DBTYPE_PREF_REV if self.rev else DBTYPE_PREF)
        return qp, tp, pp

    def restate(self, par, keep=None, same=None):
        pref = [(qk, [l for l in lines if keep is None or keep(qk, l[0])]) for qk, lines in self.pref]
        ent, pairs = restate(self.q, self.t, self.same if same is None else same, pref, self.rev, par)
        for p in pairs:
            p["cls"] = self.cls[(p["q"], p["t"])]
        return ent, pairs


# ------------------------------------------------------------------------------------------------------------------ the ladders
OVERLAPS = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 127, 128, 129, 130, 255, 256, 257)
MINS = (767, 768, 769, 770)


def _query_aln(lad, q, reverse):
    return reverse_query(q) if reverse else q


def _geometry_pairs(lad, reverse=False, forced_all=True, near_start=False):
    """min(qLen, tLen) on both sides of RS_SHORT_MAX, the other sequence equal or 300 longer; every overlap of OVERLAPS and the whole
    shorter sequence, on a positive and on a negative diagonal; per geometry one target per forced edge column"""
    rng, nucl = lad.rng, lad.nucl
    for m in MINS:
        for q_len, t_len in ((m, m), (m + 300, m), (m, m + 300)):
            q = random_seq(rng, q_len, nucl)
            if reverse:      # every IUPAC letter in the columns nearest the stored query's start and end
                q[:16] = np.frombuffer(IUPAC, dtype=np.uint8); q[-16:] = np.frombuffer(IUPAC, dtype=np.uint8)[::-1]
                q[40:56] = np.frombuffer(IUPAC, dtype=np.uint8)
            qi = lad.q.add(q)
            qa = _query_aln(lad, q, reverse)
            for ov in OVERLAPS + (m,):
                for sign in (1, -1):
                    d = diag_for(q_len, t_len, ov, sign)
                    if d is None:
                        continue
                    side = "1thread" if m <= RS_SHORT_MAX else "16lanes"
                    cls = "%s/%s/ov%s" % (side, "pos" if sign > 0 else "neg", "all" if ov == m else ov)
                    for forced in ([None] + list(range(len(EDGE_COLS))) if forced_all else [None, int(rng.integers(0, len(EDGE_COLS)))]):
                        lad.pair(qi, lad.t.add(plant(rng, qa, t_len, d, nucl, forced)), d, cls, reverse)
            if near_start:
                # overlaps whose last column is the k-th stored residue of the query (k = 1: its first): the reverse-strand fetch reads
                # the stored query byte by byte there.  A target as long as the overlap (one thread), and a target five residues longer
                # than the query that covers the aligned query from its start (the kernel min(qLen, tLen) = qLen selects)
                for k in range(1, 16):
                    for ov in (1, 9, 17, 33, 130):
                        d = q_len - k - ov + 1
                        lad.pair(qi, lad.t.add(plant(rng, qa, ov, d, nucl, int(rng.integers(0, len(EDGE_COLS))))), d, "nearstart/1thread/k%d" % k, reverse)
                    d = -(k + 4)
                    assert overlap_of(q_len, q_len + 5, d)[2] == q_len + 1 - k
                    lad.pair(qi, lad.t.add(plant(rng, qa, q_len + 5, d, nucl, int(rng.integers(0, len(EDGE_COLS))))), d,
                             "nearstart/%s/k%d" % ("1thread" if q_len <= RS_SHORT_MAX else "16lanes", k), reverse)
            # a diagonal that meets neither sequence on any wrap
            lad.pair(qi, lad.t.add(random_seq(rng, t_len, nucl)), 30000, "miss", reverse)


def _short_block(lad, reverse=False):
    rng, nucl = lad.rng, lad.nucl
    for L in range(1, 41):
        q = random_seq(rng, L, nucl)
        qi = lad.q.add(q)
        qa = _query_aln(lad, q, reverse)
        for t_len, d in ((L, 0), (L + 3, -3), (max(1, L - 1), 1 if L > 1 else 0), (L + 40, -20)):
            if overlap_of(L, t_len, d) is None:
                continue
            lad.pair(qi, lad.t.add(plant(rng, qa, t_len, d, nucl, int(rng.integers(0, len(EDGE_COLS))))), d, "short/%d" % min(L, 9), reverse)


@functools.lru_cache(maxsize=None)
def geometry(nucl):
    lad = Ladder("geo_nucl" if nucl else "geo_aa", nucl, seed=11 + nucl)
    _geometry_pairs(lad)
    _short_block(lad)
    return lad.finish()


@functools.lru_cache(maxsize=None)
def reverse_strand():
    lad = Ladder("rev_nucl", True, rev=True, seed=21)
    _geometry_pairs(lad, reverse=True, forced_all=False, near_start=True)
    _short_block(lad, reverse=True)
    # forward lines in the same reverse-capable DB
    q = random_seq(lad.rng, 900, True)
    qi = lad.q.add(q)
    for d in (0, 100, -100, 890):
        lad.pair(qi, lad.t.add(plant(lad.rng, q, 900, d, True, 0)), d, "forward-in-rev")
    return lad.finish()


STAR_KINDS = ("q0", "t0", "both0", "qlast", "tlast", "bothlast", "one", "two", "mid", "q0_tlast")


@functools.lru_cache(maxsize=None)
def stars():
    """'*' at the ends of the overlap, in an overlap of one column and of two, and in the middle; on both sides of RS_SHORT_MAX"""
    lad = Ladder("star_aa", False, seed=31)
    rng = lad.rng
    for m in (768, 769):
        for q_len, t_len in ((m, m), (m + 300, m), (m, m + 300)):
            for kind in STAR_KINDS:
                for sign in (1, -1):
                    ovs = {"one": (1,), "two": (2,)}.get(kind, (5, 16, 17, 130, m))
                    for ov in ovs:
                        d = diag_for(q_len, t_len, ov, sign)
                        if d is None:
                            continue
                        q = random_seq(rng, q_len, False)
                        t = plant(rng, q, t_len, d, False, None)
                        qo, to, n = overlap_of(q_len, t_len, d)
                        qs, ts = [], []
                        if kind in ("q0", "both0", "q0_tlast", "one", "two"):
                            qs.append(0)
                        if kind in ("t0", "both0", "one", "two"):
                            ts.append(0)
                        if kind in ("qlast", "bothlast", "two"):
                            qs.append(n - 1)
                        if kind in ("tlast", "bothlast", "q0_tlast", "two"):
                            ts.append(n - 1)
                        if kind == "mid":
                            qs.append(n // 2); ts.append(min(n - 1, n // 2 + 1))
                        if kind == "one" and sign < 0:
                            ts = []                           # the single column a '*' in the query only
                        for c in qs:
                            q[qo + c] = STAR
                        for c in ts:
                            t[to + c] = STAR
                        side = "1thread" if m <= RS_SHORT_MAX else "16lanes"
                        lad.pair(lad.q.add(q), lad.t.add(t), d, "%s/%s" % (side, kind))
    return lad.finish()


WRAP_SIZES = ((70000, 70000), (140000, 40000), (1000, 100000), (65535, 32767), (65536, 32768),
              (700, 100000))      # (the last one: several wraps on the thread-per-pair kernel)


@functools.lru_cache(maxsize=None)
def wraps(reverse):
    lad = Ladder("wrap_rev" if reverse else "wrap_fwd", True, rev=reverse, seed=41 + reverse)
    rng = lad.rng
    for q_len, t_len in WRAP_SIZES:
        q = random_seq(rng, q_len, True)
        qi = lad.q.add(q)
        qa = _query_aln(lad, q, reverse)
        n_neg, n_pos = 1 + t_len // 32768, 1 + q_len // 65536
        for w in range(n_neg + n_pos):
            # a true diagonal on wrap w that meets both sequences, if there is one
            lo, hi = (-(w + 1) * 65536, -(w + 1) * 65536 + 65535) if w < n_neg else ((w - n_neg) * 65536, (w - n_neg) * 65536 + 65535)
            lo, hi = max(lo, -(t_len - 1)), min(hi, q_len - 1)
            if lo > hi:
                continue
            for d in sorted({lo, hi, int(rng.integers(lo, hi + 1))}):
                lad.pair(qi, lad.t.add(plant(rng, qa, t_len, d, True, int(rng.integers(0, len(EDGE_COLS))))), d, "wrap/%dx%d/w%d" % (q_len, t_len, w), reverse)
    # a tie: q = t with period 64, diagonal word 32768: wraps -32768 and +32768 score the same, the first (negative) one wins
    unit = random_seq(rng, 64, True)
    per = np.tile(unit, 70000 // 64 + 1)[:70000]
    lad.pair(lad.q.add(per), lad.t.add(reverse_query(per) if reverse else per.copy()), 32768, "tie", reverse)
    # a later wrap strictly better: the target copies the query on +1000 and, over its last 5464 residues, on 1000 - 65536
    q = random_seq(rng, 70000, True)
    qa = _query_aln(lad, q, reverse)
    t = plant(rng, qa, 70000, 1000, True, 0)
    t[64536:70000] = qa[:5464]
    lad.pair(lad.q.add(q), lad.t.add(t), 1000, "later-wrap-better", reverse)
    return lad.finish(alias=False)


def _exact_target(rng, q, t_len, d, n_subs, nucl=False):
    qo, to, n = overlap_of(len(q), t_len, d)
    return plant(rng, q, t_len, d, nucl, subs=[int(i) for i in rng.choice(n, size=n_subs, replace=False)])


COV_RATIOS = ((7, 10, "0.7"), (9, 10, "0.9"), (4, 5, "0.8"), (3, 10, "0.3"))


@functools.lru_cache(maxsize=None)
def gates():
    """length ratios and coverages on the -c thresholds and just under them, identity counts on --min-seq-id and next to it, alignment
    lengths on --min-aln-len and next to it; every ratio was chosen as the float32 quotient the reference computes"""
    lad = Ladder("gates_aa", False, seed=51)
    rng = lad.rng
    for a, b, _ in COV_RATIOS:
        for k in (10, 110):
            for short in (k * a, k * a - 1, k * a + 1):
                for q_len, t_len in ((short, k * b), (k * b, short)):         # the ratio below 1 and above 1
                    q = random_seq(rng, q_len, False)
                    d = 0 if q_len <= t_len else q_len - t_len
                    lad.pair(lad.q.add(q), lad.t.add(plant(rng, q, t_len, d, False, None, rate=0.03)), d, "len/%d:%d" % (a, b))
            # coverage: equal lengths k*b, k*a (or one fewer) columns aligned; and a longer target with the same columns
            for ov in (k * a, k * a - 1):
                for t_len in (k * b, k * b + 2 * k):
                    for sign in (1, -1):
                        d = diag_for(k * b, t_len, ov, sign)
                        if d is None:
                            continue
                        q = random_seq(rng, k * b, False)
                        lad.pair(lad.q.add(q), lad.t.add(plant(rng, q, t_len, d, False, None, rate=0.03)), d, "cov/%d:%d" % (a, b))
    # identities: 100 aligned columns of qLen 125 / tLen 100 (modes 0 and 1 over 100, mode 2 over 125); 110 aligned columns of qLen 150 /
    # tLen 125 (mode 1 over 125): 90/100, 91/100, 90/125, 91/125, 100/125 and 101/125 are the float32 the flags' texts parse to
    for q_len, t_len, d, n, ids in [(125, 100, 10, 100, i) for i in (88, 89, 90, 91, 92)] + [(150, 125, 40, 110, i) for i in (98, 99, 100, 101, 102)]:
        q = random_seq(rng, q_len, False)
        assert overlap_of(q_len, t_len, d)[2] == n
        lad.pair(lad.q.add(q), lad.t.add(_exact_target(rng, q, t_len, d, n - ids)), d, "ids/%d" % t_len)
    # the same on the 16-lane side: 1000 aligned columns of qLen 1200 / tLen 1000
    for ids in (899, 900, 909, 910, 911):
        q = random_seq(rng, 1200, False)
        lad.pair(lad.q.add(q), lad.t.add(_exact_target(rng, q, 1000, 100, 1000 - ids)), 100, "ids/1000")
    # alignment lengths 99, 100, 101 (and 100 with a '*' trimmed at its end: alnLen 99)
    for ov in (99, 100, 101):
        q = random_seq(rng, 300, False)
        lad.pair(lad.q.add(q), lad.t.add(plant(rng, q, ov, 50, False, None, rate=0.03)), 50, "alnlen/%d" % ov)
    q = random_seq(rng, 300, False)
    t = plant(rng, q, 100, 50, False, None, rate=0.03); t[99] = STAR
    lad.pair(lad.q.add(q), lad.t.add(t), 50, "alnlen/100*")
    return lad.finish()


def _flags(**kw):
    p = dict(e=1e-5, min_seq_id="0.9", cov_mode=0, c="0", min_aln_len=0, seq_id_mode=0, a=0, add_self=0)
    p.update(kw)
    return p


GATE_FLAGS = [("cov%d_c%s" % (m, c), _flags(cov_mode=m, c=c, min_seq_id="0")) for m in range(6) for _, _, c in COV_RATIOS] + [
    ("idmode0_090", _flags(min_seq_id="0.9")), ("idmode0_091", _flags(min_seq_id="0.91")),
    ("idmode1_080", _flags(min_seq_id="0.8", seq_id_mode=1)), ("idmode1_0808", _flags(min_seq_id="0.808", seq_id_mode=1)),
    ("idmode2_072", _flags(min_seq_id="0.72", seq_id_mode=2)), ("idmode2_0728", _flags(min_seq_id="0.728", seq_id_mode=2)),
    ("alnlen100", _flags(min_aln_len=100, min_seq_id="0")), ("alnlen101", _flags(min_aln_len=101, min_seq_id="0")),
    ("backtrace", _flags(a=1, min_seq_id="0"))]
STRICT = _flags()
OPEN = _flags(e=1e12, min_seq_id="0")

E_QLENS = (20, 33, 100, 768, 769, 5000)
E_VALUES = (1e-5, 1e-3, 10.0)
E_DB_RESIDUES = (120000, 230000)     # (nucleotides: at both sizes the minimum of a 20-residue query and its neighbour below are scores 20 columns can give)


def _attainable_nucl(T, n_max):
    """(columns, substitutions) of a nucleotide overlap that scores T = 2 (n - a) - 3 a, or None"""
    for a in range(0, 8):
        if (T + 5 * a) % 2 == 0 and 1 <= (T + 5 * a) // 2 <= n_max and a < (T + 5 * a) // 2:
            return (T + 5 * a) // 2, a
    return None


@functools.lru_cache(maxsize=None)
def egate(nucl, big):
    """per query length and -e a family of targets whose raw scores fall in steps of 1 across the minimum passing score of that length in
    a target DB of exactly E_DB_RESIDUES[big] residues.  Protein: the query is AIAI..., A -> S costs 3 and I -> V costs 1;
    nucleotides: 2 (n - a) - 3 a over the overlap length n and the substitutions a (the matrix alone steps by 5).  Queries above
    RS_SHORT_MAX meet targets of 800 residues on a negative diagonal (16 lanes); the others meet targets as long as the overlap"""
    db_res = E_DB_RESIDUES[big]
    lad = Ladder("egate_%s_%d" % ("nucl" if nucl else "aa", big), nucl, seed=61 + 2 * nucl + big)
    rng = lad.rng
    lad.thresholds = {}
    for q_len in E_QLENS:
        q = random_seq(rng, q_len, True) if nucl else np.tile(np.frombuffer(b"AI", dtype=np.uint8), q_len // 2 + 1)[:q_len]
        qi = lad.q.add(q)
        for e in E_VALUES:
            T0 = min_score_for(nucl, db_res, q_len, e)
            lad.thresholds[(q_len, e)] = T0
            for T in range(T0 - 3, T0 + 4):
                if nucl:
                    na = _attainable_nucl(T, q_len)
                    if na is None:
                        continue
                    n, subs = na[0], [int(i) for i in rng.choice(na[0], size=na[1], replace=False)]
                else:
                    n = T // 4 + 2
                    if n > q_len:
                        n = q_len
                    cost = 4 * n - T
                    if cost < 0:
                        continue
                    subs = None
                long_t = q_len > RS_SHORT_MAX
                t_len = 800 if long_t else n
                d = -(800 - n) if long_t else int(rng.integers(0, q_len - n + 1))
                qo, to, cols = overlap_of(q_len, t_len, d)
                assert cols == n
                if not nucl:
                    region = q[qo:qo + n]
                    a_pos, i_pos = np.nonzero(region == ord("A"))[0], np.nonzero(region == ord("I"))[0]
                    na_, nb_ = cost // 3, cost % 3
                    while na_ > len(a_pos) and na_ > 0:        # too few A: pay three I -> V for one A -> S
                        na_ -= 1; nb_ += 3
                    assert na_ <= len(a_pos) and nb_ <= len(i_pos), "the query region cannot give this score"
                    t = random_seq(rng, t_len, False)
                    colsv = region.copy()
                    colsv[rng.permutation(a_pos)[:na_]] = ord("S"); colsv[rng.permutation(i_pos)[:nb_]] = ord("V")
                    t[to:to + n] = colsv
                else:
                    t = plant(rng, q, t_len, d, True, subs=subs)
                lad.pair(qi, lad.t.add(t), d, "e/%d/%g/%d" % (q_len, e, T))
    # fill the target DB up to exactly db_res residues (one more entry is added by finish(): 17 residues)
    have = sum(len(s) for s in lad.t.seqs) + 17
    assert have < db_res
    left = db_res - have
    while left > 0:
        n = min(left, 50000)
        lad.t.add(random_seq(rng, n, nucl)); left -= n
    lad.finish(lower=False, alias=False)
    assert lad.t.residues() == db_res
    return lad


@functools.lru_cache(maxsize=None)
def identity(nucl=False):
    """one DB on both sides: self lines (once per entry) next to lines to other entries; self pairs on both sides of RS_SHORT_MAX; a
    sequence of X only (its self pair scores 0); a query of 800 residues with 70 short targets (a queue beyond 64 alignments)"""
    lad = Ladder("self_nucl" if nucl else "self_aa", nucl, same=True, seed=71 + nucl)
    rng = lad.rng
    for L in (767, 768, 769, 770, 1500, 60, 61, 1, 2, 16, 17):
        q = random_seq(rng, L, nucl)
        qi = lad.q.add(q)
        lad.pair(qi, qi, 0, "self/%s" % ("1thread" if L <= RS_SHORT_MAX else "16lanes"))
        if L >= 60:
            for d in (0, 7, -7):
                ti = lad.q.add(plant(rng, q, L, d, nucl, 0, rate=0.04))
                lad.pair(qi, ti, d, "other")
                lad.pair(ti, ti, 0, "self/%s" % ("1thread" if L <= RS_SHORT_MAX else "16lanes"))
                lad.pair(ti, qi, -d, "other")
            lad.pair(qi, lad.q.add(plant(rng, q, L, 3, nucl, 0, rate=0.3)), 3, "other")          # too few identities
    xs = lad.q.add(np.full(30, ord("N" if nucl else "X"), dtype=np.uint8))
    lad.pair(xs, xs, 0, "self/X")
    xl = lad.q.add(np.full(800, ord("N" if nucl else "X"), dtype=np.uint8))
    lad.pair(xl, xl, 0, "self/X")
    s5 = lad.q.add(random_seq(rng, 900, nucl))
    lad.pair(s5, s5, 5, "self/offdiag")                 # a self line on another diagonal: accepted all the same
    if not nucl:
        q = random_seq(rng, 800, False)
        qi = lad.q.add(q)
        lad.pair(qi, qi, 0, "self/16lanes")
        for j in range(70):
            n = int(rng.integers(50, 71))
            # targets over either end (they extend the query) and inside it
            if j < 12:
                d = -int(rng.integers(5, 30))           # the target starts in front of the query
                t = random_seq(rng, n, False); t[-d:] = q[:n + d]
            elif j < 24:
                d = 800 - int(rng.integers(20, 45))     # the target runs past the query's end
                t = random_seq(rng, n, False); t[:800 - d] = q[d:]
            else:
                d = int(rng.integers(0, 800 - n))
                t = q[d:d + n].copy()
            for i in np.nonzero(rng.random(n) < 0.02)[0]:
                t[i] = _other_letter(rng, t[i], False)
            ti = lad.q.add(t)
            lad.pair(qi, ti, d, "queue70")
            lad.pair(ti, ti, 0, "self/1thread")
        lad.big_query = qi
    lad.finish(lower=not nucl, alias=False)
    if not nucl:
        lad.big_query_key = lad.q.key(lad.big_query)
    return lad


# ------------------------------------------------------------------------------------------------------------------ cases
def oracle_flags(par):
    return ["--rescore-mode", "3", "-e", repr(float(par["e"])), "-c", par["c"], "-a", str(par["a"]), "--cov-mode", str(par["cov_mode"]),
            "--min-seq-id", par["min_seq_id"], "--min-aln-len", str(par["min_aln_len"]), "--seq-id-mode", str(par["seq_id_mode"]),
            "--add-self-matches", str(par["add_self"])]


def numeric(par):
    return dict(par, c=float(par["c"]), min_seq_id=float(par["min_seq_id"]))


def param_kwargs(par):
    return dict(e=float(par["e"]), min_seq_id=float(par["min_seq_id"]), cov_mode=par["cov_mode"], c=float(par["c"]), min_aln_len=par["min_aln_len"],
                seq_id_mode=par["seq_id_mode"], a=bool(par["a"]), add_self_matches=bool(par["add_self"]))


def _cases():
    """name -> (ladder builder, its arguments, flags, 'open': the prefilter DB without the pairs that score 0)"""
    c = {}
    for tag, fn, args in (("geo_aa", geometry, (0,)), ("geo_nucl", geometry, (1,)), ("star_aa", stars, ()), ("rev_nucl", reverse_strand, ()),
                          ("wrap_fwd", wraps, (0,)), ("wrap_rev", wraps, (1,))):
        c[tag + "_strict"] = (fn, args, STRICT, False)
        c[tag + "_open"] = (fn, args, OPEN, True)
    for name, par in GATE_FLAGS:
        c["gates_" + name] = (gates, (), par, False)
    for nucl in (0, 1):
        for big in (0, 1):
            for e in E_VALUES:
                c["egate_%s_%d_e%g" % ("nucl" if nucl else "aa", big, e)] = (egate, (nucl, big), _flags(e=e, min_seq_id="0"), False)
    return c


CASES = _cases()
GROUPS = {"geometry": [n for n in CASES if n.startswith("geo_")], "stars": [n for n in CASES if n.startswith("star_")],
          "reverse": [n for n in CASES if n.startswith("rev_")], "wraps": [n for n in CASES if n.startswith("wrap_")],
          "gates": [n for n in CASES if n.startswith(("gates_", "egate_"))]}


@functools.lru_cache(maxsize=None)
def case_restated(name):
    """-> (ladder, flags, keep, entries, pairs) of a case; `keep` selects the prefilter lines of the case"""
    fn, args, par, open_ = CASES[name]
    lad = fn(*args)
    keep = None
    if open_:
        scored = {(p["q"], p["t"]) for p in case_restated(name[:-5] + "_strict")[4] if p["score"] > 0}    # (the score does not depend on the flags)
        keep = lambda qk, tk: (qk, tk) in scored          # noqa: E731
    ent, pairs = lad.restate(numeric(par), keep)
    return lad, par, keep, ent, pairs


def assert_same_entries(want, got, what):
    assert want.keys() == got.keys(), "%s: key sets differ" % what
    bad = sorted(k for k in want if want[k] != got[k])
    if bad:
        w, g = want[bad[0]].split(b"\n"), got[bad[0]].split(b"\n")
        first = next((i for i in range(min(len(w), len(g))) if w[i] != g[i]), min(len(w), len(g)))
        raise AssertionError("%s: %d entries differ (keys %s); key %d, line %d:\n  restated %r\n  got      %r" % (
            what, len(bad), bad[:8], bad[0], first, w[first:first + 2], g[first:first + 2]))
