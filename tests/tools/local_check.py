"""Plain sequential Python restatement of the reference's `rescorediagonal --rescore-mode 2` (the best-scoring ungapped local segment on
the candidate's diagonal) and of its `mergeclusters`: what plasship_rescore_local has to compute, line for line.  It is pinned byte for byte
on the DBs the unmodified reference wrote (tests/golden/local.tar.gz, --filter-hits 0 and 1) and on the CPU oracle's `rescorediagonal
--rescore-mode 2` (tests/test_local_host.py), which restates the same reference code in C++ and does not have --filter-hits.

Restated (lib/mmseqs/src): alignment/rescorediagonal.cpp:193-334 (doRescorediagonal, RESCORE_MODE_ALIGNMENT), alignment/DistanceCalculator.h:
93-201 (computeUngappedAlignment, ungappedAlignmentByDiagonal, computeSubstitutionStartEndDistance), alignment/StripedSmithWaterman.cpp:
1055-1057 (computeCov), commons/Util.cpp:533-598, alignment/Matcher.cpp:323-370 (resultToBuffer).  The substitution matrix and the E-value
come from the oracle's library (oracle/build/liboracle.so: oracle_ascii_submat, oracle_evalue, oracle_bitscore)."""
import ctypes as C
import os

import numpy as np

import hamming_check as hc
from hamming_check import F32, FLT_EPSILON, read_db, read_seqdb  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
_oracle = None


def oracle_lib():
    global _oracle
    if _oracle is None:
        lib = C.CDLL(os.path.join(ROOT, "oracle", "build", "liboracle.so"))
        lib.oracle_ascii_submat.restype = C.POINTER(C.c_byte); lib.oracle_ascii_submat.argtypes = [C.c_int]
        lib.oracle_evalue.restype = C.c_double; lib.oracle_evalue.argtypes = [C.c_int, C.c_ulonglong, C.c_double, C.c_double]
        lib.oracle_bitscore.restype = C.c_double; lib.oracle_bitscore.argtypes = [C.c_int, C.c_double]
        _oracle = lib
    return _oracle


def sub_mat(nucl):
    """the ASCII-indexed score table (SubstitutionMatrix::createAsciiSubMat), 123 x 123"""
    p = oracle_lib().oracle_ascii_submat(1 if nucl else 0)
    return np.ctypeslib.as_array(p, shape=(123 * 123,)).astype(np.int32).reshape(123, 123)


def parse_flags(text):
    """flags of a command line -> parameters (the reference module's defaults where a flag is absent); thr: --score-per-col-thr or None"""
    p = dict(min_seq_id=0.0, seq_id_mode=0, cov_mode=0, c=0.0, min_aln_len=0, e=1e-3, rescore_mode=0, a=0, filter_hits=0, thr=None)
    names = {"--min-seq-id": ("min_seq_id", float), "--seq-id-mode": ("seq_id_mode", int), "--cov-mode": ("cov_mode", int), "-c": ("c", float),
             "--min-aln-len": ("min_aln_len", int), "-e": ("e", float), "--rescore-mode": ("rescore_mode", int), "-a": ("a", int),
             "--filter-hits": ("filter_hits", int), "--score-per-col-thr": ("thr", float)}
    w = text.split() if isinstance(text, str) else list(text)
    for i in range(0, len(w), 2):
        if w[i] in names:
            p[names[w[i]][0]] = names[w[i]][1](w[i + 1])
    return p


def start_end_distance(scores):
    """computeSubstitutionStartEndDistance over the columns' scores -> (maxScore, maxStartPos, maxEndPos)"""
    max_score, max_end, max_start, min_pos, score = 0, 0, 0, -1, 0
    for pos, curr in enumerate(scores):
        score += curr
        if score <= 0:
            score = 0
            min_pos = pos
        if score > max_score:
            max_end, max_start, max_score = pos, min_pos + 1, score
    return max_score, max_start, max_end


def _by_diagonal(q, t, diagonal, mat):
    """ungappedAlignmentByDiagonal, RESCORE_MODE_ALIGNMENT -> (score, start, end, diagonalLen, distToDiagonal, diagonal); a diagonal that
    misses the sequences keeps the default constructor's start = end = -1"""
    dist = abs(diagonal)
    if diagonal >= 0 and dist < len(q):
        n = min(len(t), len(q) - dist)
        s, a, b = start_end_distance(mat[q[dist:dist + n], t[:n]].tolist())
        return s, a, b, n, dist, diagonal
    if diagonal < 0 and dist < len(t):
        n = min(len(t) - dist, len(q))
        s, a, b = start_end_distance(mat[q[:n], t[dist:dist + n]].tolist())
        return s, a, b, n, dist, diagonal
    return 0, -1, -1, 0, dist, diagonal


def ungapped_alignment(q, t, d16, mat):
    """computeUngappedAlignment: the default LocalAlignment unless a wrap scores strictly more"""
    best = (0, -1, -1, 0, 0, 0)
    for d in range(1, 1 + len(t) // 32768 + 1):
        r = _by_diagonal(q, t, -d * 65536 + d16, mat)
        if r[0] > best[0]:
            best = r
    for d in range(0, len(q) // 65536 + 1):
        r = _by_diagonal(q, t, d * 65536 + d16, mat)
        if r[0] > best[0]:
            best = r
    return best


def merge_clusters(seq_keys, first, second):
    """mergeclusters with two clusterings (lib/mmseqs/src/util/mergeclusters.cpp:28-145).  seq_keys: the sequence DB's keys; first, second:
    [(representative key, entry bytes)] -> [(key, entry bytes)] in key order.  Every entry of the first clustering is a list under its
    representative; every entry of the second splices the lists of its members (in its own member order, its own key's list stays where it
    is) behind the list of its key; the writer loop skips a sequence whose list is empty (`continue`): it gets no entry at all."""
    ids = {k: i for i, k in enumerate(sorted(seq_keys))}
    merged = [[] for _ in ids]
    for key, entry in first:
        merged[ids[key]] += [ids[int(l.split()[0])] for l in entry.split(b"\n") if l.strip(b"\0")]
    for key, entry in second:
        clu = ids[key]
        for l in entry.split(b"\n"):
            if l.strip(b"\0"):
                s = ids[int(l.split()[0])]
                if s != clu:
                    merged[clu] += merged[s]
                    merged[s] = []
    keys = sorted(seq_keys)
    return [(keys[i], b"".join(b"%d\n" % keys[m] for m in lst)) for i, lst in enumerate(merged) if lst]


def compute_cov(s, e, length):
    """SmithWaterman::computeCov on unsigned ints (start = end = -1 wraps)"""
    s, e = s & 0xFFFFFFFF, e & 0xFFFFFFFF
    return F32((min(length, max(s, e)) - min(s, e) + 1) & 0xFFFFFFFF) / F32(length)


def fmt_seq_id(x):
    """Util::fastSeqIdToBuffer as Matcher::resultToBuffer uses it"""
    if x == F32(1.0):
        return b"1.00"
    out = b"0."
    if float(x) < 0.10:
        out += b"0"
    if float(x) < 0.01:
        out += b"0"
    return out + b"%d" % int(F32(x) * F32(1000))


def rescore_local(seqs, nucl, pref, pref_dbtype, par, db_residues=None, counts=None):
    """seqs: key -> sequence bytes (one DB is query and target); pref: [(query key, entry bytes)] -> ([(query key, entry bytes)] as the
    reference writes them, [record dicts in the same order]).  par["thr"] is None: --filter-hits 0."""
    if par["rescore_mode"] != 2:
        raise ValueError("the local ungapped alignment is --rescore-mode 2")
    lib = oracle_lib()
    mat = sub_mat(nucl)
    if db_residues is None:
        db_residues = sum(len(s) for s in seqs.values())
    reverse_capable = pref_dbtype == 14
    cov_thr, seq_id_thr = F32(par["c"]), F32(par["min_seq_id"])
    arr = {}

    def seq(k):
        if k not in arr:
            arr[k] = np.frombuffer(seqs[k], dtype=np.uint8)
        return arr[k]

    def tally(name, ok):
        if counts is not None:
            counts.setdefault(name, [0, 0])[0 if ok else 1] += 1

    out, records = [], []
    for qkey, entry in pref:
        text = b""
        lines = [l for l in entry.split(b"\n") if l]
        if lines:
            q = seq(qkey)
            L = len(q)
            rev = hc.reverse_strand(q) if reverse_capable else None
        for line in lines:
            w = line.split()
            tkey, pref_score, d16 = int(w[0]), int(w[1]), int(w[2]) & 0xFFFF
            is_reverse = reverse_capable and pref_score < 0
            q_aln = rev if is_reverse else q
            t = seq(tkey)
            db_len = len(t)
            is_identity = qkey == tkey
            ok = hc._can_be_covered(cov_thr, par["cov_mode"], F32(L), F32(db_len))
            tally("canBeCovered", ok)
            if not ok:
                continue
            score, start, end, diag_len, dist, diagonal = ungapped_alignment(q_aln, t, d16, mat)
            evalue = lib.oracle_evalue(1 if nucl else 0, db_residues, float(score), float(L))
            bit_score = int(lib.oracle_bitscore(1 if nucl else 0, float(score)) + 0.5)
            aln_len = end - start + 1
            if diagonal >= 0:
                qs, qe, ds, de = start + dist, end + dist, start, end
            else:
                qs, qe, ds, de = start, end, start + dist, end + dist
            seq_id = F32(0.0)
            has_evalue = evalue <= par["e"]
            if has_evalue or is_identity:
                if start < 0:
                    # the reference compares the bytes before both strings; for an identity pair on the forward strand they are the same byte
                    ids = 1 if is_identity else 0
                else:
                    ids = int(np.count_nonzero((q_aln[qs:qe + 1] & 0xDF) == (t[ds:de + 1] & 0xDF)))
                mode = par["seq_id_mode"]
                den = aln_len if mode == 0 else min(L, db_len) if mode == 1 else max(L, db_len)
                seq_id = F32(ids) / F32(den) if mode in (0, 1, 2) else F32(0.0)
            query_cov, target_cov = compute_cov(qs, qe, L), compute_cov(ds, de, db_len)
            if is_reverse:
                qs, qe = L - qs - 1, L - qe - 1
            with np.errstate(divide="ignore", invalid="ignore"):
                per_col = F32(score) / F32(diag_len)
            has_cov = hc._has_coverage(cov_thr, par["cov_mode"], query_cov, target_cov)
            has_seq_id = bool(float(seq_id) >= float(seq_id_thr - FLT_EPSILON))
            has_aln_len = aln_len >= par["min_aln_len"]
            has_to_filter = par["thr"] is not None and bool(per_col >= F32(par["thr"]))
            if not is_identity:
                for name, v in (("hasCov", has_cov), ("hasSeqId", has_seq_id), ("hasAlnLen", has_aln_len), ("hasEvalue", has_evalue), ("hasToFilter", has_to_filter)):
                    tally(name, v)
            if is_identity or has_to_filter or (has_aln_len and has_cov and has_seq_id and has_evalue):
                text += b"%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d" % (tkey, bit_score, fmt_seq_id(seq_id), ("%.3E" % evalue).encode(), qs, qe, L, ds, de, db_len)
                if par["a"]:
                    text += b"\t%dM" % aln_len
                text += b"\n"
                records.append(dict(query=qkey, target=tkey, bit_score=bit_score, raw_score=score, seq_id=seq_id, q_start=qs, q_end=qe, q_len=L,
                                    db_start=ds, db_end=de, db_len=db_len, aln_len=aln_len, reversed=int(is_reverse), diagonal=diagonal, per_col=per_col))
        out.append((qkey, text))
    return out, records
