"""Plain Python restatement of the reference's `rescorediagonal --rescore-mode 0 [--wrapped-scoring 1]` (the Hamming score): what
plasship_rescore_hamming has to compute, line for line.  It stands where the CPU oracle stands for the other modules and is itself pinned
byte for byte to the reference's DBs in tests/golden/hamming.tar.gz (tests/test_hamming_host.py).

Restated (lib/mmseqs/src): alignment/rescorediagonal.cpp:146-356 (doRescorediagonal, RESCORE_MODE_HAMMING), alignment/DistanceCalculator.h:57-175,
276-295 (computeUngappedWrappedAlignment, computeUngappedAlignment, ungappedAlignmentByDiagonal, computeInverseHammingDistance),
commons/NucleotideMatrix.cpp:4-61 (the reverse strand's letters), commons/Util.cpp:533-598, prefiltering/QueryMatcher.h:81-126."""
import os

import numpy as np

F32 = np.float32
FLT_EPSILON = np.finfo(np.float32).eps
INT_MIN = -2147483648
U32 = 0xFFFFFFFF
FILTERS = ("canBeCovered", "wrappedTargetFits", "hasCov", "hasSeqId", "hasAlnLen")


def read_db(path):
    """(list of (key, entry bytes without the trailing NUL) in index order, dbtype)"""
    data = open(path, "rb").read()
    ent = []
    for line in open(path + ".index", "rb"):
        k, o, l = (int(x) for x in line.split()[:3])
        ent.append((k, data[o:o + l - 1]))
    dbtype = int.from_bytes(open(path + ".dbtype", "rb").read(4), "little") & 0x3FFFFFFF
    return ent, dbtype


def read_seqdb(path):
    ent, dbtype = read_db(path)
    return {k: e[:-1] if e.endswith(b"\n") else e for k, e in ent}, dbtype


def parse_flags(text):
    """the flags of a RUNS line of the fixture -> parameters (the reference's defaults where a flag is absent)"""
    p = dict(wrapped=0, min_seq_id=0.0, seq_id_mode=0, cov_mode=0, c=0.0, min_aln_len=0, e=1e-3, rescore_mode=0)
    names = {"--wrapped-scoring": ("wrapped", int), "--min-seq-id": ("min_seq_id", float), "--seq-id-mode": ("seq_id_mode", int),
             "--cov-mode": ("cov_mode", int), "-c": ("c", float), "--min-aln-len": ("min_aln_len", int), "-e": ("e", float),
             "--rescore-mode": ("rescore_mode", int)}
    w = text.split()
    for i in range(0, len(w), 2):
        if w[i] in names:
            p[names[w[i]][0]] = names[w[i]][1](w[i + 1])
    return p


def _comp_table():
    t = np.full(256, ord("X"), dtype=np.uint8)
    for letters, to in (("A", "T"), ("CMYH", "G"), ("TUW", "A"), ("GKBDVRS", "C")):
        for ch in letters:
            t[ord(ch)] = ord(to); t[ord(ch.lower())] = ord(to)
    return t


COMP = _comp_table()


def reverse_strand(q):
    """queryRevSeq: num2aa[reverseResidue(aa2num[c])] from the last residue to the first"""
    return COMP[q[::-1]]


def _can_be_covered(thr, mode, q, t):
    with np.errstate(divide="ignore", invalid="ignore"):
        if mode == 0:
            return bool(q / t >= thr and t / q >= thr)
        if mode == 1:
            return bool(q / t >= thr)
        if mode == 2:
            return bool(t / q >= thr)
        if mode == 3:
            return bool(t / q >= thr and t / q <= F32(1.0))
        if mode == 4:
            return bool(q / t >= thr and q / t <= F32(1.0))
        if mode == 5:
            return bool(min(t, q) / max(t, q) >= thr)
    return True


def _has_coverage(thr, mode, qc, tc):
    if mode == 0:
        return bool(qc >= thr and tc >= thr)
    if mode == 1:
        return bool(tc >= thr)
    if mode == 2:
        return bool(qc >= thr)
    return True


def _equal(a, b):
    return int(np.count_nonzero(a == b))


def _by_diagonal(q, t, diagonal):
    """ungappedAlignmentByDiagonal for the Hamming mode -> (score, diagonalLen)"""
    dist = abs(diagonal)
    if diagonal >= 0 and dist < len(q):
        n = min(len(t), len(q) - dist)
        return _equal(q[dist:dist + n], t[:n]), n
    if diagonal < 0 and dist < len(t):
        n = min(len(t) - dist, len(q))
        return _equal(q[:n], t[dist:dist + n]), n
    return 0, 0


def wrapped_alignment(dq, t, d16):
    """computeUngappedWrappedAlignment: dq is the doubled query -> (score, diagonal, diagonalLen)"""
    L, db_len = len(dq) // 2, len(t)
    best, best_diag = 0, 0
    d = 1
    while ((-d * 65536 + d16) & U32) > ((-db_len) & U32):
        real = (((-d * 65536 + d16) & U32) + L) & U32
        real = real - (1 << 32) if real >= (1 << 31) else real
        s, _ = _by_diagonal(dq[real:real + L], t, 0)
        if s > best:
            best, best_diag = s, real
        d += 1
    d = 0
    while ((d * 65536 + d16) & U32) < L:
        real = d * 65536 + d16
        s, _ = _by_diagonal(dq[real:real + L], t, 0)
        if s > best:
            best, best_diag = s, real
        d += 1
    return best, best_diag, min(db_len, L)


def ungapped_alignment(q, t, d16):
    """computeUngappedAlignment -> (score, diagonal, diagonalLen)"""
    best, best_diag, best_len = 0, 0, 0
    for d in range(1, 1 + len(t) // 32768 + 1):
        real = -d * 65536 + d16
        s, n = _by_diagonal(q, t, real)
        if s > best:
            best, best_diag, best_len = s, real, n
    for d in range(0, len(q) // 65536 + 1):
        real = d * 65536 + d16
        s, n = _by_diagonal(q, t, real)
        if s > best:
            best, best_diag, best_len = s, real, n
    return best, best_diag, best_len


def rescore_hamming(seqs, nucl, pref, pref_dbtype, par, counts=None):
    """seqs: key -> sequence bytes (query DB == target DB); pref: [(query key, entry bytes)] -> [(query key, entry bytes)] as the reference
    writes them.  counts (optional dict): per filter of FILTERS [lines it let pass, lines it dropped]."""
    if par["rescore_mode"] != 0:
        raise ValueError("the Hamming score is --rescore-mode 0")
    if par["wrapped"] and not nucl:
        raise ValueError("Wrapped scoring is only supported for nucleotides.")
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

    out = []
    for qkey, entry in pref:
        text = b""
        lines = [l for l in entry.split(b"\n") if l]
        if lines:
            q = seq(qkey)
            L = len(q)
            fwd = np.concatenate([q, q]) if par["wrapped"] else q
            rev = reverse_strand(fwd) if reverse_capable else None
        for line in lines:
            w = line.split()
            tkey, pref_score, diag = int(w[0]), int(w[1]), int(w[2]) & 0xFFFF
            is_reverse = reverse_capable and pref_score < 0
            q_aln = rev if is_reverse else fwd
            t = seq(tkey)
            db_len = len(t)
            is_identity = qkey == tkey
            ok = _can_be_covered(cov_thr, par["cov_mode"], F32(L), F32(db_len))
            tally("canBeCovered", ok)
            if not ok:
                continue
            if par["wrapped"]:
                tally("wrappedTargetFits", db_len <= L)
                if db_len > L:
                    continue
                score, diagonal, diag_len = wrapped_alignment(q_aln, t, diag)
            else:
                score, diagonal, diag_len = ungapped_alignment(q_aln, t, diag)
            with np.errstate(divide="ignore", invalid="ignore"):
                target_cov, query_cov = F32(diag_len) / F32(db_len), F32(diag_len) / F32(L)
                mode = par["seq_id_mode"]
                den = diag_len if mode == 0 else min(L, db_len) if mode == 1 else max(L, db_len)
                seq_id = F32(score) / F32(den) if mode in (0, 1, 2) else F32(0.0)
            has_cov = _has_coverage(cov_thr, par["cov_mode"], query_cov, target_cov)
            has_seq_id = bool(float(seq_id) >= float(seq_id_thr - FLT_EPSILON))
            has_evalue = 0.0 <= par["e"]
            has_aln_len = diag_len >= par["min_aln_len"]
            if not is_identity:
                tally("hasCov", has_cov); tally("hasSeqId", has_seq_id); tally("hasAlnLen", has_aln_len)
            if is_identity or (has_aln_len and has_cov and has_seq_id and has_evalue):
                p100 = 100.0 * float(seq_id)
                sc = INT_MIN if (p100 != p100 or abs(p100) >= 2147483648.0) else int(p100)
                if is_reverse and sc != INT_MIN:
                    sc = -sc
                d = diagonal & 0xFFFF
                text += b"%d\t%d\t%d\n" % (tkey, sc, d - 65536 if d >= 32768 else d)
        out.append((qkey, text))
    return out


def run_fixture_case(root, run_line, counts=None):
    """one line of the fixture's RUNS file -> (what the restatement writes, what the reference wrote, the parameters), both key -> entry"""
    name, db, pref, flags = run_line.rstrip("\n").split("\t")
    seqs, dbtype = read_seqdb(os.path.join(root, db))
    pref_ent, pref_type = read_db(os.path.join(root, pref))
    par = parse_flags(flags)
    mine = dict(rescore_hamming(seqs, dbtype == 1, pref_ent, pref_type, par, counts))
    ref_ent, ref_type = read_db(os.path.join(root, "ref", name, "out"))
    return mine, dict(ref_ent), ref_type, pref_type, par
