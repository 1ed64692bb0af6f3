"""Plain sequential Python restatement of the reference's `rescorediagonal --rescore-mode 1` (the best local score on the candidate's
diagonal: linclust's filter step on amino-acid DBs) and of its `result2repseq`: what plasship_rescore_subst and plasship_*_repseqs have to
compute, line for line.  Pinned byte for byte on the DBs the unmodified reference wrote (tests/golden/subst.tar.gz).

Restated (lib/mmseqs/src): alignment/rescorediagonal.cpp:193-334 (doRescorediagonal, RESCORE_MODE_SUBSTITUTION), alignment/DistanceCalculator.h:
16-38,93-175 (computeSubstitutionDistance, computeUngappedAlignment, ungappedAlignmentByDiagonal), prefiltering/QueryMatcher.h:35-38,114-126
(hit_t, prefilterHitToBuffer), util/result2repseq.cpp:37-49.  The substitution matrix and the E-value come from the oracle's library, the
per-pair rules from the Hamming restatement (tests/tools/hamming_check.py), as in tests/tools/local_check.py."""
import numpy as np

import hamming_check as hc
import local_check as lc
from hamming_check import F32, FLT_EPSILON, read_db, read_seqdb  # noqa: F401
from local_check import parse_flags, sub_mat  # noqa: F401


def substitution_distance(scores):
    """computeSubstitutionDistance, globalAlignment = false"""
    best = score = 0
    for curr in scores:
        score = max(0, score + curr)
        best = max(best, score)
    return best


def _by_diagonal(q, t, diagonal, mat):
    """ungappedAlignmentByDiagonal, RESCORE_MODE_SUBSTITUTION -> (score, diagonalLen, diagonal); a diagonal that misses the sequences scores 0"""
    dist = abs(diagonal)
    if diagonal >= 0 and dist < len(q):
        n = min(len(t), len(q) - dist)
        return substitution_distance(mat[q[dist:dist + n], t[:n]].tolist()), n, diagonal
    if diagonal < 0 and dist < len(t):
        n = min(len(t) - dist, len(q))
        return substitution_distance(mat[q[:n], t[dist:dist + n]].tolist()), n, diagonal
    return 0, 0, diagonal


def ungapped_alignment(q, t, d16, mat):
    """computeUngappedAlignment: the default LocalAlignment (score 0, diagonalLen 0, diagonal 0) unless a wrap scores strictly more"""
    best = (0, 0, 0)
    for d in range(1, 1 + len(t) // 32768 + 1):
        r = _by_diagonal(q, t, -d * 65536 + d16, mat)
        if r[0] > best[0]:
            best = r
    for d in range(0, len(q) // 65536 + 1):
        r = _by_diagonal(q, t, d * 65536 + d16, mat)
        if r[0] > best[0]:
            best = r
    return best


def rescore_subst(seqs, nucl, pref, pref_dbtype, par, db_residues=None):
    """seqs: key -> sequence bytes (one DB is query and target); pref: [(query key, entry bytes)] -> ([(query key, entry bytes)] as the
    reference writes them, [record dicts in the same order]).  par["thr"] is None: --filter-hits 0."""
    if par["rescore_mode"] != 1:
        raise ValueError("the substitution score is --rescore-mode 1")
    lib = lc.oracle_lib()
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

    out, records = [], []
    for qkey, entry in pref:
        text = b""
        lines = [l for l in entry.split(b"\n") if l.strip(b"\0")]
        if lines:
            q = seq(qkey)
            L = len(q)
            rev = hc.reverse_strand(q) if reverse_capable else None
        for line in lines:
            w = line.split()
            tkey, pref_score, d16 = int(w[0]), int(w[1]), int(w[2]) & 0xFFFF
            is_reverse = reverse_capable and pref_score < 0
            t = seq(tkey)
            db_len = len(t)
            is_identity = qkey == tkey
            if not hc._can_be_covered(cov_thr, par["cov_mode"], F32(L), F32(db_len)):
                continue
            score, diag_len, diagonal = ungapped_alignment(rev if is_reverse else q, t, d16, mat)
            evalue = lib.oracle_evalue(1 if nucl else 0, db_residues, float(score), float(L))
            bit_score = int(lib.oracle_bitscore(1 if nucl else 0, float(score)) + 0.5)
            seq_id, aln_len = 0.0, 0                                      # mode 1 computes neither
            with np.errstate(divide="ignore", invalid="ignore"):
                target_cov, query_cov = F32(diag_len) / F32(db_len), F32(diag_len) / F32(L)
                per_col = F32(score) / F32(diag_len)
            has_cov = hc._has_coverage(cov_thr, par["cov_mode"], query_cov, target_cov)
            has_seq_id = bool(seq_id >= float(seq_id_thr - FLT_EPSILON))
            has_evalue = evalue <= par["e"]
            has_aln_len = aln_len >= par["min_aln_len"]
            has_to_filter = par["thr"] is not None and bool(per_col >= F32(par["thr"]))
            if is_identity or has_to_filter or (has_aln_len and has_cov and has_seq_id and has_evalue):
                d = diagonal & 0xFFFF                                     # hit_t keeps an unsigned short, prefilterHitToBuffer prints a short
                text += b"%d\t%d\t%d\n" % (tkey, -bit_score if is_reverse else bit_score, (d ^ 0x8000) - 0x8000)
                records.append(dict(query=qkey, target=tkey, bit_score=bit_score, raw_score=score, diag_len=diag_len, diagonal=diagonal, per_col=per_col,
                                    evalue=evalue, reversed=int(is_reverse), by_filter=has_to_filter, by_gates=has_aln_len and has_cov and has_seq_id and has_evalue,
                                    identity=is_identity))
        out.append((qkey, text))
    return out, records


def repseqs(seqs, clusters):
    """result2repseq: seqs: key -> entry bytes without the NUL ("SEQ\\n"); clusters: [(key, entry bytes)] -> {key: entry bytes with the NUL}:
    the sequence of the first key on the entry's list under the entry's key; an empty entry gives none"""
    out = {}
    for key, entry in clusters:
        lines = [l for l in entry.split(b"\n") if l.strip(b"\0")]
        if lines:
            out[key] = seqs[int(lines[0].split()[0])] + b"\0"
    return out
