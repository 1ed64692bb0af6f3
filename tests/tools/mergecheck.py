"""Numpy restatement of the reference's `mergereads` (src/assembler/mergereads.cpp:15-129 over FLASH, lib/flash/combine_reads.cpp), the
checker of plasship_mergereads.  Written from the semantics, offset by offset and vectorised over pairs:

  mate 2 is reverse-complemented (lib/flash/read.cpp: IUPAC and lowercase complemented, U -> A, every other byte '.', quality reversed);
  pair_align (combine_reads.cpp:266-336) with min_overlap 15, max_overlap 65, max_mismatch_density 0.10f, no outies: for every offset
  i = max(0, L1-L2) .. L1-15 the overlap S1[i:] / S2[:L1-i]; positions where either base is 'N' are skipped and shorten the overlap
  when either whole read holds an 'N' (without one no position is 'N', so skipping them always is the same thing); mismatches and the
  sum of min(quality) over them; a candidate needs an overlap of >= 15 after the shortening; score_len = float(min(len, 65)); both
  ratios are float32 divisions of the counts; the sequential update rule keeps the lexicographic minimum of (density, qual, offset);
  rejected when best density > 0.10f;
  generate_combined_read (:338-470): agreeing bases copied, otherwise the higher quality wins, on equal quality mate 2 unless it is 'N'.
Quality bytes are compared as they are in the file (no offset); inputs with bytes >= 128 are refused by the product and not modelled.
"""
import gzip

import numpy as np

MIN_OVERLAP, MAX_OVERLAP, MAX_DENSITY = 15, 65, np.float32(0.10)

_COMP = bytearray(b"." * 256)
for a, b in zip(b"ACGTUNSWRYKMBDHV", b"TGCAANSWYRMKVHDB"):
    _COMP[a] = b
    _COMP[a + 32] = b + 32          # lowercase
COMP = np.frombuffer(bytes(_COMP), dtype=np.uint8)


def revcomp(seq):
    return bytes(COMP[np.frombuffer(seq, dtype=np.uint8)[::-1]]) if seq else b""


def parse_fastq(data):
    """strict four-line FASTQ (what the product accepts) -> list of (name, seq, qual); '\\r' before a line end is dropped like kseq.h:145"""
    if data.endswith(b"\n"):
        data = data[:-1]
    lines = data.split(b"\n") if data else []
    assert len(lines) % 4 == 0, "not four-line FASTQ"
    out = []
    for r in range(0, len(lines), 4):
        h, s, p, q = lines[r:r + 4]
        s = s[:-1] if len(s) > 1 and s.endswith(b"\r") else s
        q = q[:-1] if len(q) > 1 and q.endswith(b"\r") else q
        assert h[:1] == b"@" and p[:1] == b"+" and len(s) == len(q) and s
        name = h[1:]
        for i, c in enumerate(name):
            if c in b" \t\n\v\f\r":
                name = name[:i]
                break
        out.append((name, s, q))
    return out


def read_fastq(path):
    with (gzip.open(path, "rb") if str(path).endswith(".gz") else open(path, "rb")) as f:
        return parse_fastq(f.read())


def _pad(strs, width):
    m = np.zeros((len(strs), width), dtype=np.uint8)
    for k, s in enumerate(strs):
        m[k, :len(s)] = np.frombuffer(s, dtype=np.uint8)
    return m


def align_pairs(s1, q1, s2, q2, trace=None):
    """s2 / q2 already reverse-complemented / reversed.  -> (best offset or -1 per pair).  `trace`: a list that receives one dict per pair
    with pair_align's intermediate values: l1, l2, off = {offset: (overlap after the uncalled positions, mismatches, quality sum, density,
    quality score)} for every offset scanned (the last two None where the overlap is no candidate), and bd, bq, bp = the best density,
    its quality score and its offset BEFORE the threshold (1.1, 0, -1 where no offset is a candidate)"""
    n = len(s1)
    L1 = np.array([len(s) for s in s1], dtype=np.int64)
    L2 = np.array([len(s) for s in s2], dtype=np.int64)
    best = np.full(n, -1, dtype=np.int64)
    if trace is not None:
        trace[:] = [{"l1": int(L1[k]), "l2": int(L2[k]), "off": {}, "bd": np.float32(1.1), "bq": np.float32(0), "bp": -1} for k in range(n)]
    order = np.argsort(L1, kind="stable")
    CH = 2048
    for c0 in range(0, n, CH):
        idx = order[c0:c0 + CH]
        l1, l2 = L1[idx], L2[idx]
        M1 = int(l1.max())
        if M1 < MIN_OVERLAP:
            continue
        W2 = max(M1, int(l2.max()))
        A, QA = _pad([s1[k] for k in idx], M1), _pad([q1[k] for k in idx], M1)
        B, QB = _pad([s2[k] for k in idx], W2), _pad([q2[k] for k in idx], W2)
        start = np.maximum(0, l1 - l2)
        bd = np.full(len(idx), np.float32(1.1), dtype=np.float32)
        bq = np.zeros(len(idx), dtype=np.float32)
        bp = np.full(len(idx), -1, dtype=np.int64)
        for i in range(0, M1 - MIN_OVERLAP + 1):
            act = (i >= start) & (i <= l1 - MIN_OVERLAP)
            if not act.any():
                continue
            sel = np.nonzero(act)[0]
            W = M1 - i
            a, b = A[sel, i:], B[sel, :W]
            ov = l1[sel] - i
            col = np.arange(W)[None, :] < ov[:, None]
            unc = ((a == 78) | (b == 78)) & col
            mis = (a != b) & col & ~unc
            cnt = mis.sum(1)
            qt = np.where(mis, np.minimum(QA[sel, i:], QB[sel, :W]).astype(np.int64), 0).sum(1)
            ln = ov - unc.sum(1)
            ok = ln >= MIN_OVERLAP
            sl = np.minimum(ln, MAX_OVERLAP).astype(np.float32)
            sl[~ok] = 1
            q = qt.astype(np.float32) / sl
            d = cnt.astype(np.float32) / sl
            if trace is not None:
                for j, k in enumerate(idx[sel]):
                    trace[k]["off"][i] = (int(ln[j]), int(cnt[j]), int(qt[j]), d[j] if ok[j] else None, q[j] if ok[j] else None)
            better = ok & ((d < bd[sel]) | ((d == bd[sel]) & (q < bq[sel])))
            s = sel[better]
            bd[s], bq[s], bp[s] = d[better], q[better], i
        if trace is not None:
            for j, k in enumerate(idx):
                trace[k].update(bd=bd[j], bq=bq[j], bp=int(bp[j]))
        bp[bd > MAX_DENSITY] = -1
        best[idx] = bp
    return best


def combine(s1, q1, s2, q2, pos):
    a, b = np.frombuffer(s1, dtype=np.uint8), np.frombuffer(s2, dtype=np.uint8)
    qa, qb = np.frombuffer(q1, dtype=np.uint8), np.frombuffer(q2, dtype=np.uint8)
    ov = len(a) - pos
    x, y, qx, qy = a[pos:], b[:ov], qa[pos:], qb[:ov]
    mid = np.where(x == y, x, np.where(qx > qy, x, np.where(qx < qy, y, np.where(y == 78, x, y))))
    return bytes(a[:pos]) + bytes(mid.astype(np.uint8)) + bytes(b[ov:])


def merge_records(r1, r2, trace=None):
    """two lists of (name, seq, qual) -> (sequence entries, header entries, n_combined); entries without the '\\0'.  `trace`: see align_pairs"""
    n = min(len(r1), len(r2))
    s1 = [r1[k][1] for k in range(n)]; q1 = [r1[k][2] for k in range(n)]
    s2 = [revcomp(r2[k][1]) for k in range(n)]; q2 = [r2[k][2][::-1] for k in range(n)]
    pos = align_pairs(s1, q1, s2, q2, trace)
    seqs, hdrs = [], []
    for k in range(n):
        if pos[k] >= 0:
            seqs.append(combine(s1[k], q1[k], s2[k], q2[k], int(pos[k])) + b"\n"); hdrs.append(r1[k][0] + b"\n")
        else:
            seqs += [s1[k] + b"\n", s2[k] + b"\n"]; hdrs += [r1[k][0] + b"\n", r2[k][0] + b"\n"]
    return seqs, hdrs, int((pos >= 0).sum())


def merge_files(paths):
    """`mergereads r1 r2 [r1b r2b ...]`: file pairs in sequence, keys continuing -> (sequence entries, header entries)"""
    seqs, hdrs = [], []
    for k in range(0, len(paths), 2):
        s, h, _ = merge_records(read_fastq(paths[k]), read_fastq(paths[k + 1]))
        seqs += s; hdrs += h
    return seqs, hdrs
