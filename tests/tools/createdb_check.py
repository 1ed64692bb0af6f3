#!/usr/bin/env python3
"""Plain-Python restatement of the reference's createdb on read files (lib/mmseqs/src/util/createdb.cpp:15-333 over kseq,
lib/mmseqs/lib/ksw2/kseq.h:96-233): what tests/test_gpu_createdb.py compares the device parser with on inputs it generates itself.
tests/test_createdb_host.py pins this file against the files the unmodified reference wrote (tests/golden/createdb.tar.gz).

    kseq_records(data)  the entries kseq_read returns: (name, comment, sequence) — a byte-level port of the macro, so that every corner
                        ('\\r' handling, blank lines, a last line without '\\n', multi-line FASTQ) is the reference's
    createdb(files, shuffle, id_offset) -> {suffix: bytes} for "", ".index", ".dbtype", "_h", "_h.index", "_h.dbtype", ".lookup", ".source"
"""
import gzip
import os
import struct

SPACE = b" \t\n\v\f\r"


class _Stream:
    def __init__(self, data):
        self.d, self.p = data, 0

    def getc(self):
        if self.p >= len(self.d):
            return -1
        c = self.d[self.p]; self.p += 1
        return c

    def getuntil(self, sep_line, buf):
        """ks_getuntil2: appends to buf up to the delimiter (a line end, or any isspace byte), returns (delimiter or -1, gotany)"""
        d, n = self.d, len(self.d)
        if self.p >= n:
            return -1, False
        i = self.p
        if sep_line:
            j = d.find(b"\n", i)
            j = n if j < 0 else j
        else:
            j = i
            while j < n and d[j] not in SPACE:
                j += 1
        buf += d[i:j]
        self.p = min(j + 1, n)
        dret = d[j] if j < n else -1
        if sep_line and len(buf) > 1 and buf[-1] == 13:       # kseq.h:145
            del buf[-1]
        return dret, True


def kseq_records(data):
    ks = _Stream(bytes(data)); last = 0; out = []
    while True:
        if last == 0:
            while True:
                c = ks.getc()
                if c < 0 or c in b">@":
                    break
            if c < 0:
                return out
            last = c
        name, comment, seq, qual = bytearray(), bytearray(), bytearray(), bytearray()
        c, got = ks.getuntil(False, name)
        if not got:
            return out
        if c != 10:
            ks.getuntil(True, comment)
        while True:
            c = ks.getc()
            if c < 0 or c in b">+@":
                break
            if c == 10:
                continue
            seq.append(c)
            ks.getuntil(True, seq)
        if c >= 0 and c in b">@":
            last = c
        if c != 43:
            out.append((bytes(name), bytes(comment), bytes(seq)))
            if c < 0:
                return out
            continue
        while True:
            c = ks.getc()
            if c < 0 or c == 10:
                break
        if c < 0:
            return out                                       # -2: no quality string; ReadEntry ends the file
        while True:
            _, got = ks.getuntil(True, qual)
            if not got or len(qual) >= len(seq):
                break
        last = 0
        if len(seq) != len(qual):
            return out                                       # -2: createdb stops reading this file
        out.append((bytes(name), bytes(comment), bytes(seq)))


def read_file(path):
    with open(path, "rb") as f:
        raw = f.read()
    return gzip.decompress(raw) if str(path).endswith(".gz") else raw


def shuffle_keys(n, shuffle=True, id_offset=0):
    """position in the data file (= key after createRenumberedDB) of input entry i: split (id_offset + i) % 32, splits concatenated"""
    if not shuffle:
        return list(range(n))
    splits = [[] for _ in range(32)]
    for i in range(n):
        splits[(id_offset + i) % 32].append(i)
    pos = [0] * n; k = 0
    for s in splits:
        for i in s:
            pos[i] = k; k += 1
    return pos


_PREFIXES = [("uc", 2, 0), ("cl|", 3, 1), ("sp|", 3, 1), ("tr|", 3, 1), ("gb|", 3, 1), ("ref|", 4, 1), ("pdb|", 4, 1), ("bbs|", 4, 1), ("lcl|", 4, 1),
             ("pir||", 5, 1), ("prf||", 5, 1), ("gnl|", 4, 2), ("pat|", 4, 2), ("gi|", 3, 3)]


def lookup_name(word):
    """Util::parseFastaHeader (Util.cpp:173-256) on the header's first word"""
    if not word:
        return b""
    off = 10 if word.startswith(b"consensus_") else 0
    for pre, ln, bar in _PREFIXES:
        if word[off:].startswith(pre.encode()):
            start = off + ln
            for _ in range(max(bar - 1, 0)):
                e = word.find(b"|", start)
                if e < 0:
                    return b""
                start = e + 1
            e = word.find(b"|", start)
            if e < 0:
                e = len(word)
            return word[start:e]
    return word[off:]


def is_nucleotide(records):
    """createdb.cpp:171-200: only the first ten entries are ever sampled (sampleCount stops at 10)"""
    import numpy as np
    for _, _, s in records[:10]:
        cnt = sum(1 for b in s.upper() if b in b"TAGCUN")
        if not len(s) or not (float(np.float32(cnt) / np.float32(len(s))) > 0.9):
            return False
    return True


def createdb(files, shuffle=True, id_offset=0):
    recs, fileno = [], []
    for fi, p in enumerate(files):
        r = kseq_records(read_file(p))
        recs += r; fileno += [fi] * len(r)
    n = len(recs)
    pos = shuffle_keys(n, shuffle, id_offset)
    order = [0] * n
    for i, k in enumerate(pos):
        order[k] = i
    data, hdr, idx, hidx, lookup = bytearray(), bytearray(), bytearray(), bytearray(), bytearray()
    for k, i in enumerate(order):
        name, comment, seq = recs[i]
        h = name + (b" " + comment if comment else b"") + b"\n\0"
        e = seq + b"\n\0"
        key = k if shuffle else id_offset + i
        idx += b"%d\t%d\t%d\n" % (key, len(data), len(e)); hidx += b"%d\t%d\t%d\n" % (key, len(hdr), len(h))
        data += e; hdr += h
        lookup += b"%d\t%s\t%d\n" % (k, lookup_name(name), fileno[i])          # (the header's first word is kseq's name)
    source = b"".join(b"%d\t%s\n" % (fi, os.path.basename(str(p)).encode()) for fi, p in enumerate(files))
    dbtype = 1 if is_nucleotide(recs) else 0
    return {"": bytes(data), ".index": bytes(idx), ".dbtype": struct.pack("<i", dbtype), "_h": bytes(hdr), "_h.index": bytes(hidx),
            "_h.dbtype": struct.pack("<i", 12), ".lookup": bytes(lookup), ".source": source}


SUFFIXES = ["", ".index", ".dbtype", "_h", "_h.index", "_h.dbtype", ".lookup", ".source"]


def read_db(prefix):
    out = {}
    for s in SUFFIXES:
        with open(str(prefix) + s, "rb") as f:
            out[s] = f.read()
    return out
