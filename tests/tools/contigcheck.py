"""numpy restatement of the workflows' tail: which contigs are reported and how the FASTA file looks.  The checker the GPU's
plasship_select_contigs / plasship_fasta_write are compared with; tests/test_contigcheck.py pins it to the reference's own FASTA files
(tests/golden/fasta_tail_*.tar.gz, made by tests/golden/make_fasta_tail.sh).

Selection ("entry length" = the index length: sequence + "\\n\\0"; ranks are data-file order, which is key order in the canonical layout):
  protein     data/assemble.sh:170-182 (--filter-proteins 0).  S1 = keys in RESULT and SOURCE whose RESULT entry length is larger (:173-174,
              `$3 > $6`); S2 = keys k of RESULT such that the entry on data-file line k of RESULT matches /^\\x00?\\*[A-Z]*\\*$/ (:176: the rank
              of one entry is compared with the key of another); the subset is S1 | S2 (:178, sort | uniq).
  nucleotide  data/nuclassemble.sh:151-167.  contig-output-mode 1: keys in RESULT and SOURCE whose RESULT entry length is larger; mode 0:
              every key; then entry length > min_contig_len + 1.
FASTA (src/util/createhdb.cpp:45-58, lib/mmseqs/src/util/convert2fasta.cpp:41-56): per selected entry in key order
  ">" <rank in the subset> " len:" <sequence length> [" cycle:" <0|1>] "\\n" <sequence> "\\n"
with the cycle field when a cycle DB exists (nuclassemble.sh:173-189); 1 for the keys in it.

    python tests/tools/contigcheck.py --assert-fixture DIR     (generation time: the fixture's non-vacuity conditions)
"""
import hashlib
import os
import sys

import numpy as np


class DB:
    """a DB's index (sorted by key) and, optionally, its data file"""

    def __init__(self, keys, off, elen, data=None):
        o = np.argsort(keys, kind="stable")
        self.keys = np.asarray(keys, dtype=np.int64)[o]
        self.off = np.asarray(off, dtype=np.int64)[o]
        self.elen = np.asarray(elen, dtype=np.int64)[o]
        self.data = data

    @property
    def n(self):
        return len(self.keys)

    def seq(self, i):
        o = int(self.off[i])
        return bytes(self.data[o:o + int(self.elen[i]) - 2])


def read_index(path):
    a = np.loadtxt(path, dtype=np.int64, ndmin=2) if os.path.getsize(path) else np.zeros((0, 3), dtype=np.int64)
    return a[:, 0], a[:, 1], a[:, 2]


def read_db(path, with_data=True):
    k, o, l = read_index(path + ".index")
    data = np.fromfile(path, dtype=np.uint8) if with_data else None
    return DB(k, o, l, data)


def index_db(path):
    k, o, l = read_index(path)
    return DB(k, o, l)


def _in_sorted(sorted_keys, q):
    if len(sorted_keys) == 0:
        return np.zeros(len(q), dtype=bool), np.zeros(len(q), dtype=np.int64)
    p = np.searchsorted(sorted_keys, q)
    pc = np.minimum(p, len(sorted_keys) - 1)
    return sorted_keys[pc] == q, pc


def _star_match(db, ids):
    """which of the entries `ids` match /^\\*[A-Z]*\\*$/"""
    ids = np.asarray(ids, dtype=np.int64)
    out = np.zeros(len(ids), dtype=bool)
    if len(ids) == 0:
        return out
    L = db.elen[ids] - 2
    first = db.data[db.off[ids]]
    last = db.data[db.off[ids] + np.maximum(L, 1) - 1]
    cand = np.nonzero((L >= 2) & (first == 0x2A) & (last == 0x2A))[0]
    for c in cand:
        o, n = int(db.off[ids[c]]), int(L[c])
        mid = db.data[o + 1:o + n - 1]
        out[c] = bool(np.all((mid >= 0x41) & (mid <= 0x5A)))
    return out


def select(mode, result, source, only_extended=True, min_contig_len=1000):
    """ids (key order) of the selected RESULT entries, and the protein sets {"s1", "s2"} as boolean arrays over RESULT's ids"""
    found, pos = _in_sorted(source.keys, result.keys)
    ext = found & (result.elen > np.where(found, source.elen[pos], 0))
    if mode == "protein":
        # data-file line k = the entry with the k-th smallest offset
        file_order = np.argsort(result.off, kind="stable")
        s2 = np.zeros(result.n, dtype=bool)
        has = result.keys < result.n
        s2[has] = _star_match(result, file_order[result.keys[has]])
        keep = ext | s2
        return np.nonzero(keep)[0], {"s1": ext, "s2": s2}
    keep = ext if only_extended else np.ones(result.n, dtype=bool)
    keep &= result.elen > min_contig_len + 1
    return np.nonzero(keep)[0], {}


def fasta_chunks(result, ids, cycle_keys=None, batch=1 << 16):
    """the FASTA file, in pieces of `batch` entries"""
    cyc = None
    if cycle_keys is not None:
        cyc, _ = _in_sorted(np.sort(np.asarray(cycle_keys, dtype=np.int64)), result.keys[ids])
    for b in range(0, len(ids), batch):
        parts = []
        for r in range(b, min(len(ids), b + batch)):
            i = int(ids[r])
            s = result.seq(i)
            h = b">%d len:%d" % (r, len(s))
            if cyc is not None:
                h += b" cycle:%d" % int(cyc[r])
            parts.append(h + b"\n" + s + b"\n")
        yield b"".join(parts)


def fasta(result, ids, cycle_keys=None):
    return b"".join(fasta_chunks(result, ids, cycle_keys))


def fasta_sha256(result, ids, cycle_keys=None):
    h, n = hashlib.sha256(), 0
    for c in fasta_chunks(result, ids, cycle_keys):
        h.update(c); n += len(c)
    return h.hexdigest(), n


def fixture_case(d):
    """(mode, flags, RESULT, SOURCE, cycle keys or None, reference FASTA bytes) of one case directory of fasta_tail.tar.gz"""
    mode = open(os.path.join(d, "mode")).read().strip()
    flags = open(os.path.join(d, "flags")).read().split()
    result = read_db(os.path.join(d, "result"))
    source = index_db(os.path.join(d, "source.index"))
    cp = os.path.join(d, "cycle.index")
    cyc = index_db(cp).keys if os.path.exists(cp) else None
    rp = os.path.join(d, "ref.fasta")
    if os.path.exists(rp):
        ref = open(rp, "rb").read()
    else:                               # a large FASTA is kept as "<sha256> <entries> <bytes>"
        h, ne, nb = open(rp + ".sha256").read().split()
        ref = (h, int(ne), int(nb))
    return mode, flags, result, source, cyc, ref


def matches(got, ref):
    """FASTA bytes `got` against a fixture's reference (bytes, or (sha256, entries, bytes))"""
    if isinstance(ref, bytes):
        return got == ref
    return (hashlib.sha256(got).hexdigest(), got.count(b"\n>") + (1 if got.startswith(b">") else 0), len(got)) == ref


def case_params(flags):
    """(only_extended, min_contig_len) of a nucleotide case's workflow flags (Nuclassembler.cpp defaults 1 / 1000)"""
    only, mn = True, 1000
    for i, a in enumerate(flags):
        if a == "--contig-output-mode":
            only = flags[i + 1] == "1"
        if a == "--min-contig-len":
            mn = int(flags[i + 1])
    return only, mn


def check_case(d):
    mode, flags, result, source, cyc, ref = fixture_case(d)
    only, mn = case_params(flags)
    ids, sets = select(mode, result, source, only, mn)
    got = fasta(result, ids, cyc)
    return matches(got, ref), mode, flags, result, source, cyc, ids, sets


def assert_fixture(root):
    cases = sorted(x for x in os.listdir(root) if x.startswith("case"))
    s2_only = 0
    for c in cases:
        ok, mode, flags, result, source, cyc, ids, sets = check_case(os.path.join(root, c))
        assert ok, "%s: the checker's FASTA differs from the reference's" % c
        assert len(ids) > 0, "%s selects nothing" % c
        if mode == "protein":
            s2_only += int(np.sum(sets["s2"] & ~sets["s1"]))
        print("%s: %d of %d entries selected" % (c, len(ids), result.n))
    assert s2_only > 0, "no key in S2 \\ S1 in the protein cases"
    _, _, result, source, cyc, _ = fixture_case(os.path.join(root, "case5"))
    ids, _ = select("nucleotide", result, source, True, 1000)
    assert b" cycle:1\n" in fasta(result, ids, cyc), "case5 has no circular contig"
    _, flags, result, source, cyc, _ = fixture_case(os.path.join(root, "case4"))
    ids0, _ = select("nucleotide", result, source, False, case_params(flags)[1])
    ids1, _ = select("nucleotide", result, source, True, case_params(flags)[1])
    assert len(ids0) > len(ids1), "case4: mode 1 would drop nothing"
    print("fixture ok: %d S2-only keys" % s2_only)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--assert-fixture":
        assert_fixture(sys.argv[2])
    else:
        sys.exit(__doc__)
