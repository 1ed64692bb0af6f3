"""Hand-made candidate lists with a PLANTED keep pattern, for compactCsr (plass_amd/csrc/scan.hip) through the public calls that end in it.

One nucleotide DB of N entries that are all either the 32-mer S (even index) or S' (odd index): S with every base substituted
(A -> C -> G -> T -> A), so that no position of S matches S'.  Every line of a prefilter DB names diagonal 0, so a line is kept iff query and
target are the same kind (32 of 32 columns equal), or it is the identity line:
  * `rescorediagonal --rescore-mode 0 --wrapped-scoring 0 --min-seq-id 1.0` (16-byte records): a pair of different kinds has no equal column,
    no alias scores, its sequence identity is 0 / 0; a kept line is written as "<target key>\t100\t0";
  * `rescorediagonal` with the default flags (64-byte records): a pair of different kinds scores -96 -> 0, which passes no E-value.
A case is (total lines, keep pattern, layout); the shapes stand around the scan's tile of 2048 flags (SCAN_TILE, device_utils.hpp).
Neither this file nor its host test (tests/test_csr_compact_host.py) needs a GPU.
"""
import functools

from rescore_ladder import DBTYPE_NUCL, DBTYPE_PREF, write_text_db

S = b"ACGTTGCAAGCTTCGATCAGGTCAACGTGTAC"
S_OTHER = S.translate(bytes.maketrans(b"ACGT", b"CGTA"))
assert len(S) == 32 and all(a != b for a, b in zip(S, S_OTHER))
N = 4200                      # entries; index i has key 3 i + 7 and kind i % 2
SCAN_TILE = 2048
TOTALS = (0, 1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1)
PATTERNS = ("all", "none", "alternating", "first", "last")
HAMMING_PAR = dict(rescore_mode=0, wrapped=0, min_seq_id=1.0, seq_id_mode=0, cov_mode=0, c=0.0, min_aln_len=0, e=1e-3)      # the module's defaults but --min-seq-id


def key(i):
    return 3 * i + 7


def write_seqdb(path):
    from plass_amd.synth import write_db
    path = str(path)
    write_db(path, b"".join((S_OTHER if i % 2 else S) + b"\n\0" for i in range(N)), [34 * i for i in range(N)], [34] * N, [key(i) for i in range(N)], DBTYPE_NUCL)
    return path


def seqs():
    return {key(i): (S_OTHER if i % 2 else S) for i in range(N)}


def keep_pattern(name, total):
    return [{"all": True, "none": False, "alternating": j % 2 == 0, "first": j == 0, "last": j == total - 1}[name] for j in range(total)]


def layout(name, total):
    """[(query index, lines)] in query order.  spread: every 80th query from 5 on holds 1, 3, 64, 65, 2, 130, 17, ... lines, so queries without
    lines stand at the front, between any two holders and at the end of the DB; single: query 2100 holds them all"""
    if name == "single":
        return [(2100, total)] if total else []
    out, q, k = [], 5, 0
    while total:
        n = min(total, (1, 3, 64, 65, 2, 130, 17)[k % 7])
        out.append((q, n)); total -= n; q += 80; k += 1
    assert q - 80 < N - 5
    return out


@functools.lru_cache(maxsize=None)
def case(lay, total, pattern):
    """-> ({query key: prefilter entry}, {query key: [target keys of the kept lines, in input order]}) with an entry for every query"""
    keep = keep_pattern(pattern, total)
    pref = {key(i): b"\0" for i in range(N)}
    kept = {key(i): [] for i in range(N)}
    at = 0
    for q, n in layout(lay, total):
        text, identity_used = b"", False
        for j in range(n):
            if keep[at] and not identity_used:
                t, identity_used = q, True                                   # the query's first kept line is its identity line
            else:
                t = (q + 2 * (j + 1) if keep[at] else q + 2 * j + 1) % N     # same kind / the other kind; distinct within the query (n < N / 2)
            text += b"%d\t%d\t0\n" % (key(t), 1 + at % 97)
            if keep[at]:
                kept[key(q)].append(key(t))
            at += 1
        pref[key(q)] = text + b"\0"
    assert at == total and sum(len(v) for v in kept.values()) == sum(keep)
    return pref, kept


def _cases():
    seen, out = set(), []
    for lay, totals in (("spread", TOTALS), ("single", (SCAN_TILE + 1,))):
        for total in totals:
            for pattern in PATTERNS:
                k = (lay, tuple(keep_pattern(pattern, total)))
                if k not in seen:                                             # (0 lines: one case; 1 line: kept or not)
                    seen.add(k); out.append((lay, total, pattern))
    return out


CASES = _cases()
CASE_IDS = ["%s-%d-%s" % c for c in CASES]


def write_pref(path, pref):
    return write_text_db(path, pref, DBTYPE_PREF)


def first_columns(entry):
    return [int(l.split(b"\t")[0]) for l in entry.rstrip(b"\0").split(b"\n") if l]
