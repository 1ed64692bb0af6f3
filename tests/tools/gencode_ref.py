"""A short sequential restatement of extractorfs and translatenucs for any genetic code (--translation-table, --use-all-table-starts), written
from the reference's rules (mm/commons/Orf.cpp:55-91,127-159,228-348; mm/commons/TranslateNucl.h:110-246,334-503; mm/util/extractorfs.cpp:67-125;
mm/util/translatenucs.cpp:48-103).  tests/test_gencode_host.py pins it on the DBs the unmodified reference wrote (tests/golden/gencode.tar.gz); the GPU
tests then use it on generated reads.  DBs are lists of (key, bytes of the sequence without "\\n\\0")."""

# NCBI gc.prt: residues and start / stop flags of the 64 codons in T, C, A, G order
TABLES = {
    1: ("FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG", "---M------**--*----M---------------M----------------------------"),
    2: ("FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNKKSS**VVVVAAAADDEEGGGG", "----------**--------------------MMMM----------**---M------------"),
    3: ("FFLLSSSSYY**CCWWTTTTPPPPHHQQRRRRIIMMTTTTNNKKSSRRVVVVAAAADDEEGGGG", "----------**----------------------MM----------------------------"),
    4: ("FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG", "--MM------**-------M------------MMMM---------------M------------"),
    5: ("FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNKKSSSSVVVVAAAADDEEGGGG", "---M------**--------------------MMMM---------------M------------"),
    6: ("FFLLSSSSYYQQCC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG", "--------------*--------------------M----------------------------"),
    9: ("FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNNKSSSSVVVVAAAADDEEGGGG", "----------**-----------------------M---------------M------------"),
    10: ("FFLLSSSSYY**CCCWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG", "----------**-----------------------M----------------------------"),
    11: ("FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG", "---M------**--*----M------------MMMM---------------M------------"),
    12: ("FFLLSSSSYY**CC*WLLLSPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG", "----------**--*----M---------------M----------------------------"),
    13: ("FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNKKSSGGVVVVAAAADDEEGGGG", "---M------**----------------------MM---------------M------------"),
    14: ("FFLLSSSSYYY*CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNNKSSSSVVVVAAAADDEEGGGG", "-----------*-----------------------M----------------------------"),
    15: ("FFLLSSSSYY*QCC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG", "----------*---*--------------------M----------------------------"),
    16: ("FFLLSSSSYY*LCC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG", "----------*---*--------------------M----------------------------"),
    21: ("FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNNKSSSSVVVVAAAADDEEGGGG", "----------**-----------------------M---------------M------------"),
    22: ("FFLLSS*SYY*LCC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG", "------*---*---*--------------------M----------------------------"),
    23: ("FF*LSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG", "--*-------**--*-----------------M--M---------------M------------"),
    24: ("FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSSKVVVVAAAADDEEGGGG", "---M------**-------M---------------M---------------M------------"),
    25: ("FFLLSSSSYY**CCGWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG", "---M------**-----------------------M---------------M------------"),
    26: ("FFLLSSSSYY**CC*WLLLAPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG", "----------**--*----M---------------M----------------------------"),
    27: ("FFLLSSSSYYQQCCWWLLLAPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG", "--------------*--------------------M----------------------------"),
    28: ("FFLLSSSSYYQQCCWWLLLAPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG", "----------**--*--------------------M----------------------------"),
    29: ("FFLLSSSSYYYYCC*WLLLAPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG", "--------------*--------------------M----------------------------"),
    30: ("FFLLSSSSYYEECC*WLLLAPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG", "--------------*--------------------M----------------------------"),
    31: ("FFLLSSSSYYEECCWWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG", "----------**-----------------------M----------------------------"),
}
VALID = sorted(TABLES)
INVALID = (0, 7, 17, 32)
TCAG = "TCAG"
CHAR_MAX = 127


def codons(table, use_all_table_starts):
    """(stop codons, start codons) of the ORF scan, as upper-case strings.  The reference collects the stops while it fills its residue table
    (TranslateNucl.h:429-436), so they are the '*' of the RESIDUE string; the starts are the 'M' of the start / stop string, or ATG alone"""
    res, sta = TABLES[table]
    name = [a + b + c for a in TCAG for b in TCAG for c in TCAG]
    stops = {name[i] for i in range(64) if res[i] == "*"}
    starts = {name[i] for i in range(64) if sta[i] == "M"} if use_all_table_starts else {"ATG"}
    return stops, starts


# ---- translation: ncbi4na base codes, ambiguity letters expanded (TranslateNucl.h:334-486) ----
def _base_codes():
    t = [0] * 256
    for i, ch in enumerate("-ACMGRSVTWYHKDBN"):
        t[ord(ch)] = i
        t[ord(ch.lower())] = i
    for ch in "Uu":
        t[ord(ch)] = 8
    for ch in "Xx":
        t[ord(ch)] = 15
    for i in range(16):
        t[i] = i
    return t


BASE = _base_codes()
_IDX = {1: 2, 2: 1, 4: 3, 8: 0}       # A, C, G, T -> position in T, C, A, G
_LUT = {}


def residue_lut(table):
    if table in _LUT:
        return _LUT[table]
    res = TABLES[table][0]
    lut = []
    for i in range(16):
        for j in range(16):
            for k in range(16):
                aa = None
                for x in (1, 2, 4, 8):
                    for y in (1, 2, 4, 8):
                        for z in (1, 2, 4, 8):
                            if not (x & i and y & j and z & k):
                                continue
                            ch = res[16 * _IDX[x] + 4 * _IDX[y] + _IDX[z]]
                            if aa is None:
                                aa = ch
                            elif aa != ch:
                                if aa in "BDN" and ch in "DN":
                                    aa = "B"
                                elif aa in "ZEQ" and ch in "EQ":
                                    aa = "Z"
                                elif aa in "JIL" and ch in "IL":
                                    aa = "J"
                                else:
                                    aa = "X"
                lut.append(ord(aa or "X"))
    _LUT[table] = lut
    return lut


def translate(table, nucl, length):
    """TranslateNucl::translate on the first `length` bytes: length // 3 residues (the caller overwrites what a ragged end adds)"""
    lut = residue_lut(table)
    out = bytearray()
    for i in range(0, length - length % 3, 3):
        c = nucl[i:i + 3]
        r = lut[(BASE[c[0]] << 8) | (BASE[c[1]] << 4) | BASE[c[2]]]
        if any(97 <= b <= 122 for b in c) and 65 <= r <= 90:
            r += 32
        out.append(r)
    return bytes(out)


# ---- the ORF scan ----
_COMP = dict(zip(b"ABCDGHKMNRSTUVWY", b"TVGHCDMKNYSAABWR"))


def _complement(b):
    lower = 97 <= b <= 122
    r = _COMP.get(b - 32 if lower else b)
    if r is None:
        return ord("N")                  # '.' of the table, which setSequence turns into 'N'
    return r + 32 if lower else r


def _is_gap(b):                          # isGapOrN on an upper-cased letter (CHAR_MAX included)
    return b == ord("N") or (b - 32 if 97 <= b <= 122 else b) not in _COMP


def strands(seq):
    """Orf::setSequence: 'u' -> 't' only (the 'U' line is overwritten), the reverse complement, unknown letters -> 'N'"""
    fwd = bytes(ord("t") if b == ord("u") else b for b in seq)
    return fwd, bytes(_complement(b) for b in reversed(fwd))


def find_forward(s, stops, starts, min_length, max_length, max_gaps, frames, start_mode, _cache={}):
    """Orf::findForward on one strand: [(from, to, incomplete start, incomplete end)].  Behind the sequence lies CHAR_MAX: a codon that reaches it is
    incomplete, and a complete codon whose successor is incomplete is the last of its frame"""
    L = len(s)
    up = bytes(b & 0xDF for b in s).decode("latin-1") + chr(CHAR_MAX) * 8
    known = _cache.setdefault((frozenset(stops), frozenset(starts)), {})
    inside, has_start, gaps, length, frm = [True] * 3, [False] * 3, [0] * 3, [0] * 3, [0, 1, 2]
    out = []
    for position in range(3 * (L // 3)):
        f = position % 3
        if not frames & (1 << f):
            continue
        word = up[position:position + 3]
        what = known.get(word)
        if what is None:
            what = known[word] = (word in starts, word in stops, any(_is_gap(ord(c)) for c in word))
        is_start, stop, gap = what
        last = position + 3 <= L < position + 6
        should = (not inside[f] and is_start) if start_mode == 0 else (not inside[f]) if start_mode == 1 else is_start
        if should:
            inside[f], has_start[f], frm[f], gaps[f], length[f] = True, True, position, 0, 0
        if inside[f]:
            if not stop:
                length[f] += 1
            if gap:
                gaps[f] += 1
            if stop or last:
                inside[f] = False
                if length[f] == 0 and stop:
                    continue
                to = position + 2 if (last and not stop) else position - 1
                if gaps[f] > max_gaps or length[f] > max_length or length[f] < min_length:
                    continue
                out.append((frm[f], to, not has_start[f], not stop))
    return out


DEFAULTS = dict(min_length=30, max_length=32734, max_gaps=2147483647, contig_start_mode=2, contig_end_mode=2, orf_start_mode=1, forward_frames=7,
                reverse_frames=7, translate=0, max_seq_len=65535)


def extractorfs(reads, table=1, use_all_table_starts=False, **kw):
    """reads: [(key, sequence bytes)] in index order -> (ORF entries, header entries), both [(new key, bytes with the final "\\n")]"""
    p = dict(DEFAULTS, **kw)
    stops, starts = codons(table, use_all_table_starts)
    orfs, hdrs = [], []
    for key, seq in reads:
        L = len(seq)
        if L < 3:
            continue
        data = bytes(seq) + b"\n\0" + bytes(8)
        for strand, (s, frames) in enumerate(zip(strands(seq), (p["forward_frames"], p["reverse_frames"]))):
            if not frames:
                continue
            for frm, to, inc_s, inc_e in find_forward(s, stops, starts, p["min_length"], p["max_length"], p["max_gaps"], frames, p["orf_start_mode"]):
                if (p["contig_start_mode"] < 2 and int(inc_s) == p["contig_start_mode"]) or (p["contig_end_mode"] < 2 and int(inc_e) == p["contig_end_mode"]):
                    continue
                n = to - frm + 1
                body = s[frm:frm + n]
                if p["translate"]:       # extractorfs.cpp:103-116 (the length test indexes the READ, as written there)
                    if (data[n] != 10 and n % 3 != 0) and (data[n - 1] == 10 and (n - 1) % 3 != 0):
                        n -= n % 3
                    if n < 3:
                        continue
                    n = min(n, 3 * p["max_seq_len"])
                    body = translate(table, s[frm:frm + n] + bytes(3), n)
                a, b = (L - 1 - frm, L - 1 - to) if strand else (frm, to)
                complete = int(inc_s) | int(inc_e) << 1      # Orf::writeOrfHeader
                hdrs.append((len(hdrs), ("%d\t%d%s%d%s\n" % (key, a, "+" if a < b else "-", abs(a - b), "\t%d" % complete if complete else "")).encode()))
                orfs.append((len(orfs), body + b"\n"))
    return orfs, hdrs


def parse_header(h):
    """Orf::parseOrfHeader of a header this module wrote -> (incomplete start, incomplete end)"""
    w = h.split()
    complete = int(w[2]) if len(w) == 3 else 0
    return bool(complete & 1), bool(complete & 2)


def translatenucs(orfs, hdrs, table=1, add_orf_stop=False, max_seq_len=65535):
    """orfs: [(key, entry bytes with the final "\\n")], hdrs: the header entries of the same keys -> [(key, bytes with the final "\\n")]"""
    hdr = dict(hdrs or [])
    out = []
    for key, entry in orfs:
        if not entry:
            continue
        data = entry + b"\0" + bytes(8)
        length = len(entry)              # the entry without its NUL: the "\n" counts (translatenucs.cpp:69)
        at_start = at_end = False
        if add_orf_stop:
            inc_s, inc_e = parse_header(hdr[key])
            at_start, at_end = not inc_s, not inc_e
        if (data[length] != 10 and length % 3 != 0) and (data[length - 1] == 10 and (length - 1) % 3 != 0):
            length -= length % 3
        if length < 3:
            continue
        length = min(length, 3 * max_seq_len)
        aa = translate(table, data, length)
        if at_end and aa[-1:] == b"*":
            at_end = False
        out.append((key, (b"*" if at_start else b"") + aa + (b"*" if at_end else b"") + b"\n"))
    return out


def concat(a, b):
    """concatdbs: A's entries with their keys, then B's numbered from max(keyA) + 1 on"""
    base = max((k for k, _ in a), default=-1) + 1 if a else 1
    return list(a) + [(base + i, e) for i, (_, e) in enumerate(b)]


# ---- DB files ----
def db_files(entries):
    """(data file bytes, index file bytes) of a DB whose entries lie in the given order"""
    data, index, off = bytearray(), [], 0
    for key, e in entries:
        data += e + b"\0"
        index.append("%d\t%d\t%d\n" % (key, off, len(e) + 1))
        off += len(e) + 1
    return bytes(data), "".join(index).encode()


def read_entries(path):
    """[(key, entry bytes without the NUL)] in index order"""
    data = open(path, "rb").read()
    out = []
    for line in open(path + ".index", "rb"):
        k, o, n = (int(x) for x in line.split()[:3])
        out.append((k, data[o:o + n - 1]))
    return out


def read_seqs(path):
    return [(k, e[:-1] if e.endswith(b"\n") else e) for k, e in read_entries(path)]
