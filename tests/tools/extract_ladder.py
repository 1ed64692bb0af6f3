"""Length ladders for kmermatcher's extraction tiers (tests/test_gpu_extract_ladder.py, tests/test_extract_ladder_host.py).

kmermatchImpl (plass_amd/csrc/kmermatch.hip) sends every sequence to a kernel by its window count nWin = L - k + 1, its length L and
consideredRaw = (size_t)((float)(kps - 1) + scale * (float)L); a sequence a kernel cannot hold is queued for the next one.  A ladder is
one random "genome" per alphabet, a few substrings ("rungs") of every length on and next to a hand-over edge, and short reads tiled
over the whole genome so that every rung has overlap partners.  The expectation is the CPU oracle's; nothing here needs a GPU.

Where the decisions are made (the edge lists below follow these lines):
  kmermatch_extract.hpp  SHORT_MAXL = 128; extractShortKernel / extractShortFastKernel hand a sequence to the wave kernels when
                         `L > SHORT_MAXL || nWin > consideredRaw`, the fast kernel also when `multi && nWin > 48`; both sort it into
                         the 4-scores list, the 16-scores list (`nw > longWindows`, 256) or the 48-scores queue (`nw > hugeWindows`,
                         1024); classifyWindowsKernel does the same by window count alone (nucleotide, protein k > 16)
  kmermatch_extract.hpp  extractKernel: `min(nWin, consideredRaw) > cap` and `nWin > 64 * REGS` (REGS 4 / 16 / 48 -> 256 / 1024 / 3072
                         windows) queue for the next tier; the register tiers stage 16 bytes per lane behind the first 256 (L + 31 > 256);
                         the three-pass tier keeps `L <= RES_L` (8160) resident in LDS and re-stages a longer sequence tile by tile in every
                         pass -- it hands on only a candidate set beyond its CAP (128 protein, 1024 nucleotide)
  kmermatch.hip          CAP = 128 (4- and 16-scores tiers), CAP48 = 512 nucleotide / 128 protein, CAP2 = 1024 / 128; the row kernels'
                         bins end at 96, 128 and 192 windows (binWaveListKernel); `allWork` (no nWin above kps - 1) picks the LDS-staged
                         thread-per-sequence kernel; plasship_kmermatch takes the 24-byte layout from an entry length (L + 2) of
                         SHRT_MAX, i.e. from L = 32765, and for nucleotide k > 23
"""
import functools
import os
import re

import numpy as np

AA_LETTERS = "ACDEFGHIKLMNPQRSTVWY"
NT_LETTERS = "ACGT"

SHORT_MAXL = 128            # kmermatch_extract.hpp: constexpr uint32_t SHORT_MAXL
MULTI_WINDOWS = 48          # extractShortFastKernel: multi && nWin > 48
TIER_WINDOWS = (256, 1024, 3072)        # 64 * REGS of the 4-, 16- and 48-scores tiers (kmermatch.hip: TIER0_WINDOWS, hugeWindows, <…, 48, 992>)
RES_L = 8160                # extractKernel<…, 0, 8160>: longest sequence resident in LDS
ROW_BINS = (96, 128, 192)   # binWaveListKernel(…, 96u, 128u, 192u, …)
STAGING = 992               # RESL of the register tiers (their LDS code buffer is max(RESL, 64 * REGS + 32) + 32 bytes)
LAYOUT_SWITCH_L = 32765     # entry length L + 2 == SHRT_MAX

# window counts on and next to an edge; every one is cut with d = -1, 0, +1, +2 windows more
WINDOW_EDGES_AA = [1, MULTI_WINDOWS, MULTI_WINDOWS + 1, 64, 65, ROW_BINS[0], ROW_BINS[0] + 1, ROW_BINS[1], ROW_BINS[1] + 1, ROW_BINS[2], ROW_BINS[2] + 1,
                   TIER_WINDOWS[0], TIER_WINDOWS[0] + 1, STAGING, TIER_WINDOWS[1], TIER_WINDOWS[1] + 1, TIER_WINDOWS[2], TIER_WINDOWS[2] + 1]
WINDOW_EDGES_NUCL = [e for e in WINDOW_EDGES_AA if e >= 64]
DELTAS = (-1, 0, 1, 2)
TOP_AA, TOP_NUCL = 9000, 12000


def caps(nucl):
    """candidate capacities a sequence meets on its way down the launch chain: (4-scores, 16-scores, 48-scores, three-pass)"""
    return (128, 128, 512, 1024) if nucl else (128, 128, 128, 128)


def considered_raw(L, kps, scale):
    """(size_t)((float)(kps - 1) + scale * (float)L) in single precision, as boundsKernel, the kernels and the oracle compute it"""
    L = np.asarray(L)
    return (np.float32(kps - 1) + np.float32(scale) * L.astype(np.float32)).astype(np.int64)


def windows(L, k):
    L = np.asarray(L, dtype=np.int64)
    return np.maximum(L - k + 1, 0)


CLASSES = ("short", "w256", "w1024", "w3072", "lds", "beyond")


def tier_class(L, k, kps, scale, nucl, multi=True, alph=13):
    """the hand-over class of a sequence: which kernel of the launch chain is the first that keeps it.  "short": the thread-per-sequence
    kernel; "w256" / "w1024" / "w3072": the register tiers; "lds": the three-pass tier with the sequence resident; "beyond": L > 8160 (the
    three-pass tier re-staging it, or the HBM-scratch launch when its candidate set exceeds the last CAP)"""
    nw = int(windows(L, k)); cr = int(considered_raw(L, kps, scale))
    if not nucl and k <= 16:
        fast = k == 14            # extractShortFastKernel (either instantiation); its extra hand-over
        if not (L > SHORT_MAXL or nw > cr or (fast and multi and nw > MULTI_WINDOWS)):
            return "short"
    if L > RES_L:
        return "beyond"
    c = caps(nucl)
    for i, w in enumerate(TIER_WINDOWS):
        if nw <= w and min(nw, cr) <= c[i]:
            return CLASSES[1 + i]
    return "lds"


def goes_to_scratch(L, k, kps, scale, nucl):
    """min(nWin, consideredRaw) above the last tier's CAP: no LDS tier can hold the candidate set"""
    return min(int(windows(L, k)), int(considered_raw(L, kps, scale))) > caps(nucl)[3]


def crossing_lengths(nucl, k, kps, scale, top):
    """lengths at which `nWin > consideredRaw` or `min(nWin, consideredRaw) > CAP` changes its value, each with its neighbours"""
    Ls = np.arange(max(k - 1, 1), top + 1)
    nw, cr = windows(Ls, k), considered_raw(Ls, kps, scale)
    out = set()
    preds = [nw > cr] + [np.minimum(nw, cr) > c for c in sorted(set(caps(nucl)))]
    for p in preds:
        for i in np.nonzero(p[1:] != p[:-1])[0]:
            L = int(Ls[i + 1])
            out.update((L - 2, L - 1, L, L + 1))
    return out


def ladder_lengths(nucl, k, kps, scale):
    top = TOP_NUCL if nucl else TOP_AA
    Ls = {k - 1, k, k + 1, top}
    edges = list(WINDOW_EDGES_NUCL) if nucl else WINDOW_EDGES_AA + [max(kps - 1, 1), max(kps, 1)]
    for e in edges:
        for d in DELTAS:
            Ls.add(e + k - 1 + d)
    if not nucl:
        Ls.update(range(SHORT_MAXL - 1, SHORT_MAXL + 3))
    Ls.update(range(RES_L - 1, RES_L + 3))
    Ls |= crossing_lengths(nucl, k, kps, scale, top)
    return sorted(L for L in Ls if 1 <= L <= top)


def _genome(nucl, n, seed):
    rng = np.random.default_rng(seed)
    letters = NT_LETTERS if nucl else AA_LETTERS
    return "".join(letters[i] for i in rng.integers(0, len(letters), n))


_COMP = str.maketrans("ACGT", "TGCA")


def _revcomp(s):
    return s.translate(_COMP)[::-1]


def _partners(genome, nucl, rng):
    """reads of 45-75 residues (150-250 nucleotides) tiled over the genome at about a third of their length; every other nucleotide read
    is of the reverse strand"""
    lo, hi = (150, 251) if nucl else (45, 76)
    out, p, i = [], 0, 0
    while p < len(genome):
        l = int(rng.integers(lo, hi))
        s = genome[p:p + l]
        if len(s) >= lo:
            out.append(_revcomp(s) if (nucl and i % 2) else s)
        p += max(1, l // 3); i += 1
    return out


class Ladder:
    """seqs[i], keys[i] in index-file order; is_rung[i]; lengths[i]"""

    def __init__(self, nucl, seqs, is_rung, rng):
        n = len(seqs)
        keys = np.cumsum(rng.integers(1, 4, size=n)).astype(np.uint32)         # sparse, non-contiguous
        perm = rng.permutation(n)                                                # index file order != key order
        self.nucl = nucl
        self.seqs = [seqs[i] for i in perm]
        self.keys = keys[perm]
        self.is_rung = np.asarray(is_rung, dtype=bool)[perm]
        self.lengths = np.array([len(s) for s in self.seqs], dtype=np.int64)

    def write(self, path):
        path = str(path)
        off = 0
        with open(path, "wb") as f, open(path + ".index", "wb") as ix:
            for s, k in zip(self.seqs, self.keys):
                e = s.encode() + b"\n\0"
                f.write(e); ix.write(b"%d\t%d\t%d\n" % (int(k), off, len(e))); off += len(e)
        with open(path + ".dbtype", "wb") as f:
            f.write(int(1 if self.nucl else 0).to_bytes(4, "little"))
        return path

    def length_of_key(self):
        return {int(k): int(l) for k, l in zip(self.keys, self.lengths)}


@functools.lru_cache(maxsize=None)
def ladder(nucl, k, kps, scale=None):
    """the main ladder of an alphabet for (k, kps, scale): the same genome and partner reads whatever the flags, rungs of the lengths
    that are edges under these flags.  Three rungs per length, five of every length beyond 8000 (so that the classes of the last two
    tiers hold more than ten sequences)."""
    if scale is None:
        scale = 0.1 if nucl else 0.0
    top = TOP_NUCL if nucl else TOP_AA
    genome = _genome(nucl, top + 400, 20260 + int(nucl))
    rng = np.random.default_rng(77 + int(nucl))
    seqs = _partners(genome, nucl, rng)
    is_rung = [False] * len(seqs)
    for L in ladder_lengths(nucl, k, kps, scale):
        for j in range(5 if L > 8000 else 3):
            p = int(rng.integers(0, len(genome) - L + 1))
            s = genome[p:p + L]
            seqs.append(_revcomp(s) if (nucl and j == 1) else s)
            is_rung.append(True)
    return Ladder(nucl, seqs, is_rung, rng)


@functools.lru_cache(maxsize=None)
def layout_switch_db(L):
    """a protein DB whose longest entries are one pair of rungs of L residues (the 16-byte layout up to L = 32764, the 24-byte one from
    32765), kept apart so that the main ladder stays in the short layout"""
    genome = _genome(False, 33000, 4242)
    rng = np.random.default_rng(L)
    seqs = _partners(genome, False, rng)
    is_rung = [False] * len(seqs)
    for p in (0, len(genome) - L):
        seqs.append(genome[p:p + L]); is_rung.append(True)
    return Ladder(False, seqs, is_rung, rng)


@functools.lru_cache(maxsize=None)
def all_work_dbs(k=14, kps=60):
    """(reads only, the same reads plus one rung of 300 residues, under the same keys): every read has nWin <= kps - 1, so the first DB
    takes the LDS-staged thread-per-sequence kernel and the second, whose rung must be queued, the unstaged one.  The rung is cut from
    ANOTHER random genome: a rung that shared k-mers with the reads would become their groups' representative (the longest member) and
    so change the lines the reads have among themselves by construction."""
    base = ladder(False, k, kps)
    reads = [(int(key), s) for key, s, r in zip(base.keys, base.seqs, base.is_rung) if not r and len(s) - k + 1 <= kps - 1]
    rung = _genome(False, 300, 99)
    a, b = Ladder.__new__(Ladder), Ladder.__new__(Ladder)
    for d, extra in ((a, []), (b, [(max(key for key, _ in reads) + 5, rung)])):
        rows = reads + extra
        d.nucl = False; d.seqs = [s for _, s in rows]; d.keys = np.array([key for key, _ in rows], dtype=np.uint32)
        d.is_rung = np.array([False] * len(reads) + [True] * len(extra)); d.lengths = np.array([len(s) for s in d.seqs], dtype=np.int64)
    return a, b


# ---- the cases: one kmermatcher call each ------------------------------------------------------------------------------------------
def _case(name, nucl=False, k=None, alph=None, kps=60, scale=None, multi=True, ext=None, hash_shift=67, c=0.0, cov_mode=0):
    return dict(name=name, nucl=nucl, k=k if k is not None else (22 if nucl else 14), alph=alph if alph is not None else (5 if nucl else 13), kps=kps,
                scale=scale if scale is not None else (0.1 if nucl else 0.0), multi=multi, ext=ext if ext is not None else nucl, hash_shift=hash_shift,
                c=c, cov_mode=cov_mode)


AA_CASES = [
    _case("default"),                                            # extractShortFastKernel<…, true> + every wave tier
    _case("ext1_seed68", ext=True, hash_shift=68),
    _case("alph21_k14", alph=21),                                # extractShortFastKernel<…, false>: 20^7 does not fit the half-index
    _case("alph21_k12", alph=21, k=12),                          # extractShortKernel; fastIdx off (base 20 > 16)
    _case("k10", k=10),                                          # extractShortKernel, fastIdx on
    _case("k17", k=17),                                          # no thread-per-sequence kernel: classifyWindowsKernel, fastIdx off
    _case("k23_alph21", k=23, alph=21),                          # widest protein key (20^23 < 2^100: the 64-bit index wraps as the reference's)
    _case("kps20", kps=20),                                      # the short kernel gives up at 19 windows
    _case("kps200", kps=200),                                    # overflowPossible by kps > 120; consideredRaw 199 > CAP 128 from 129 windows on
    _case("kps10_scale05", kps=10, scale=0.5),                   # length-scaled selection; row tier and selected-window cache ineligible
    _case("multi0", multi=False),                                # --ignore-multi-kmer 0
    _case("multi0_kps10_scale05", kps=10, scale=0.5, multi=False),      # ... with hundreds of selected windows: surplus in the threshold bin is the rule
    _case("c09_cov1", c=0.9, cov_mode=1),
    _case("kps1", kps=1),                                        # consideredRaw = 0: identity records only
]
NUCL_CASES = [
    _case("nucl_default", nucl=True),
    _case("nucl_k15_ext0", nucl=True, k=15, ext=False),
    _case("nucl_k24", nucl=True, k=24),                          # 24-byte layout on short sequences
    _case("nucl_k31", nucl=True, k=31),
    _case("nucl_kps20_scale03_multi0_seed3", nucl=True, kps=20, scale=0.3, multi=False, hash_shift=3),
]
CASES = {c["name"]: c for c in AA_CASES + NUCL_CASES}


def oracle_flags(case):
    return ["--alph-size", str(case["alph"]), "--kmer-per-seq", str(case["kps"]), "--kmer-per-seq-scale", "%.3f" % case["scale"], "-k", str(case["k"]),
            "-c", "%g" % case["c"], "--cov-mode", str(case["cov_mode"]), "--ignore-multi-kmer", str(int(case["multi"])), "--hash-shift", str(case["hash_shift"]),
            "--include-only-extendable", str(int(case["ext"]))]


def param_kwargs(case):
    """keyword arguments of plass_amd.KmermatchParams"""
    return dict(k=case["k"], alph_size=case["alph"], kmer_per_seq=case["kps"], kmer_per_seq_scale=case["scale"], hash_shift=case["hash_shift"],
                include_only_extendable=case["ext"], ignore_multi_kmer=case["multi"], cov_mode=case["cov_mode"], c=case["c"])


def case_ladder(case):
    return ladder(case["nucl"], case["k"], case["kps"], case["scale"])


# ---- the oracle's side --------------------------------------------------------------------------------------------------------------
_COUNTS = re.compile(r"oracle kmermatcher: \d+ seqs, N_k=(\d+) N_m=(\d+) N_c=(\d+)")


def oracle_counts(log):
    """(N_k, N_m, N_c) of the line the oracle's kmermatcher prints on stderr"""
    m = _COUNTS.search(log)
    assert m, "no N_k / N_m / N_c line in the oracle's output:\n%s" % log
    return tuple(int(x) for x in m.groups())


def assert_counts(kst, log, what=""):
    """KmermatchStats against the oracle's N_k (records the extraction wrote), N_m (records assignGroup kept) and N_c (candidate lines)"""
    nk, nm, nc = oracle_counts(log)
    got = (int(kst.n_kmer_records), int(kst.n_grouped), int(kst.n_candidates))
    assert got == (nk, nm, nc), "%s: (n_kmer_records, n_grouped, n_candidates) = %r, the oracle's (N_k, N_m, N_c) = %r" % (what, got, (nk, nm, nc))


def read_pref(path):
    """{query key: [target keys other than itself]} of a prefilter DB"""
    path = str(path)
    data = open(path, "rb").read()
    out = {}
    for line in open(path + ".index", "rb"):
        key, o, l = (int(x) for x in line.split()[:3])
        tg = [int(r.split(b"\t", 1)[0]) for r in data[o:o + l].rstrip(b"\0").split(b"\n") if r]
        out[key] = [t for t in tg if t != key]
    return out


def connected_keys(pref):
    """keys with a candidate line naming another sequence, as query or as target"""
    keys = set()
    for q, tg in pref.items():
        if tg:
            keys.add(q); keys.update(tg)
    return keys


def class_coverage(lad, case, pref):
    """{class: number of the ladder's sequences of that class that are connected in `pref`}"""
    conn = connected_keys(pref)
    cov = {}
    for key, L in lad.length_of_key().items():
        c = tier_class(L, case["k"], case["kps"], case["scale"], case["nucl"], case["multi"], case["alph"])
        cov.setdefault(c, 0)
        cov[c] += key in conn
    return cov


def expected_classes(case):
    if case["nucl"] or case["k"] > 16:
        return CLASSES[1:]
    return CLASSES


def check_ladder_reaches_every_class(lad, case, pref, minimum=10):
    """the honesty condition: for every hand-over class at least `minimum` sequences of the class take part in a candidate line with
    another sequence, so a record lost or doubled in that class's kernel changes the candidate DB"""
    cov = class_coverage(lad, case, pref)
    for c in expected_classes(case):
        assert cov.get(c, 0) >= minimum, "%s: class %s has %d connected sequences (%r)" % (case["name"], c, cov.get(c, 0), cov)
    return cov


def check_conditions(lad, case, pref_path, log, main=True):
    """what the oracle's output alone must show before a GPU result is compared with it.  `main`: `lad` is the main ladder of the case
    (under the default flags every hand-over class must then be reached)"""
    pref = read_pref(pref_path)
    assert set(pref) == {int(k) for k in lad.keys}
    nk, nm, nc = oracle_counts(log)
    if case["kps"] == 1:
        assert nk == len(lad.seqs) and nm == 0 and nc == 0          # consideredRaw = 0: identity records only
        return None
    assert nk > len(lad.seqs) and nm > 0 and nc > 0
    if main and case["name"] in ("default", "nucl_default"):
        return check_ladder_reaches_every_class(lad, case, pref, minimum=10)
    return None
