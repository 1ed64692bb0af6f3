"""mergereads on hand-made read pairs at every edge of plasship_mergereads' kernels (plass_amd/csrc/mergereads.hip).

A seeded builder that needs no GPU.  `rungs()` returns the named rungs; a rung states what it is for and holds a short list of pairs as
they stand in the two FASTQ files (mate 2 BEFORE its reverse complement).  Every pair carries reach conditions: (text, predicate) over
the intermediate values of tests/tools/mergecheck.py's pair_align (`align_pairs(..., trace=...)`, plus `pos`, the offset after the
threshold), so that tests/test_merge_ladder_host.py can assert that the pair is where it was meant to be: on the threshold, in a tie at
the stated distance, decided by the one designed mismatch.  Flanks are random bases of a fixed seed; `alone(i)` asserts that no offset
but the designed one comes near.  What the pairs must give is not stated here: the reference's own FLASH decides that
(tests/golden/make_mergereads_ladder.sh, oracle/tools/flash_pin.cpp -> tests/golden/mergereads_ladder.tar.gz).

    python3 merge_ladder.py <outdir>      writes <outdir>/<rung>_1.fastq, <rung>_2.fastq and <outdir>/RUNGS (the names, in order)

The rules of the reference the kernel's header cites, and the rungs that name them:
  mergereads.cpp:19-23     min_overlap 15, max_overlap 65, density 0.10f, no outies   overlap_len, threshold, nothing_agrees
  mergereads.cpp:52        the shorter file ends the pairs                             (tests/test_gpu_mergereads.py, three records more)
  mergereads.cpp:75-111    reverse_complement, one entry or two, the names             every rung (entries), short_mates, nothing_agrees
  read.cpp:3-8             IUPAC and lower case complemented, U -> A, others '.'       writer (letters), n_rule (n)
  read.cpp:42-47           the quality string reversed                                 quality, ties_keys (qualities sit at chosen places)
  combine_reads.cpp:122-131  'N' in either read is uncalled, else mismatch + min qual  n_rule, quality
  combine_reads.cpp:147-254  the same without 'N' (SSE2 + remainder)                   mask (overlaps of 20-33: one vector and a remainder)
  combine_reads.cpp:270-271  haveN over the whole reads                                n_rule (N outside the overlap)
  combine_reads.cpp:287-289  offsets max(0, l1 - l2) .. l1 - 15                        handover, short_mates, writer (inside), ties_repeat
  combine_reads.cpp:303      overlap >= 15 after the uncalled positions                n_rule (16 with two N), overlap_len
  combine_reads.cpp:304-306  score_len = min(len, 65), float divisions                 overlap_len, threshold, n_rule (70 with six N), ties_keys
  combine_reads.cpp:308-316  smaller density, then smaller quality, then first         ties_repeat, ties_keys, long_mates (64 apart)
  combine_reads.cpp:329      rejected above 0.10f, accepted on it                      threshold, mask
  combine_reads.cpp:345-351  combined length l2 + offset                               writer (lengths)
  combine_reads.cpp:378-381  read 1 before the overlap                                 writer
  combine_reads.cpp:385-432  agreeing base; higher quality; equal: mate 2 unless 'N'   writer
  combine_reads.cpp:442-445  the rest of read 2                                        writer (letters in mate 2's tail)
and the kernel's own edges: the 512 / 513 hand-over to the wave kernel (handover, batch_slots, big_alone, long_mates), the funnel shift at
every i & 3 with the mask of the last word at every overlap & 3 (mask), equal keys in neighbouring lanes, in one lane 16 and 32 offsets
apart and 64 apart in the wave kernel (ties_repeat, ties_keys, long_mates), each byte lane of a dword (n_rule, quality)."""
import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mergecheck  # noqa: E402

SEED = 65
F32 = np.float32
MAXD = mergecheck.MAX_DENSITY
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
NEXT = {65: 67, 67: 71, 71: 84, 84: 65}          # another base
QLONG = np.array([33, 40, 50, 60, 70, 73, 74, 126], dtype=np.uint8)

Pair = collections.namedtuple("Pair", "name s1 q1 s2 q2 reach")


class Rung:
    def __init__(self, name, purpose, k):
        self.name, self.purpose, self.pairs = name, purpose, []
        self.rng = np.random.default_rng([SEED, k])

    # ---- pieces
    def bases(self, n):
        return bytearray(ACGT[self.rng.integers(0, 4, size=n)].tobytes())

    def quals(self, n):
        """35..74 for short reads; eight values, '!' and '~' among them, for long ones (they compress)"""
        if n <= 300:
            return bytearray(self.rng.integers(35, 75, size=n, dtype=np.uint8).tobytes())
        return bytearray(QLONG[self.rng.integers(0, 8, size=n)].tobytes())

    def overlap(self, l1, l2, ov, mm=(), const_q=None):
        """mate 1 of l1 random bases; mate 2 (as aligned) begins with mate 1's last ov bases and goes on with random ones; at the overlap
        positions mm mate 2 gets another base -> s1, q1, s2rc, q2rc (bytearrays)"""
        assert ov <= min(l1, l2)
        s1 = self.bases(l1)
        s2 = s1[l1 - ov:] + self.bases(l2 - ov)
        for j in mm:
            s2[j] = NEXT[s2[j]]
        if const_q is None:
            return s1, self.quals(l1), s2, self.quals(l2)
        return s1, bytearray([const_q]) * l1, s2, bytearray([const_q]) * l2

    def add(self, tag, s1, q1, s2rc, q2rc, *reach):
        """mate 2 given as it is aligned: written to the file reverse-complemented"""
        s2 = mergecheck.revcomp(bytes(s2rc))
        assert mergecheck.revcomp(s2) == bytes(s2rc), "mate 2 holds letters whose complement does not come back: use add_file"
        self.add_file(tag, s1, q1, s2, bytes(q2rc)[::-1], *reach)

    def add_file(self, tag, s1, q1, s2, q2, *reach):
        assert len(s1) == len(q1) and len(s2) == len(q2)
        name = ("%s.%d.%s" % (self.name, len(self.pairs), tag)).encode()
        self.pairs.append(Pair(name, bytes(s1), bytes(q1), bytes(s2), bytes(q2), list(reach)))

    def fastq(self):
        """(file 1, file 2); every third name carries a comment the header DB must drop"""
        f = [b"", b""]
        for k, p in enumerate(self.pairs):
            c = (b" c%d" % k, b"\tx", b"")[k % 3]
            f[0] += b"@%s/1%s\n%s\n+\n%s\n" % (p.name, c, p.s1, p.q1)
            f[1] += b"@%s/2%s\n%s\n+\n%s\n" % (p.name, c, p.s2, p.q2)
        return f[0], f[1]


# ---------------------------------------------------------------------------------------------------------------- reach conditions
def _key(T, i):
    return (T["off"][i][3], T["off"][i][4]) if i in T["off"] and T["off"][i][3] is not None else None


def lengths(l1, l2):
    return ("the mates have %d and %d bases" % (l1, l2), lambda T: (T["l1"], T["l2"]) == (l1, l2))


def merged_at(i):
    return ("merged at offset %d" % i, lambda T: T["pos"] == i)


def rejected():
    return ("not merged", lambda T: T["pos"] == -1)


def best_is(i, ln, mism):
    return ("the best offset before the threshold is %d with %d called positions and %d mismatches" % (i, ln, mism),
            lambda T: T["bp"] == i and T["off"][i][:2] == (ln, mism))


def stats_at(i, ln, mism, qsum=None):
    return ("offset %d has %d called positions, %d mismatches%s" % (i, ln, mism, "" if qsum is None else ", quality sum %d" % qsum),
            lambda T: T["off"][i][:2] == (ln, mism) and (qsum is None or T["off"][i][2] == qsum))


def density_is(m, sl):
    return ("the best density is float32(%d) / float32(%d)" % (m, sl), lambda T: T["bd"] == F32(m) / F32(sl))


def density_on_threshold():
    return ("the best density equals float32(0.10)", lambda T: T["bd"] == MAXD)


def no_candidate(i):
    return ("offset %d is scanned and is no candidate" % i, lambda T: i in T["off"] and T["off"][i][3] is None)


def alone(i):
    """nothing but the designed offset competes: every other candidate is above the threshold and above the designed density"""
    def f(T):
        d0 = T["off"][i][3]
        return all(v[3] is None or v[3] > max(MAXD, d0 if d0 is not None else MAXD) for j, v in T["off"].items() if j != i)
    return ("no offset but %d comes near" % i, f)


def only_candidates(*offs):
    return ("no offset but %s is at or under the threshold" % (offs,),
            lambda T: all(v[3] is None or v[3] > MAXD for j, v in T["off"].items() if j not in offs))


def equal_keys(dist, count=2):
    """at least `count` offsets share the best (density, quality) key, `dist` apart, and the first of all that share it is the best"""
    def f(T):
        same = sorted(i for i in T["off"] if _key(T, i) == (T["bd"], T["bq"]))
        return same[0] == T["bp"] and all(same[0] + dist * c in same for c in range(count))
    return ("%d offsets %d apart share the best key and the first of them wins" % (count, dist), f)


def keys_compare(ia, ib, d, q):
    """d, q in '<', '=', '>': how offset ia's density and quality score compare with offset ib's"""
    def c(x, y, op):
        return {"<": x < y, "=": x == y, ">": x > y}[op]
    return ("offset %d against offset %d: density %s, quality %s" % (ia, ib, d, q),
            lambda T: c(_key(T, ia)[0], _key(T, ib)[0], d) and c(_key(T, ia)[1], _key(T, ib)[1], q))


def scanned(first, last):
    return ("offsets %d .. %d are scanned" % (first, last), lambda T: sorted(T["off"]) == list(range(first, last + 1)))


def most_mismatches(n, qsum):
    return ("some offset has at least %d mismatches and a quality sum of at least %d" % (n, qsum),
            lambda T: any(v[1] >= n and v[2] >= qsum for v in T["off"].values()))


# ---------------------------------------------------------------------------------------------------------------- two-offset pairs
class TwoOffsets:
    """A pair with exactly two offsets that come near: iA with an overlap of ovA and the later iB with ovB <= ovA / 2.  Mate 2 (as aligned)
    begins with P = Y + M + Y, len(Y) = ovB, len(P) = ovA, and mate 1 ends with P.  Mismatches are then placed at one offset only."""

    def __init__(self, r, ovA, ovB, pre=23, post=19, q=60):
        assert 2 * ovB <= ovA
        self.r, self.ovA, self.ovB = r, ovA, ovB
        y = r.bases(ovB)
        p = y + r.bases(ovA - 2 * ovB) + y
        self.s1 = r.bases(pre) + p
        self.s2 = p + r.bases(post)
        self.q1, self.q2 = bytearray([q]) * len(self.s1), bytearray([q]) * len(self.s2)
        self.iA, self.iB = pre, pre + ovA - ovB

    def a_only(self, j, qa, qb):
        """mate 2's base j, ovB <= j < ovA - ovB: outside the later overlap, and mate 1's partner outside it too"""
        assert self.ovB <= j < self.ovA - self.ovB
        self.s2[j] = NEXT[self.s2[j]]
        self.q1[self.iA + j], self.q2[j] = qa, qb

    def a_only_any(self, j, qa, qb):
        """as a_only for ovA = 2 ovB and the like: j >= ovB only (mate 1's partner lies in the later overlap, where it still agrees)"""
        assert self.ovB <= j < self.ovA
        self.s2[j] = NEXT[self.s2[j]]
        self.q1[self.iA + j], self.q2[j] = qa, qb

    def b_only(self, j, qa, qb):
        """mate 2's base j < ovB changed, and mate 1's partner at the earlier offset changed with it"""
        assert j < self.ovB
        self.s2[j] = NEXT[self.s2[j]]
        self.s1[self.iA + j] = self.s2[j]
        self.q1[self.iB + j], self.q2[j] = qa, qb

    def add(self, tag, *reach):
        self.r.add(tag, self.s1, self.q1, self.s2, self.q2, only_candidates(self.iA, self.iB), *reach)


# ---------------------------------------------------------------------------------------------------------------- the rungs
def _handover(r):
    ovs = [15, 64, 65, 66]
    k = 0
    for l1 in (511, 512, 513):
        for l2 in (511, 512, 513):
            ov = ovs[k % 4]; k += 1
            r.add("ov%d" % ov, *r.overlap(l1, l2, ov), lengths(l1, l2), merged_at(l1 - ov), alone(l1 - ov))
            if l2 <= l1:
                r.add("whole", *r.overlap(l1, l2, l2), lengths(l1, l2), merged_at(l1 - l2), scanned(l1 - l2, l1 - 15), alone(l1 - l2))
    r.add("513x15", *r.overlap(513, 15, 15), lengths(513, 15), merged_at(498), scanned(498, 498))
    r.add("15x513", *r.overlap(15, 513, 15), lengths(15, 513), merged_at(0), scanned(0, 0))
    for ov in ovs:                                     # every true overlap on both sides of the hand-over
        r.add("512x512ov%d" % ov, *r.overlap(512, 512, ov), lengths(512, 512), merged_at(512 - ov), alone(512 - ov))
        r.add("513x300ov%d" % ov, *r.overlap(513, 300, ov), lengths(513, 300), merged_at(513 - ov), alone(513 - ov))
        r.add("300x513ov%d" % ov, *r.overlap(300, 513, ov), lengths(300, 513), merged_at(300 - ov), alone(300 - ov))


def _batch_slots(r):
    def big():
        r.add("big", *r.overlap(513, 100, 40, (7,)), lengths(513, 100), merged_at(473), alone(473))

    def small(n):
        for _ in range(n):
            r.add("small", *r.overlap(100, 90, 30, (3,)), merged_at(70), alone(70))
    big(); small(3); big(); small(2); big(); big(); small(1); big()


def _big_alone(r):
    r.add("big", *r.overlap(100, 513, 40, (39,)), lengths(100, 513), merged_at(60), alone(60))


def _overlap_len(r):
    for ov in (13, 14, 15, 16, 17, 63, 64, 65, 66, 67):
        i = 100 - ov
        if ov < 15:
            r.add("ov%d_clean" % ov, *r.overlap(100, 100, ov), rejected(), scanned(0, 85), only_candidates())
            continue
        sl = min(ov, 65); m = sl // 10
        r.add("ov%d_clean" % ov, *r.overlap(100, 100, ov), merged_at(i), stats_at(i, ov, 0), alone(i))
        mm = [0, ov - 1, ov // 2, ov // 3, 2 * ov // 3, ov // 5, 4 * ov // 5]
        r.add("ov%d_mm%d" % (ov, m), *r.overlap(100, 100, ov, mm[:m]), merged_at(i), density_is(m, sl), stats_at(i, ov, m), alone(i))
        r.add("ov%d_mm%d" % (ov, m + 1), *r.overlap(100, 100, ov, mm[:m + 1]), rejected(), best_is(i, ov, m + 1), density_is(m + 1, sl), alone(i))


def _threshold(r):
    for m, ov, acc in ((2, 20, 1), (3, 30, 1), (4, 40, 1), (5, 50, 1), (6, 60, 1), (2, 19, 0), (3, 29, 0), (7, 65, 0), (7, 200, 0), (6, 65, 1),
                       (6, 200, 1), (3, 31, 1)):
        l1, l2 = ov + 37, ov + 41
        mm = sorted(set([0, ov - 1] + [(k * ov) // (m - 1) for k in range(1, m - 1)]))      # the first, the last and m - 2 between
        assert len(mm) == m
        i = l1 - ov
        cond = [best_is(i, ov, m), density_is(m, min(ov, 65)), alone(i), merged_at(i) if acc else rejected()]
        if 10 * m == ov:
            cond.append(density_on_threshold())
        r.add("%d_in_%d" % (m, ov), *r.overlap(l1, l2, ov, mm), *cond)


def _mask(r):
    for a in range(4):
        for ov in (20, 21, 22, 23, 30, 31, 32, 33):
            l1, l2, i = ov + 40 + a, ov + 33, 40 + a
            mm = (0, ov // 2, ov - 1)
            common = [("offset & 3 = %d, overlap & 3 = %d" % (a, ov & 3), lambda T, a=a, ov=ov: T["bp"] & 3 == a and (T["l1"] - T["bp"]) & 3 == ov & 3), alone(i)]
            if ov < 30:                                # three mismatches reject; any two of them accept
                r.add("i%d_ov%d_all" % (a, ov), *r.overlap(l1, l2, ov, mm), rejected(), best_is(i, ov, 3), *common)
                for d, what in enumerate(("first", "middle", "last")):
                    r.add("i%d_ov%d_no_%s" % (a, ov, what), *r.overlap(l1, l2, ov, mm[:d] + mm[d + 1:]), merged_at(i), stats_at(i, ov, 2), *common)
            else:                                      # three accept; a fourth, as a byte counted beyond the overlap would be, rejects
                r.add("i%d_ov%d_three" % (a, ov), *r.overlap(l1, l2, ov, mm), merged_at(i), stats_at(i, ov, 3), *common,
                      ("mate 2 goes on beyond mate 1's end", lambda T, ov=ov: T["l2"] > ov))
                r.add("i%d_ov%d_four" % (a, ov), *r.overlap(l1, l2, ov, mm + (ov // 4,)), rejected(), best_is(i, ov, 4), *common)


def _n_rule(r):
    N = ord("N")

    def put(tag, l1, l2, ov, n1=(), n2=(), mm=(), low=(), *reach, before=()):
        s1, q1, s2, q2 = r.overlap(l1, l2, ov, mm)
        for k in before:                               # 'N' in mate 1 before the overlap
            s1[k] = N
        for j in n1:
            s1[l1 - ov + j] = N
        for j in n2:
            s2[j] = N
        for j, both in low:                            # 'n' is a base
            s1[l1 - ov + j] = ord("n")
            if both:
                s2[j] = ord("n")
        r.add(tag, s1, q1, s2, q2, *reach)
    put("ov16_two_N", 61, 58, 16, (3,), (9,), (), (), rejected(), no_candidate(45), stats_at(45, 14, 0), only_candidates())
    put("ov17_two_N", 61, 58, 17, (3,), (9,), (), (), merged_at(44), stats_at(44, 15, 0), alone(44))
    put("ov16_N_mate1", 61, 58, 16, (5,), (), (11,), (), merged_at(45), stats_at(45, 15, 1), alone(45))
    put("ov16_N_mate2", 61, 58, 16, (), (5,), (11,), (), merged_at(45), stats_at(45, 15, 1), alone(45))
    put("ov16_N_both_one_position", 61, 58, 16, (5,), (5,), (11,), (), merged_at(45), stats_at(45, 15, 1), alone(45))
    for lane in range(4):                              # 'N' in each byte lane: counted as a mismatch (2 / 15) or not seen (2 / 16) it would reject
        put("N_lane%d_mate1" % lane, 62 + lane, 58, 16, (8 + lane,), (), (1,), (), merged_at(46 + lane), stats_at(46 + lane, 15, 1), alone(46 + lane))
        put("N_lane%d_mate2" % lane, 62 + lane, 58, 16, (), (8 + lane,), (1,), (), merged_at(46 + lane), stats_at(46 + lane, 15, 1), alone(46 + lane))
    for ov, j in ((17, 16), (18, 16), (18, 17), (19, 18)):                # in the partial last word
        put("N_last_word_ov%d_at%d_mate1" % (ov, j), 63, 58, ov, (j,), (), (2,), (), merged_at(63 - ov), stats_at(63 - ov, ov - 1, 1), alone(63 - ov))
        put("N_last_word_ov%d_at%d_mate2" % (ov, j), 62, 58, ov, (), (j,), (2,), (), merged_at(62 - ov), stats_at(62 - ov, ov - 1, 1), alone(62 - ov))
    put("ov70_six_N_six_mismatches", 110, 101, 70, (4, 21, 69), (0, 33, 50), (1, 13, 26, 39, 52, 68), (), merged_at(40), stats_at(40, 64, 6),
        density_is(6, 64), alone(40))
    put("ov70_six_N_seven_mismatches", 110, 101, 70, (4, 21, 69), (0, 33, 50), (1, 13, 26, 39, 52, 60, 68), (), rejected(), best_is(40, 64, 7),
        density_is(7, 64), alone(40))
    put("N_outside_the_overlap", 61, 58, 16, (), (), (11,), (), merged_at(45), stats_at(45, 16, 1), alone(45), before=(7,))
    put("n_in_both_is_a_match", 61, 58, 16, (), (), (), ((3, True), (9, True)), merged_at(45), stats_at(45, 16, 0), alone(45))
    put("n_is_a_mismatch", 61, 58, 16, (), (), (11,), ((3, False),), rejected(), best_is(45, 16, 2), alone(45))


def _ties_repeat(r):
    for unit in (1, 2, 3, 4, 16, 17):
        while True:
            u = r.bases(unit)
            if unit == 1 or all(u != u[s:] + u[:s] for s in range(1, unit)):     # no shorter period
                break
        for l1, l2 in ((90, 101), (101, 83)):
            c = 3 % unit
            s1 = (u * 200)[:l1]
            s2 = (u * 200)[c:c + l2]                   # s1[i + j] = s2[j] for i = c (mod unit)
            r.add("unit%d_%dx%d" % (unit, l1, l2), s1, bytearray(b"I") * l1, s2, bytearray(b"I") * l2, lengths(l1, l2), equal_keys(unit, 3),
                  ("the best key is (0, 0)", lambda T: T["bd"] == 0 and T["bq"] == 0),
                  ("the first offset of the period at or after max(0, l1 - l2) wins", lambda T, c=c, unit=unit: T["bp"] == min(i for i in T["off"] if i % unit == c)))
    # unit 16 again, mate 1 the longer, random qualities (none is counted: there is no mismatch)
    u = r.bases(16)
    s1, s2 = (u * 10)[:120], (u * 10)[5:5 + 77]
    r.add("unit16_120x77", s1, r.quals(120), s2, r.quals(77), equal_keys(16, 3), ("the first tie is not the first offset scanned", lambda T: T["bp"] > min(T["off"])))


def _ties_keys(r):
    t = TwoOffsets(r, 40, 20); t.a_only_any(22, 40, 40); t.a_only_any(37, 40, 40); t.b_only(6, 70, 30)
    t.add("equal_density_later_smaller_quality", keys_compare(t.iA, t.iB, "=", ">"), merged_at(t.iB), stats_at(t.iA, 40, 2, 80), stats_at(t.iB, 20, 1, 30))
    t = TwoOffsets(r, 40, 20); t.a_only_any(22, 30, 30); t.a_only_any(37, 30, 30); t.b_only(6, 70, 30)
    t.add("equal_key_first_wins", keys_compare(t.iA, t.iB, "=", "="), merged_at(t.iA), stats_at(t.iA, 40, 2, 60), stats_at(t.iB, 20, 1, 30))
    t = TwoOffsets(r, 48, 16); t.a_only(20, 30, 30); t.a_only(25, 30, 30); t.a_only(30, 30, 30); t.b_only(6, 70, 30)
    t.add("equal_key_same_lane_32_apart", keys_compare(t.iA, t.iB, "=", "="), merged_at(t.iA), stats_at(t.iA, 48, 3, 90), stats_at(t.iB, 16, 1, 30),
          ("the two offsets are 32 apart", lambda T, t=t: t.iB - t.iA == 32))
    t = TwoOffsets(r, 32, 16); t.a_only_any(20, 30, 30); t.a_only_any(25, 30, 30); t.b_only(6, 70, 30)
    t.add("equal_key_same_lane_16_apart", keys_compare(t.iA, t.iB, "=", "="), merged_at(t.iA), stats_at(t.iA, 32, 2, 60), stats_at(t.iB, 16, 1, 30),
          ("the two offsets are 16 apart", lambda T, t=t: t.iB - t.iA == 16))
    t = TwoOffsets(r, 140, 66); t.a_only(67, 50, 50); t.a_only(70, 50, 50); t.b_only(6, 50, 50)
    t.add("later_smaller_density", keys_compare(t.iA, t.iB, ">", ">"), merged_at(t.iB), stats_at(t.iA, 140, 2), stats_at(t.iB, 66, 1))
    t = TwoOffsets(r, 140, 66); t.a_only(67, 40, 90); t.b_only(6, 39, 90)
    t.add("quality_sum_one_less_later_wins", keys_compare(t.iA, t.iB, "=", ">"), merged_at(t.iB), stats_at(t.iA, 140, 1, 40), stats_at(t.iB, 66, 1, 39))
    t = TwoOffsets(r, 140, 66); t.a_only(67, 39, 90); t.b_only(6, 90, 40)
    t.add("quality_sum_one_more_first_wins", keys_compare(t.iA, t.iB, "=", "<"), merged_at(t.iA), stats_at(t.iA, 140, 1, 39), stats_at(t.iB, 66, 1, 40))
    t = TwoOffsets(r, 40, 20); t.a_only_any(22, 90, 90); t.b_only(6, 35, 35)
    t.add("smaller_density_beats_smaller_quality", keys_compare(t.iA, t.iB, "<", ">"), merged_at(t.iA), stats_at(t.iA, 40, 1, 90), stats_at(t.iB, 20, 1, 35))


    # max_overlap is 65, not 64: six mismatches in 120 (6 / 65) against five in 54 lie on either side of 6 / 64
    t = TwoOffsets(r, 120, 54)
    for j in (54, 56, 58, 60, 62, 64):
        t.a_only(j, 60, 60)
    for j in (3, 13, 23, 33, 43):
        t.b_only(j, 60, 60)
    t.add("score_len_65_decides_between_two_offsets", keys_compare(t.iA, t.iB, "<", "<"), merged_at(t.iA), stats_at(t.iA, 120, 6, 360), stats_at(t.iB, 54, 5, 300),
          ("6 / 65 < 5 / 54 < 6 / 64 in float32", lambda T: F32(6) / F32(65) < F32(5) / F32(54) < F32(6) / F32(64)))


def _quality(r):
    # the later offset's one mismatch has min(qa, qb) = 30 in each byte lane and each order; the earlier offset's two sum to 61 or 59:
    # 30 / 20 against 61 / 40 (later wins) and 59 / 40 (first wins).  A minimum taken wrong (50) turns the first kind round.
    for lane in range(4):
        for what, qa, qb in (("lt", 30, 50), ("gt", 50, 30), ("eq", 30, 30)):
            for sa in (61, 59):
                t = TwoOffsets(r, 40, 20); t.a_only_any(22, 30, 30); t.a_only_any(37, sa - 30, sa - 30); t.b_only(8 + lane, qa, qb)
                t.add("min_%s_lane%d_%d" % (what, lane, sa), keys_compare(t.iA, t.iB, "=", ">" if sa == 61 else "<"), merged_at(t.iB if sa == 61 else t.iA),
                      stats_at(t.iA, 40, 2, sa), stats_at(t.iB, 20, 1, 30))
    for what, qa, qb, lo in (("bang_lt", 33, 127, 33), ("bang_gt", 127, 33, 33), ("tilde_del", 126, 127, 126), ("del_tilde", 127, 126, 126)):
        t = TwoOffsets(r, 40, 20, q=127); t.a_only_any(22, lo, lo); t.a_only_any(37, lo + 1, 127); t.b_only(9, qa, qb)
        t.add("bytes_%s" % what, keys_compare(t.iA, t.iB, "=", ">"), merged_at(t.iB), stats_at(t.iA, 40, 2, 2 * lo + 1), stats_at(t.iB, 20, 1, lo))
    t = TwoOffsets(r, 40, 20, q=127); t.a_only_any(22, 127, 127); t.a_only_any(37, 127, 127); t.b_only(9, 127, 127)      # 127 on both sides: equal keys
    t.add("bytes_del_del", keys_compare(t.iA, t.iB, "=", "="), merged_at(t.iA), stats_at(t.iA, 40, 2, 254), stats_at(t.iB, 20, 1, 127))
    s1 = r.bases(100)
    s2 = bytearray(NEXT[c] for c in s1[10:])           # every position of offset 10 disagrees
    r.add("ninety_mismatches_of_top_quality", s1, bytearray([127]) * 100, s2, bytearray([127]) * 90, rejected(), stats_at(10, 90, 90, 90 * 127), most_mismatches(65, 65 * 127))


def _writer(r):
    N = ord("N")
    # one merged pair, overlap 64 at offset 20: positions of the overlap and what stands there
    s1, q1, s2, q2 = r.overlap(84, 90, 64, (), 60)
    i = 20

    def at(j, x=None, y=None, qx=60, qy=60):
        if x is not None:
            s1[i + j] = x
        if y is not None:
            s2[j] = y
        q1[i + j], q2[j] = qx, qy
    at(2, y=NEXT[s2[2]], qx=70, qy=40)                # mismatch, qx > qy: mate 1's base
    at(7, y=NEXT[s2[7]], qx=40, qy=70)                # qx < qy: mate 2's
    at(12, y=NEXT[s2[12]])                            # equal, neither 'N': mate 2's
    at(17, y=N)                                       # equal, y = 'N': mate 1's
    at(22, x=N)                                       # equal, x = 'N': mate 2's
    at(27, x=N, qx=70, qy=40)                         # x = 'N' of higher quality: 'N'
    at(33, y=N, qx=40, qy=70)                         # y = 'N' of higher quality: 'N'
    at(38, x=s1[i + 38] + 32)                         # 'a' against 'A', equal quality: mate 2's
    at(43, x=s1[i + 43] + 32, qx=61)                  # 'a' against 'A', mate 1 higher: 'a'
    at(63, y=NEXT[s2[63]], qx=59)                     # the overlap's last position
    r.add("every_rule_in_one_pair", s1, q1, s2, q2, merged_at(20), stats_at(20, 60, 6), alone(20))
    # letters: mate 2 written as it stands in its file.  Overlap 80 at offset 10, tail of 40.
    s1, q1, s2rc, q2rc = r.overlap(90, 120, 80, (), 60)
    s2 = bytearray(mergecheck.revcomp(bytes(s2rc))); q2 = bytearray(q2rc[::-1])
    f = lambda j: 120 - 1 - j                          # file position of aligned position j
    L = []

    def put(j, ch, x=None, qx=60, qy=60):
        s2[f(j)] = ch
        if x is not None:
            s1[10 + j] = x
        q1[10 + j], q2[f(j)] = qx, qy
        L.append(j)
    put(3, ord("U"), x=ord("A"))                       # U -> A: agrees
    put(8, ord("u"), x=ord("a"))                       # u -> a: agrees
    put(13, ord("X"), x=ord("."))                      # non-IUPAC -> '.': agrees with a '.' in mate 1
    put(18, ord("X"))                                  # '.' against a base, equal quality: '.'
    put(23, ord("R"), x=ord("Y"))
    put(28, ord("k"), x=ord("m"))
    put(33, 0xC3, qx=50, qy=70)                        # a byte over 127: '.', of higher quality
    put(38, ord("A"), x=ord("U"), qx=70, qy=50)        # U in mate 1 stays U: 'T' against 'U', mate 1 higher
    put(43, ord("*"), qx=70, qy=50)                    # '.' of lower quality: mate 1's base
    tail = b"RYKMSWBDHVNUrykmswbdhvnuX*-." + bytes([0xC3]) + b"acgt"
    for k, ch in enumerate(tail):
        s2[f(82 + k)] = ch
    r.add_file("letters", s1, q1, s2, q2, merged_at(10), stats_at(10, 80, 4), alone(10))
    # lengths: l2 > l1 at offset 0, and outputs of 15..17 and 31..33 bytes
    for l2 in (15, 16, 17):
        r.add("out%d" % l2, *r.overlap(15, l2, 15), lengths(15, l2), merged_at(0))
        r.add("out%d" % (16 + l2), *r.overlap(31, l2, 15), lengths(31, l2), merged_at(16), alone(16))
    r.add("l2_longer_offset_0", *r.overlap(40, 75, 40, (0, 39)), lengths(40, 75), merged_at(0), alone(0))
    r.add("mate2_inside_mate1", *r.overlap(60, 25, 25, (0, 24)), lengths(60, 25), merged_at(35), scanned(35, 45), alone(35))


def _short_mates(r):
    for l1 in (1, 14, 15, 16):
        for l2 in (1, 14, 15, 16):
            if min(l1, l2) >= 15:
                r.add("%dx%d" % (l1, l2), *r.overlap(l1, l2, 15), lengths(l1, l2), merged_at(l1 - 15), scanned(max(0, l1 - l2), l1 - 15))
            else:
                r.add("%dx%d" % (l1, l2), r.bases(l1), r.quals(l1), r.bases(l2), r.quals(l2), lengths(l1, l2), rejected(), only_candidates())


def _nothing_agrees(r):
    for l1, l2 in ((100, 90), (90, 100), (600, 90)):
        r.add("A_against_C_%dx%d" % (l1, l2), b"A" * l1, b"I" * l1, b"C" * l2, b"I" * l2, rejected(), density_is(1, 1),
              ("every offset has nothing but mismatches", lambda T: all(v[0] == v[1] for v in T["off"].values())))


def _long_mates(r):
    N = ord("N")
    for l1 in (513, 1000, 5000):
        for l2 in (15, 512, 513, 5000):
            ov = 15 if l2 == 15 else 700 if min(l1, l2) >= 1000 else 513 if (l1, l2) == (513, 513) else 100
            mm = tuple(range(5, ov, 97))[:6] if ov >= 65 else ()
            s1, q1, s2, q2 = r.overlap(l1, l2, ov, mm)
            i = l1 - ov
            nn = 0
            if ov >= 100:                              # 'N' present: two in the overlap, one before it or after it
                s1[i + 50] = N; s2[77] = N; nn = 2
                if i > 0:
                    s1[i // 2] = N
                elif l2 > ov:
                    s2[ov + 3] = N
            r.add("%dx%d" % (l1, l2), s1, q1, s2, q2, lengths(l1, l2), merged_at(i), stats_at(i, ov - nn, len(mm)), alone(i))
    u = r.bases(64)
    s1, s2 = (u * 20)[:1000], (u * 20)[7:7 + 513]
    r.add("tie_64_apart", s1, bytearray(b"I") * 1000, s2, bytearray(b"I") * 513, lengths(1000, 513), equal_keys(64, 3),
          ("the first tie is not the first offset scanned", lambda T: T["bp"] > min(T["off"])))
    t = TwoOffsets(r, 774, 70, pre=100, post=40); t.a_only(200, 60, 60); t.b_only(6, 70, 60)
    t.add("equal_key_704_apart_first_wins", keys_compare(t.iA, t.iB, "=", "="), merged_at(t.iA), stats_at(t.iA, 774, 1, 60), stats_at(t.iB, 70, 1, 60),
          ("the two offsets are 704 apart", lambda T, t=t: t.iB - t.iA == 704),
          ("the overlap of the winner is over 512", lambda T: T["l1"] - T["pos"] > 512))


_RUNGS = (
    ("handover", "mates of 511, 512 and 513 bases in every combination, 513 with 15, true overlaps of 15, 64, 65 and 66 and of a whole mate: the "
                 "row kernel's largest pair and the wave kernel's smallest", _handover),
    ("batch_slots", "pairs for the wave kernel first, last and between pairs for the row kernel", _batch_slots),
    ("big_alone", "one pair for the wave kernel and nothing else: a batch whose row kernel has no pair to decide", _big_alone),
    ("overlap_len", "l1 = l2 = 100 with true overlaps of 13-17 and 63-67, clean, with the most mismatches 0.10 allows and with one more", _overlap_len),
    ("threshold", "mismatch densities on the threshold (equal to float32 0.10: accepted), just over and just under it", _threshold),
    ("mask", "every offset & 3 with every overlap & 3: mismatches at the overlap's first, middle and last position decide; nothing beyond counts", _mask),
    ("n_rule", "'N' shortens the overlap, in either mate, once per position, in every byte lane and in the last word; 'n' is a base", _n_rule),
    ("ties_repeat", "tandem repeats of unit 1, 2, 3, 4, 16 and 17: equal keys in neighbouring lanes and in one lane; the first offset wins", _ties_repeat),
    ("ties_keys", "two offsets that come near: density first, then quality, then the first", _ties_keys),
    ("quality", "min(qa, qb) in every byte lane and order, the quality bytes '!', '~' and 127, ninety mismatches of top quality", _quality),
    ("writer", "generate_combined_read's rules in one pair, letters of every kind, output lengths of 15-17 and 31-33, mate 2 inside mate 1", _writer),
    ("short_mates", "mates of 1, 14, 15 and 16 bases in every combination", _short_mates),
    ("nothing_agrees", "all A against all C: never merged, both entries written", _nothing_agrees),
    ("long_mates", "mates of 513, 1 000 and 5 000 bases with 15, 512, 513 and 5 000, 'N' present, overlaps over 512, ties 64 and 704 offsets apart", _long_mates),
)


_CACHE = []


def rungs():
    """name -> Rung, in order"""
    if not _CACHE:
        out = collections.OrderedDict()
        for k, (name, purpose, fn) in enumerate(_RUNGS):
            r = Rung(name, purpose, k)
            fn(r)
            out[name] = r
        _CACHE.append(out)
    return _CACHE[0]


def fixture():
    """tests/golden/mergereads_ladder.tar.gz -> name -> (file 1, file 2, [(status, [sequence entries without the '\\0'])] per pair): the pairs
    and what the reference's FLASH made of them (tests/golden/make_mergereads_ladder.sh)"""
    import tarfile
    golden = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "mergereads_ladder.tar.gz")
    out = collections.OrderedDict()
    with tarfile.open(golden) as t:
        get = lambda n: t.extractfile("mergereads_ladder/" + n).read()
        for row in get("RUNGS").decode().splitlines():
            name, pairs = row.split("\t")[:2]
            lines = get(name + ".expected").split(b"\n")
            exp, k = [], 0
            while len(exp) < int(pairs):
                st = int(lines[k])
                exp.append((st, [x + b"\n" for x in lines[k + 1:k + (2 if st else 3)]]))
                k += 2 if st else 3
            assert lines[k:] == [b""], name
            out[name] = (get(name + "_1.fastq"), get(name + "_2.fastq"), exp)
    return out


def expected_dbs(f1, f2, exp):
    """-> (sequence entries, header entries, combined): the fixture's entries, and mate 1's name for a merged pair, both names for another"""
    r1, r2 = mergecheck.parse_fastq(f1), mergecheck.parse_fastq(f2)
    assert len(r1) == len(r2) == len(exp)
    seqs, hdrs = [], []
    for (n1, _, _), (n2, _, _), (st, ent) in zip(r1, r2, exp):
        seqs += ent
        hdrs += [n1 + b"\n"] if st else [n1 + b"\n", n2 + b"\n"]
    return seqs, hdrs, sum(st for st, _ in exp)


def main(outdir):
    os.makedirs(outdir, exist_ok=True)
    R = rungs()
    for name, r in R.items():
        f1, f2 = r.fastq()
        open(os.path.join(outdir, name + "_1.fastq"), "wb").write(f1)
        open(os.path.join(outdir, name + "_2.fastq"), "wb").write(f2)
    open(os.path.join(outdir, "RUNGS"), "w").write("".join("%s\t%d\t%s\n" % (n, len(r.pairs), r.purpose) for n, r in R.items()))
    print("%d rungs, %d pairs" % (len(R), sum(len(r.pairs) for r in R.values())))


if __name__ == "__main__":
    main(sys.argv[1])
