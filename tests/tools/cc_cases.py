"""Hand-made and seeded random inputs of connected-component clustering (`clust --cluster-mode 1`): small sequence DBs and result DBs over them,
written as DB files.  make_cc_inputs.py writes the hand-made ones into tests/golden/cc.tar.gz, where the reference ran on them; the random ones are
made again by every test that needs them and are checked against the restatement (tests/tools/cc_check.py), which the fixture pins.

A case is (name, [(key, length)], {key: [target keys in line order]} — a key without an item has an EMPTY entry —, dbtype)."""
import os
import random
import struct


def write_db(path, entries, dbtype):
    off = 0
    with open(path, "wb") as fd, open(path + ".index", "w") as fi:
        for key, data in entries:
            e = data + b"\0"
            fd.write(e); fi.write("%d\t%d\t%d\n" % (key, off, len(e))); off += len(e)
    with open(path + ".dbtype", "wb") as ft:
        ft.write(struct.pack("<i", dbtype))


def pref_line(i, tkey, qlen):
    return "%d\t%d\t%d\n" % (tkey, 97 + i % 50, i % 7)


def rev_line(i, tkey, qlen):
    return "%d\t%d\t%d\n" % (tkey, -(97 + i % 50) if i % 2 else 97 + i % 50, -(i % 7))


def aln_line(i, tkey, qlen):
    """an alignment line as Matcher::resultToBuffer writes it; every third one with a backtrace column"""
    s = "%d\t%d\t0.%03d\t1.000E-10\t0\t%d\t%d\t0\t%d\t%d" % (tkey, 50 + i % 40, 970 + i % 30, qlen - 1, qlen, qlen - 1, qlen)
    return s + ("\t%dM\n" % qlen if i % 3 == 2 else "\n")


LINE = {7: pref_line, 14: rev_line, 5: aln_line}


def write_case(out, name, seqs, lists, dbtype, rnd, skip_entry=()):
    """<out>/<name> (nucleotide sequence DB) and <out>/<name>_res (result DB); skip_entry: keys that get NO entry in the result DB"""
    seqs = sorted(seqs)
    write_db(os.path.join(out, name), [(k, ("".join(rnd.choice("ACGT") for _ in range(n)) + "\n").encode()) for k, n in seqs], 1)
    write_db(os.path.join(out, name + "_res"), [(k, "".join(LINE[dbtype](i, t, n) for i, t in enumerate(lists.get(k, []))).encode())
                                                for k, n in seqs if k not in skip_entry], dbtype)


def _mixed():
    """keys with gaps and in another order than the lengths.
       A = {3, 10, 17, 40}: 10 lists all four, nobody answers but 40 -> the largest list is neither the smallest nor the largest key
       B = {5, 6, 8} and C = {21, 22, 25}: two cliques, joined by the one line 8 -> 21
       D = {30, 31, 33, 34}: a ring of equal list sizes, lengths 50, 70, 70, 60: the larger id — the SHORTER sequence, key 30 — must win
       E = {50, 51}: 51 lists 50 only (no line to itself), 50 has an empty entry
       60: an empty entry, listed by nobody; 61: lists itself only"""
    seqs = [(3, 80), (10, 45), (17, 90), (40, 30), (5, 61), (6, 62), (8, 63), (21, 64), (22, 65), (25, 66), (30, 50), (31, 70), (33, 70), (34, 60),
            (50, 55), (51, 56), (60, 99), (61, 20)]
    lists = {10: [10, 3, 17, 40], 3: [3], 17: [17], 40: [40, 10],
             5: [5, 6, 8], 6: [6, 5, 8], 8: [8, 5, 6, 21], 21: [21, 22, 25], 22: [22, 21, 25], 25: [25, 21, 22],
             30: [30, 31], 31: [31, 33], 33: [33, 34], 34: [34, 30],
             51: [50], 61: [61]}
    return seqs, lists


def hand_made(rnd):
    """[(name, seqs, lists, dbtype, flags, skip_entry)]"""
    cases = []
    cases.append(("one", [(7, 33)], {7: [7]}, 7, "", ()))
    cases.append(("one_empty", [(7, 33)], {}, 7, "", ()))
    seqs, lists = _mixed()
    for dbtype in (7, 14, 5):
        cases.append(("mixed%d" % dbtype, seqs, lists, dbtype, "--similarity-type 2" if dbtype == 5 else "", ()))
    # an entry that lists one target twice: 2 lists 4 twice and is not answered -> 4's list grows by two
    cases.append(("dup", [(1, 40), (2, 41), (4, 42), (9, 43)], {1: [1, 2], 2: [2, 4, 4], 4: [4], 9: [9, 4]}, 7, "", ()))
    # a star whose hub (key 1000, not the longest sequence) has 5 000 lines; the leaves list themselves
    n = 5000
    seqs = [(k, rnd.randint(20, 40)) for k in range(1, n + 2)]
    hub = 1000
    leaves = [k for k, _ in seqs if k != hub]
    rnd.shuffle(leaves)
    cases.append(("star", seqs, dict([(hub, [hub] + leaves)] + [(k, [k]) for k in leaves]), 7, "", ()))
    # a star that is listed from the leaves only: the hub's entry is empty, its list size is all missing links
    seqs = [(3 * k + 2, rnd.randint(20, 40)) for k in range(1500)]
    hub = seqs[700][0]
    cases.append(("star_in", seqs, {k: [k, hub] for k, _ in seqs if k != hub}, 7, "", ()))
    # a path of 300 in shuffled key order, every line in one direction only: many hook and jump rounds
    keys = list(range(10, 10 + 2 * 300, 2))
    rnd.shuffle(keys)
    seqs = [(k, rnd.randint(20, 40)) for k in keys]
    cases.append(("path300", seqs, {keys[i]: [keys[i], keys[i + 1]] if i + 1 < 300 else [keys[i]] for i in range(300)}, 14, "", ()))
    # the depth rule with --max-iterations 3: R (key 1) lists three leaves and p1, the path goes on p1 -> p2 -> ... -> pk; R has the largest list,
    # its eccentricity is k: k = 4 = m + 1 is the last the order-free rule covers, k = 5 = m + 2 leaves p5 to a later search, which steals p4
    for k, name in ((4, "depth_m1"), (5, "depth_m2")):
        seqs = [(1, 50)] + [(100 + i, 40 + i) for i in range(3)] + [(10 + i, 30 + i) for i in range(1, k + 1)]
        lists = {1: [1, 100, 101, 102, 11]}
        lists.update({100 + i: [100 + i] for i in range(3)})
        lists.update({10 + i: [10 + i] + ([11 + i] if i < k else []) for i in range(1, k + 1)})
        cases.append((name, seqs, lists, 7, "--max-iterations 3", ()))
        if k == 5:
            cases.append((name + "_deeper", seqs, lists, 7, "--max-iterations 4", ()))
    # a sequence without an entry: the reference ends with "Sequence db size != result db size"
    cases.append(("noentry", [(1, 30), (2, 31), (3, 32)], {1: [1, 2], 2: [2], 3: [3]}, 7, "", (3,)))
    return cases


def random_case(seed):
    """a seeded random graph of small dense groups, some joined by single lines, a share of the lines in one direction only, empty entries, keys
    with gaps, many equal lengths -> (seqs, lists, dbtype, max_iterations).  The groups are dense so that most graphs meet the eccentricity
    condition of the order-free rule for the small max_iterations drawn here (tests/test_cc_host.py counts the ones that do not)."""
    rnd = random.Random(seed)
    n = rnd.choice((1, 2, 3, 17, 64, 65, 130, 257, 300))
    keys = sorted(rnd.sample(range(1, 4 * n + 10), n))
    seqs = [(k, rnd.randint(20, 26)) for k in keys]
    lists = {k: ([k] if rnd.random() < 0.7 else []) for k in keys}
    order = keys[:]
    rnd.shuffle(order)
    groups, at = [], 0
    while at < n:
        g = rnd.randint(1, 7)
        groups.append(order[at:at + g]); at += g
    one_way = rnd.choice((0.0, 0.3, 0.8))

    def line(a, b):
        lists[a].append(b)
        if rnd.random() >= one_way:
            lists[b].append(a)
    for g in groups:
        for i, a in enumerate(g):
            for b in g[i + 1:]:
                if rnd.random() < 0.7:
                    line(*rnd.sample((a, b), 2))
    for g, h in zip(groups, groups[1:]):
        if rnd.random() < 0.1:
            line(rnd.choice(g), rnd.choice(h))
    for k in keys:
        rnd.shuffle(lists[k])
    return seqs, {k: v for k, v in lists.items() if v}, rnd.choice((7, 14, 5)), rnd.choice((2, 3, 5))


N_RANDOM = 200
