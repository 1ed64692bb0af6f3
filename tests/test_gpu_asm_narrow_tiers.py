"""assembleresults' register-queue tiers at their hand-overs: queues of at most 8 record slots run in assembleGroupKernel<8> (eight lanes per
query), 9..16 in <16>, 17..32 in <32>.  A few hundred fragments of one random protein at low depth give every queue size from 2 to 17 among
the queries that pass the pre-screen; every sixth fragment carries substitutions, so that some pairs fail the identity threshold.  The chain runs on the device (the alignment list stays sparse: a query's queue size is its number of
prefilter lines, rejected pairs are holes), and the output must be the CPU oracle's, byte for byte.

What the seeded input contains is not taken on trust: `analyse` below replays the queue fill and the first round of the pop loop from the
oracle's prefilter and alignment DBs, and the tests assert on it that queries of the 8-lane tier defer and re-score hits, extend on both
sides in one round, have two best hits that tie on score and length (the rank among the targets decides), hold holes, and carry the self
line in their first and in their last (eighth) slot.  The library's PLASSHIP_DEBUG_ASMHIST line must report exactly the analysed number of
queries for every tier, so no pass is possible with the narrow queries in a wider kernel."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import AA_AS, AA_KM, AA_RS, ROOT, assert_same_db, read_db, run_oracle
import test_gpu_parity as P

pytestmark = pytest.mark.gpu

SEED, N_FRAGMENTS = 1, 300          # chosen on the CPU with `analyse` (see _check_input)


def make_fragments(seed, n):
    """in the manner of test_gpu_asm_queue.test_high_coverage_queues: fragments of 40-110 residues cut from a random 1 500-residue base"""
    rng = np.random.default_rng(seed)
    aa = list("ACDEFGHIKLMNPQRSTVWY")
    base = "".join(rng.choice(aa, size=1500))
    seqs = []
    for i in range(n):
        p = int(rng.integers(0, 1450)); m = int(rng.integers(40, 110))
        s = list(base[p:p + m])
        if i % 6 == 0:                      # every sixth one with substitutions: pairs that share a k-mer and fail --min-seq-id (holes)
            for j in range(len(s)):
                if rng.random() < 0.12:
                    s[j] = str(rng.choice(aa))
        seqs.append("".join(s))
    return seqs


def self_last(pref):
    """the prefilter entries with the self line of every second query moved from the first to the last place"""
    out = {}
    for q, e in pref.items():
        lines = [l for l in e.split(b"\n") if l.strip(b"\0")]
        if q % 2 == 0 and lines and int(lines[0].split(b"\t")[0]) == q:
            lines = lines[1:] + lines[:1]
        out[q] = b"".join(l + b"\n" for l in lines) + b"\0"
    return out


def write_entries(path, ent, like):
    """a DB file of the entries {key: bytes}, with the dbtype of the DB `like`"""
    off, index = 0, []
    with open(path, "wb") as f:
        for k in sorted(ent):
            f.write(ent[k]); index.append("%d\t%d\t%d\n" % (k, off, len(ent[k]))); off += len(ent[k])
    open(str(path) + ".index", "w").write("".join(index))
    open(str(path) + ".dbtype", "wb").write(open(str(like) + ".dbtype", "rb").read())


def _raw_from_bit():
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "build", "liboracle.so"))
    lib.oracle_raw_from_bit.restype = ctypes.c_double
    lib.oracle_raw_from_bit.argtypes = [ctypes.c_int, ctypes.c_double]
    return lambda bits: int(lib.oracle_raw_from_bit(0, float(bits)) + 0.5)


def analyse(pref, aln, max_seq_len):
    """pref, aln: {key: entry bytes} of the prefilter and the alignment DB (keys = ids).  Returns one dict per query that passes the
    pre-screen: h (record slots), hole, self_slot, and of the first round of the pop loop: both (extends on both sides), defers (a hit is
    deferred and re-scored), tie (the best right- or left-extending hit shares score and length with another one of its kind), broke (the
    left extension would reach the length cap: the pop loop ends) and stay (it does, and hits ranked below the left hit stay queued).
    Only the FIRST round is modelled: what later rounds do is checked by the byte comparison with the oracle alone."""
    raw = _raw_from_bit()
    f32 = np.float32
    res = {}
    for q, pe in pref.items():
        slots = [int(l.split(b"\t")[0]) for l in pe.split(b"\n") if l.strip(b"\0")]
        acc = {}
        for l in aln.get(q, b"").split(b"\n"):
            f = l.strip(b"\0").split(b"\t")
            if len(f) >= 10:
                acc[int(f[0])] = (int(f[1]),) + tuple(int(x) for x in f[4:10])
        assert list(acc) == [t for t in slots if t in acc]                 # the alignments are a subsequence of the prefilter lines
        hits, can, total = [], False, 0
        for t, (bits, qs, qe, ql, ds, de, dl) in acc.items():
            if t == q:
                continue
            total += dl
            right_start, left_start = ds == 0 and de != dl - 1, qs == 0 and qe != ql - 1
            r_branch = l_branch = r_type = l_type = False
            if (right_start or left_start) and not (ds == 0 and qs == 0):
                if ds == 0:
                    r_branch, r_type = True, dl - (de + 1) > 0 and qe == ql - 1
                    can |= r_type
                elif qs == 0:
                    l_branch, l_type = True, ds > 0 and de == dl - 1
                    can |= l_type and ql + ds < max_seq_len
            aln_len = max(abs(qe - max(qs, 0)), abs(de - max(ds, 0))) + 1
            score = int(f32(f32(raw(bits)) / f32(aln_len + 0.5)) * f32(100))
            hits.append(dict(t=t, key=(score, aln_len), r_branch=r_branch, l_branch=l_branch, r_type=r_type, l_type=l_type, frag_r=dl - (de + 1), ds=ds, qe=qe, ql=ql,
                             de=de, dl=dl))
        if not (can and total):
            continue
        # first round: ties broken by the SMALLER target id (CompareResultByScore)
        order = lambda x: (x["key"], -x["t"])
        rs, ls = [x for x in hits if x["r_type"]], [x for x in hits if x["l_type"]]
        best_r, best_l = (max(rs, key=order) if rs else None), (max(ls, key=order) if ls else None)
        tie = any(b is not None and sum(1 for x in k if x["key"] == b["key"]) > 1 for b, k in ((best_r, rs), (best_l, ls)))
        qlen = hits[0]["ql"]
        right_off = best_r["frag_r"] if best_r else 0
        broke = best_l is not None and qlen + (right_off if best_r and (not best_l or order(best_r) > order(best_l)) else 0) + best_l["ds"] >= max_seq_len
        left_off = best_l["ds"] if best_l and not broke else 0
        if broke and best_r and order(best_r) < order(best_l):
            right_off = 0
        defers = False
        for x in hits:
            if x is best_r or x is best_l or (broke and order(x) < order(best_l)):
                continue
            if x["r_branch"]:
                defers |= x["frag_r"] > right_off and x["qe"] == x["ql"] - 1 and right_off > 0
            elif x["l_branch"]:
                defers |= x["ds"] > left_off and x["de"] == x["dl"] - 1 and left_off > 0
        res[q] = dict(h=len(slots), hole=len(acc) < len(slots), self_slot=slots.index(q) if q in slots else -1, both=right_off > 0 and left_off > 0, defers=defers, tie=tie,
                      broke=broke, stay=broke and any(order(x) < order(best_l) for x in hits))
    return res


def tier_counts(res):
    hs = [r["h"] for r in res.values()]
    return [sum(h <= 8 for h in hs), sum(8 < h <= 16 for h in hs), sum(16 < h <= 32 for h in hs), sum(32 < h <= 64 for h in hs), sum(h > 64 for h in hs)]


def _check_input(res):
    """what the issue asks of the seeded input, on the analysis at the default length cap"""
    narrow = [r for r in res.values() if r["h"] <= 8]
    assert {r["h"] for r in res.values()} >= set(range(2, 18)), sorted({r["h"] for r in res.values()})
    assert any(r["defers"] for r in narrow) and any(r["both"] for r in narrow) and any(r["tie"] for r in narrow)
    assert any(r["hole"] and r["h"] == 8 for r in narrow)
    assert any(r["self_slot"] == 0 for r in narrow) and any(r["self_slot"] == 7 and r["h"] == 8 for r in narrow)


@pytest.fixture(scope="module")
def ctx():
    import plass_amd
    c = plass_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def case(oracle_bin, tmp_path_factory):
    """the seeded DB, the oracle's prefilter DB with every second self line moved to the end (kmermatcher writes it first), and the oracle's
    alignment DB of that, made once"""
    d = tmp_path_factory.mktemp("narrow")
    P._write_fasta_like_db(d / "seq", make_fragments(SEED, N_FRAGMENTS), 0)
    run_oracle(oracle_bin, ["kmermatcher", d / "seq", d / "o_pref"] + AA_KM + ["--hash-shift", "67", "--include-only-extendable", "0"])
    write_entries(d / "p_pref", self_last(read_db(d / "o_pref")[1]), d / "o_pref")
    run_oracle(oracle_bin, ["rescorediagonal", d / "seq", d / "seq", d / "p_pref", d / "o_aln"] + AA_RS)
    return d, read_db(d / "p_pref")[1], read_db(d / "o_aln")[1]


def test_input_has_the_cases(case):
    _, pref, aln = case
    _check_input(analyse(pref, aln, 65535))
    capped = analyse(pref, aln, 400)
    assert tier_counts(capped)[0] > 0 and tier_counts(capped)[1] > 0
    # A query grows by at most one target on either side (a deferred hit extends only as far as it reaches beyond the best one), so these
    # fragments of at most 109 residues never come near 400: that cap checks only that nothing changes.  120 is a cap they do reach.
    assert not any(r["broke"] for r in capped.values())
    tight = analyse(pref, aln, 120)
    assert any(r["broke"] and r["h"] <= 8 for r in tight.values())            # an 8-lane query ends at the length cap ...
    assert any(r["stay"] and r["h"] <= 8 for r in tight.values())             # ... with hits ranked below the left hit still queued


@pytest.mark.parametrize("max_seq_len", [65535, 400, 120])
@pytest.mark.parametrize("keep_target", [0, 1])
def test_narrow_tiers(ctx, case, oracle_bin, tmp_path, capfd, monkeypatch, keep_target, max_seq_len):
    import plass_amd
    d, pref, aln = case
    expect = tier_counts(analyse(pref, aln, max_seq_len))
    db = ctx.read_seqdb(d / "seq")
    cands, _ = ctx.kmermatcher(db, P.km_params(0))
    cands.write(tmp_path / "g_pref")
    assert_same_db(d / "o_pref", tmp_path / "g_pref", "narrow tiers kmermatcher")
    alns, _ = ctx.rescorediagonal(db, db, ctx.read_prefdb(db, db, d / "p_pref"), plass_amd.RescoreParams(min_seq_id=0.9))
    alns.write(tmp_path / "g_aln")
    assert_same_db(d / "o_aln", tmp_path / "g_aln", "narrow tiers rescorediagonal")
    flags = list(AA_AS)
    flags[flags.index("--max-seq-len") + 1] = str(max_seq_len)
    flags[flags.index("--keep-target") + 1] = str(keep_target)
    run_oracle(oracle_bin, ["assembleresults", d / "seq", d / "o_aln", tmp_path / "o_seq"] + flags)
    monkeypatch.setenv("PLASSHIP_DEBUG_ASMHIST", "1")
    capfd.readouterr()
    out, st = ctx.assembleresults(db, alns, plass_amd.AssembleParams(min_seq_id=0.9, max_seq_len=max_seq_len, keep_target=bool(keep_target)))
    err = capfd.readouterr().err
    out.write(tmp_path / "g_seq")
    assert_same_db(tmp_path / "o_seq", tmp_path / "g_seq", f"narrow tiers assembleresults, keep-target {keep_target}, max-seq-len {max_seq_len}")
    m = re.findall(r"asmHist call \d+ .*\| tier queries <=8,<=16,<=32,<=64,more: (\d+) (\d+) (\d+) (\d+) (\d+)", err)
    assert m, err
    got = [int(x) for x in m[-1]]
    assert got == expect and got[0] > 0 and got[1] > 0 and got[2] > 0, (got, expect)
    assert st.tier_alignments[0] > 0
