"""GPU parity tests (run with `-m gpu` on an MI355X): the HIP path through the C-ABI (ctypes binding of
include/plasship.h) against (a) golden DBs written by the unmodified reference and (b) the CPU oracle on
seeded synthetic and adversarial inputs.  Everything is bit-exact: DB entries are compared byte for byte."""
import os
import sys

import numpy as np
import pytest

from conftest import (AA_AS, AA_KM, AA_RS, GD_AS, GD_KM, GD_P2N, GD_RS, NUCL_AS, NUCL_KM, NUCL_RS, ROOT, aa_iter_flags, assert_same_db, read_db, run_oracle,
                      sweep_positional, sweep_variants)

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
from extract_ladder import assert_counts  # noqa: E402  (KmermatchStats against the oracle's N_k / N_m / N_c)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import plass_amd
    c = plass_amd.Context(0)
    yield c
    c.close()


def km_params(it, nucl=False):
    import plass_amd
    if nucl:
        return plass_amd.KmermatchParams(k=22, alph_size=5, kmer_per_seq=60, kmer_per_seq_scale=0.1, hash_shift=67,
                                         include_only_extendable=True, ignore_multi_kmer=True, cov_mode=0, c=0.0)
    return plass_amd.KmermatchParams(k=14, alph_size=13, kmer_per_seq=60, kmer_per_seq_scale=0.0, hash_shift=67 if it == 0 else 68,
                                     include_only_extendable=(it > 0), ignore_multi_kmer=True, cov_mode=0, c=0.0)


@pytest.mark.parametrize("it", [0, 1, 2])
def test_golden_aa_modules(ctx, golden, tmp_path, it):
    """each module separately, inputs = the reference's DBs, outputs must equal the reference's DBs"""
    import plass_amd
    s = os.path.join(golden, "aa")
    db = ctx.read_seqdb(f"{s}/seq_{it}")
    cands, st = ctx.kmermatcher(db, km_params(it))
    cands.write(tmp_path / "pref")
    assert_same_db(f"{s}/pref_{it}", tmp_path / "pref", "kmermatcher")
    pref = ctx.read_prefdb(db, db, f"{s}/pref_{it}")
    alns, _ = ctx.rescorediagonal(db, db, pref, plass_amd.RescoreParams(min_seq_id=0.9))
    alns.write(tmp_path / "aln")
    assert_same_db(f"{s}/aln_{it}", tmp_path / "aln", "rescorediagonal")
    aln_in = ctx.read_alndb(db, f"{s}/aln_{it}")
    out, _ = ctx.assembleresults(db, aln_in, plass_amd.AssembleParams(min_seq_id=0.9))
    out.write(tmp_path / "seq")
    assert_same_db(f"{s}/seq_{it + 1}", tmp_path / "seq", "assembleresults")


def test_golden_aa_modules_through_the_row_kernels(ctx, golden, tmp_path, monkeypatch):
    """the reference-written golden DBs of the bundled example with the four-sequences-per-wavefront extraction kernels forced (round 6; by default
    they take sets of 4 M sequences and more)"""
    monkeypatch.setenv("PLASSHIP_TUNE_ROWTIER", "3")
    for it in (0, 1, 2):
        test_golden_aa_modules(ctx, golden, tmp_path, it)


def test_golden_aa_chained_on_device(ctx, golden, tmp_path):
    """three iterations without touching disk in between: the contigs must equal the reference's"""
    import plass_amd
    s = os.path.join(golden, "aa")
    db = ctx.read_seqdb(f"{s}/seq_0")
    for it in range(3):
        cands, _ = ctx.kmermatcher(db, km_params(it))
        alns, _ = ctx.rescorediagonal(db, db, cands, plass_amd.RescoreParams(min_seq_id=0.9))
        db2, _ = ctx.assembleresults(db, alns, plass_amd.AssembleParams(min_seq_id=0.9))
        db2.write(tmp_path / f"seq_{it + 1}")
        assert_same_db(f"{s}/seq_{it + 1}", tmp_path / f"seq_{it + 1}", f"chained iteration {it}")
        alns.free(); cands.free()
        db = db2


def test_golden_aa_keep_target0(ctx, golden, tmp_path):
    import plass_amd
    s = os.path.join(golden, "aa")
    db = ctx.read_seqdb(f"{s}/seq_0")
    aln_in = ctx.read_alndb(db, f"{s}/aln_0")
    out, _ = ctx.assembleresults(db, aln_in, plass_amd.AssembleParams(min_seq_id=0.9, keep_target=False))
    out.write(tmp_path / "seq")
    assert_same_db(f"{s}/seq_1_keeptarget0", tmp_path / "seq", "keep-target 0")


@pytest.mark.parametrize("it", [0, 1])
def test_golden_nucl_kmermatcher_rescore(ctx, golden, tmp_path, it):
    import plass_amd
    s = os.path.join(golden, "nucl")
    db = ctx.read_seqdb(f"{s}/seq_{it}")
    cands, _ = ctx.kmermatcher(db, km_params(it, nucl=True))
    cands.write(tmp_path / "pref")
    assert_same_db(f"{s}/pref_{it}", tmp_path / "pref", "nucl kmermatcher")
    alns, _ = ctx.rescorediagonal(db, db, cands, plass_amd.RescoreParams(min_seq_id=0.99))
    alns.write(tmp_path / "aln")
    assert_same_db(f"{s}/aln_{it}", tmp_path / "aln", "nucl rescorediagonal")


def test_golden_nucleotide_strand_ties(ctx, golden, tmp_path):
    """a (rep, target, diagonal) triple with records of both strands: the pair's strand is that of the member with the largest k-mer
    (the reference's effective order, kmermatcher.h:98-130 / kmermatcher.cpp:866-893; tests/golden/make_strand_ties.py) — the
    reference's pref and aln DBs"""
    import plass_amd
    s = os.path.join(golden, "strand_ties")
    db = ctx.read_seqdb(f"{s}/seq_0")
    cands, _ = ctx.kmermatcher(db, km_params(0, nucl=True))
    cands.write(tmp_path / "pref")
    assert_same_db(f"{s}/pref_0", tmp_path / "pref", "strand ties kmermatcher")
    alns, _ = ctx.rescorediagonal(db, db, cands, plass_amd.RescoreParams(min_seq_id=0.99))
    alns.write(tmp_path / "aln")
    assert_same_db(f"{s}/aln_0", tmp_path / "aln", "strand ties rescorediagonal")


def nucl_as_params():
    import plass_amd
    return plass_amd.AssembleParams(min_seq_id=0.99, max_seq_len=200000)


@pytest.mark.parametrize("it", [0, 1])
def test_golden_nucl_assembleresults(ctx, golden, tmp_path, it):
    """nuclassembleresults (Bayesian comparator, libstdc++ heap order, reverse-strand hits): the reference's contigs"""
    s = os.path.join(golden, "nucl")
    db = ctx.read_seqdb(f"{s}/seq_{it}")
    aln_in = ctx.read_alndb(db, f"{s}/aln_{it}")
    out, st = ctx.assembleresults(db, aln_in, nucl_as_params())
    out.write(tmp_path / "seq")
    assert_same_db(f"{s}/seq_{it + 1}", tmp_path / "seq", "nuclassembleresults")
    assert st.n_extended > 0


def test_golden_nucl_chained_on_device(ctx, golden, tmp_path):
    import plass_amd
    s = os.path.join(golden, "nucl")
    db = ctx.read_seqdb(f"{s}/seq_0")
    for it in range(2):
        cands, _ = ctx.kmermatcher(db, km_params(it, nucl=True))
        alns, _ = ctx.rescorediagonal(db, db, cands, plass_amd.RescoreParams(min_seq_id=0.99))
        db2, _ = ctx.assembleresults(db, alns, nucl_as_params())
        db2.write(tmp_path / f"seq_{it + 1}")
        assert_same_db(f"{s}/seq_{it + 1}", tmp_path / f"seq_{it + 1}", f"nucl chained iteration {it}")
        db = db2


@pytest.mark.parametrize("it", [0, 1])
def test_golden_long_nucleotide_contigs(ctx, golden, tmp_path, it):
    """contigs of 17-36 kb growing to 70 kb (KmerPosition<int>, 16-bit diagonal wrap-around, contig-contig reverse-strand
    overlaps): every module on the reference's DBs"""
    import plass_amd
    s = os.path.join(golden, "longnucl")
    db = ctx.read_seqdb(f"{s}/seq_{it}")
    assert db.info()["max_entry_len"] > 32767
    cands, _ = ctx.kmermatcher(db, km_params(it, nucl=True))
    cands.write(tmp_path / "pref")
    assert_same_db(f"{s}/pref_{it}", tmp_path / "pref", "long nucl kmermatcher")
    pref = ctx.read_prefdb(db, db, f"{s}/pref_{it}")
    alns, _ = ctx.rescorediagonal(db, db, pref, plass_amd.RescoreParams(min_seq_id=0.99))
    alns.write(tmp_path / "aln")
    assert_same_db(f"{s}/aln_{it}", tmp_path / "aln", "long nucl rescorediagonal")
    aln_in = ctx.read_alndb(db, f"{s}/aln_{it}")
    out, _ = ctx.assembleresults(db, aln_in, nucl_as_params())
    out.write(tmp_path / "seq")
    assert_same_db(f"{s}/seq_{it + 1}", tmp_path / "seq", "long nucl nuclassembleresults")


@pytest.mark.parametrize("ext", [False, True])
def test_golden_adversarial_inputs(ctx, golden, tmp_path, ext):
    """hostile protein and nucleotide inputs, every module on the reference's DBs (adversarial.tar.gz)"""
    import plass_amd
    s = os.path.join(golden, "adversarial")
    e = int(ext)
    db = ctx.read_seqdb(f"{s}/aa_seq")
    par = km_params(0); par.include_only_extendable = ext
    cands, _ = ctx.kmermatcher(db, par)
    cands.write(tmp_path / "p")
    assert_same_db(f"{s}/aa_pref{e}", tmp_path / "p", "adversarial aa kmermatcher")
    alns, _ = ctx.rescorediagonal(db, db, ctx.read_prefdb(db, db, f"{s}/aa_pref{e}"), plass_amd.RescoreParams(min_seq_id=0.9))
    alns.write(tmp_path / "a")
    assert_same_db(f"{s}/aa_aln{e}", tmp_path / "a", "adversarial aa rescorediagonal")
    out, _ = ctx.assembleresults(db, ctx.read_alndb(db, f"{s}/aa_aln{e}"), plass_amd.AssembleParams(min_seq_id=0.9))
    out.write(tmp_path / "o")
    assert_same_db(f"{s}/aa_out{e}", tmp_path / "o", "adversarial aa assembleresults")
    ndb = ctx.read_seqdb(f"{s}/nucl_seq")
    npar = km_params(0, nucl=True); npar.include_only_extendable = ext
    cands, _ = ctx.kmermatcher(ndb, npar)
    cands.write(tmp_path / "np")
    assert_same_db(f"{s}/n_pref{e}", tmp_path / "np", "adversarial nucl kmermatcher")
    alns, _ = ctx.rescorediagonal(ndb, ndb, ctx.read_prefdb(ndb, ndb, f"{s}/n_pref{e}"), plass_amd.RescoreParams(min_seq_id=0.99))
    alns.write(tmp_path / "na")
    assert_same_db(f"{s}/n_aln{e}", tmp_path / "na", "adversarial nucl rescorediagonal")
    out, _ = ctx.assembleresults(ndb, ctx.read_alndb(ndb, f"{s}/n_aln{e}"), nucl_as_params())
    out.write(tmp_path / "no")
    assert_same_db(f"{s}/n_out{e}", tmp_path / "no", "adversarial nucl nuclassembleresults")


def test_synthetic_nucl_three_iterations_vs_oracle(ctx, oracle_bin, tmp_path):
    """15 k read pairs of a synthetic genome, both strands: every DB of three penguin-style iterations equals the oracle's"""
    import plass_amd
    from plass_amd import synth
    data, off, elen, key = synth.nucleotide_read_db(15000, seed=17)
    synth.write_db(str(tmp_path / "o_seq_0"), data, off, elen, key, 1)
    db = ctx.upload_seqdb(data, off, elen, key, 1)
    for it in range(3):
        log = run_oracle(oracle_bin, ["kmermatcher", tmp_path / f"o_seq_{it}", tmp_path / f"o_pref_{it}"] + NUCL_KM)
        run_oracle(oracle_bin, ["rescorediagonal", tmp_path / f"o_seq_{it}", tmp_path / f"o_seq_{it}", tmp_path / f"o_pref_{it}", tmp_path / f"o_aln_{it}"] + NUCL_RS)
        run_oracle(oracle_bin, ["nuclassembleresults", tmp_path / f"o_seq_{it}", tmp_path / f"o_aln_{it}", tmp_path / f"o_seq_{it + 1}"] + NUCL_AS)
        cands, kst = ctx.kmermatcher(db, km_params(it, nucl=True))
        cands.write(tmp_path / "g_pref")
        assert_same_db(tmp_path / f"o_pref_{it}", tmp_path / "g_pref", f"nucl kmermatcher it{it}")
        assert_counts(kst, log, f"nucl kmermatcher it{it}")
        alns, rst = ctx.rescorediagonal(db, db, cands, plass_amd.RescoreParams(min_seq_id=0.99))
        alns.write(tmp_path / "g_aln")
        assert_same_db(tmp_path / f"o_aln_{it}", tmp_path / "g_aln", f"nucl rescorediagonal it{it}")
        db2, ast = ctx.assembleresults(db, alns, nucl_as_params())
        db2.write(tmp_path / "g_seq")
        assert_same_db(tmp_path / f"o_seq_{it + 1}", tmp_path / "g_seq", f"nuclassembleresults it{it}")
        if it == 0:
            assert ast.n_extended > 1000
        db = db2


def gd_km_params():
    import plass_amd
    return plass_amd.KmermatchParams(k=14, alph_size=13, kmer_per_seq=60, kmer_per_seq_scale=0.1, hash_shift=67,
                                     include_only_extendable=True, ignore_multi_kmer=True, cov_mode=1, c=0.0)


def gd_rs_params():
    import plass_amd
    return plass_amd.RescoreParams(min_seq_id=0.97, cov_mode=1, a=True)


def test_synthetic_hairpin_genome_strand_ties_vs_oracle(ctx, oracle_bin, tmp_path):
    """20 k read pairs of a genome with 40 planted inverted repeats at 30x: dozens of (rep, target, diagonal) triples hold records of
    both strands, in hub queries with many targets, over two iterations (contig-contig ties in the second) — every DB against the oracle,
    and the oracle must have met ties (its log says so)"""
    import plass_amd
    from plass_amd import synth
    reads, _ = synth.nucleotide_hairpin_reads(20000, 40, seed=23, coverage=30.0)
    data, off, elen, key = synth.fixed_length_db(reads)
    synth.write_db(str(tmp_path / "o_seq_0"), data, off, elen, key, 1)
    db = ctx.upload_seqdb(data, off, elen, key, 1)
    ties = 0
    for it in range(2):
        log = run_oracle(oracle_bin, ["kmermatcher", tmp_path / f"o_seq_{it}", tmp_path / f"o_pref_{it}"] + NUCL_KM)
        ties += sum(int(l.split(": ", 1)[1].split()[0]) for l in log.splitlines() if "hold both strands" in l)
        run_oracle(oracle_bin, ["rescorediagonal", tmp_path / f"o_seq_{it}", tmp_path / f"o_seq_{it}", tmp_path / f"o_pref_{it}", tmp_path / f"o_aln_{it}"] + NUCL_RS)
        run_oracle(oracle_bin, ["nuclassembleresults", tmp_path / f"o_seq_{it}", tmp_path / f"o_aln_{it}", tmp_path / f"o_seq_{it + 1}"] + NUCL_AS)
        cands, _ = ctx.kmermatcher(db, km_params(it, nucl=True))
        cands.write(tmp_path / "g_pref")
        assert_same_db(tmp_path / f"o_pref_{it}", tmp_path / "g_pref", f"hairpin kmermatcher it{it}")
        alns, _ = ctx.rescorediagonal(db, db, cands, plass_amd.RescoreParams(min_seq_id=0.99))
        db2, _ = ctx.assembleresults(db, alns, nucl_as_params())
        db2.write(tmp_path / "g_seq")
        assert_same_db(tmp_path / f"o_seq_{it + 1}", tmp_path / "g_seq", f"hairpin nuclassembleresults it{it}")
        db = db2
    assert ties >= 10, "the read set holds no strand ties: the test does not reach the rule it is for"


def test_golden_guided_modules(ctx, golden, tmp_path):
    """penguin's protein-guided stage, module by module on the reference's DBs: kmermatcher and rescorediagonal -a 1 on
    the translated ORFs, proteinaln2nucl, guidedassembleresults (nucleotide ORFs + protein twins)"""
    import plass_amd
    s = os.path.join(golden, "guided")
    aa = ctx.read_seqdb(f"{s}/aa_0"); nu = ctx.read_seqdb(f"{s}/nucl_0")
    cands, _ = ctx.kmermatcher(aa, gd_km_params())
    cands.write(tmp_path / "pref")
    assert_same_db(f"{s}/pref_0", tmp_path / "pref", "guided kmermatcher")
    pref = ctx.read_prefdb(aa, aa, f"{s}/pref_0")
    alns, _ = ctx.rescorediagonal(aa, aa, pref, gd_rs_params())
    alns.write(tmp_path / "aln")
    assert_same_db(f"{s}/aln_0", tmp_path / "aln", "guided rescorediagonal -a 1")
    aln_in = ctx.read_alndb(aa, f"{s}/aln_0")                      # text with backtrace column
    naln, _ = ctx.proteinaln2nucl(nu, aa, aln_in)
    naln.write(tmp_path / "aln_nucl")
    assert_same_db(f"{s}/aln_nucl_0", tmp_path / "aln_nucl", "proteinaln2nucl")
    naln_in = ctx.read_alndb(nu, f"{s}/aln_nucl_0")
    on, oa, st = ctx.guidedassembleresults(nu, aa, naln_in)
    on.write(tmp_path / "nucl_1"); oa.write(tmp_path / "aa_1")
    assert_same_db(f"{s}/nucl_1", tmp_path / "nucl_1", "guidedassembleresults nucl")
    assert_same_db(f"{s}/aa_1", tmp_path / "aa_1", "guidedassembleresults aa")
    assert st.n_extended > 100


def test_golden_guided_chained_on_device(ctx, golden, tmp_path):
    """two guided iterations without touching disk: the contigs and their protein twins equal the reference's"""
    s = os.path.join(golden, "guided")
    aa = ctx.read_seqdb(f"{s}/aa_0"); nu = ctx.read_seqdb(f"{s}/nucl_0")
    for it in range(2):
        cands, _ = ctx.kmermatcher(aa, gd_km_params())
        alns, _ = ctx.rescorediagonal(aa, aa, cands, gd_rs_params())
        naln, _ = ctx.proteinaln2nucl(nu, aa, alns)
        nu2, aa2, _ = ctx.guidedassembleresults(nu, aa, naln)
        nu2.write(tmp_path / f"nucl_{it + 1}"); aa2.write(tmp_path / f"aa_{it + 1}")
        assert_same_db(f"{s}/nucl_{it + 1}", tmp_path / f"nucl_{it + 1}", f"guided chained nucl it{it}")
        assert_same_db(f"{s}/aa_{it + 1}", tmp_path / f"aa_{it + 1}", f"guided chained aa it{it}")
        nu, aa = nu2, aa2


def test_golden_cyclecheck(ctx, golden, tmp_path):
    """row N4 on the reference's outputs: both --chop-cycle modes, the remainder DB the workflow continues with, and the
    example's contigs (none circular: empty DBs)"""
    c = os.path.join(golden, "cyc")
    db = ctx.read_seqdb(f"{c}/in")
    for chop in (False, True):
        cyc, rest, st = ctx.cyclecheck(db, max_seq_len=50000, chop_cycle=chop, with_rest=True)
        cyc.write(tmp_path / f"c{int(chop)}"); rest.write(tmp_path / f"r{int(chop)}")
        assert_same_db(f"{c}/cycle_chop{int(chop)}", tmp_path / f"c{int(chop)}", f"cyclecheck chop {chop}")
        assert st.n_cyclic == 64 and st.n_wave_small > 300 and st.n_wave_large > 10 and st.n_block > 20
        _, ein = read_db(f"{c}/in"); _, ec = read_db(tmp_path / f"c{int(chop)}"); _, er = read_db(tmp_path / f"r{int(chop)}")
        assert set(ec) | set(er) == set(ein) and not (set(ec) & set(er)) and all(er[k] == ein[k] for k in er)
    for src, name in ((os.path.join(golden, "nucl", "seq_2"), "nucl_seq_2"), (os.path.join(golden, "longnucl", "seq_0"), "longnucl_seq_0"),
                      (os.path.join(golden, "longnucl", "seq_2"), "longnucl_seq_2")):
        cyc, _ = ctx.cyclecheck(ctx.read_seqdb(src), max_seq_len=200000, chop_cycle=True)
        cyc.write(tmp_path / name)
        assert_same_db(f"{c}/{name}_cycle", tmp_path / name, f"cyclecheck {name}")


def _cyclecheck_cases(rng, n_random, long_ones):
    B = "ACGT"
    rnd = lambda n: "".join(B[i] for i in rng.integers(0, 4, n))
    seqs = []
    for _ in range(n_random):
        n = int(rng.integers(40, 60000) if rng.random() < 0.3 else rng.integers(40, 3000))
        g = rnd(n)
        kind = int(rng.integers(0, 5))
        if kind == 0:
            seqs.append(g)
        elif kind == 1:
            seqs.append(g + g[:int(rng.integers(22, n + 1))])
        elif kind == 2:
            x = g[:int(rng.integers(22, n + 1))]
            seqs.append(g + "".join(c if rng.random() > 0.03 else B[int(rng.integers(0, 4))] for c in x))
        elif kind == 3:
            u = rnd(int(rng.integers(5, 200))); seqs.append((u * (n // len(u) + 1))[:n])
        else:
            seqs.append(g[:n // 2] + "N" * int(rng.integers(1, 50)) + g[:n // 2])
    if long_ones:
        # round 4: contigs that need several passes over the LDS table (a phase of a 130 kb contig holds 43 k k-mers, the table 4 k per
        # pass), and two beyond 2^18 letters (position and k-mer no longer share a 64-bit entry: the HBM-table kernel)
        g = rnd(130000); seqs.append(g + g[:40000])
        seqs.append(rnd(150000))
        g = rnd(90000); seqs.append(g[:45000] + "N" * 7 + g[:45000] + g[45000:])
        g = rnd(200000); seqs.append(g + g[:75000])
        seqs.append(rnd(270000))
    return seqs


def test_cyclecheck_vs_oracle(ctx, oracle_bin, tmp_path):
    """reads + random circular / linear / repetitive contigs of all kernel tiers against the oracle"""
    from plass_amd import synth
    seqs = _cyclecheck_cases(np.random.default_rng(23), 120, True)
    data, off, elen, key = synth.nucleotide_read_db(3000, seed=9)
    synth.write_db(str(tmp_path / "reads"), data, off, elen, key, 1)
    _, er = read_db(tmp_path / "reads")
    seqs += [v[:-2].decode() for v in list(er.values())[:2000]]
    _write_fasta_like_db(tmp_path / "seq", seqs, dbtype=1)
    db = ctx.read_seqdb(tmp_path / "seq")
    n_cyc = 0
    for chop in (0, 1):
        run_oracle(oracle_bin, ["cyclecheck", tmp_path / "seq", tmp_path / f"o{chop}", "--max-seq-len", "300000", "--chop-cycle", chop])
        cyc, st = ctx.cyclecheck(db, max_seq_len=300000, chop_cycle=bool(chop))
        cyc.write(tmp_path / f"g{chop}")
        assert_same_db(tmp_path / f"o{chop}", tmp_path / f"g{chop}", f"cyclecheck vs oracle, chop {chop}")
        n_cyc = st.n_cyclic
        assert st.n_block >= 7 and st.n_wave_large > 20
    assert n_cyc > 20


def test_cyclecheck_table_overflow_falls_back(ctx, oracle_bin, tmp_path, monkeypatch):
    """a contig whose k-mers do not fit the LDS table of a pass is handed to the HBM-table kernel: forced here by allowing the workgroup
    tier ONE pass whatever the length (PLASSHIP_TUNE_CYC_PASSES=1), so every contig beyond ~12 kb overflows; results as the oracle's"""
    seqs = _cyclecheck_cases(np.random.default_rng(31), 60, True)
    _write_fasta_like_db(tmp_path / "seq", seqs, dbtype=1)
    db = ctx.read_seqdb(tmp_path / "seq")
    run_oracle(oracle_bin, ["cyclecheck", tmp_path / "seq", tmp_path / "o", "--max-seq-len", "300000", "--chop-cycle", 1])
    cyc, st0 = ctx.cyclecheck(db, max_seq_len=300000, chop_cycle=True)
    monkeypatch.setenv("PLASSHIP_TUNE_CYC_PASSES", "1")
    cyc, st = ctx.cyclecheck(db, max_seq_len=300000, chop_cycle=True)
    monkeypatch.delenv("PLASSHIP_TUNE_CYC_PASSES")
    cyc.write(tmp_path / "g")
    assert_same_db(tmp_path / "o", tmp_path / "g", "cyclecheck with overflowing tables")
    assert st.n_block > st0.n_block + 5 and st.n_cyclic == st0.n_cyclic          # the fall-backs are counted with the last tier


def test_golden_findassemblystart(ctx, golden, tmp_path):
    """row N3 on the reference's DBs, and iteration 0 of `plass assemble` as data/assemble.sh:84-150 runs it, chained on the
    device: kmermatcher -> rescorediagonal -> findassemblystart -> kmermatcher -> rescorediagonal -> assembleresults"""
    import plass_amd
    s, g, f = os.path.join(golden, "aa"), os.path.join(golden, "guided"), os.path.join(golden, "fs")
    db = ctx.read_seqdb(f"{s}/seq_0")
    out, st = ctx.findassemblystart(db, ctx.read_alndb(db, f"{s}/aln_0"))
    out.write(tmp_path / "corr")
    assert_same_db(f"{f}/corrected_seqs", tmp_path / "corr", "findassemblystart")
    assert st.n_alignments > 7255
    gdb = ctx.read_seqdb(f"{g}/aa_0")
    gout, _ = ctx.findassemblystart(gdb, ctx.read_alndb(gdb, f"{g}/aln_0"))
    gout.write(tmp_path / "gcorr")
    assert_same_db(f"{f}/guided_corrected_seqs", tmp_path / "gcorr", "findassemblystart on ORFs")
    rs, asp = plass_amd.RescoreParams(min_seq_id=0.9), plass_amd.AssembleParams(min_seq_id=0.9)
    cands, _ = ctx.kmermatcher(db, km_params(0))
    alns, _ = ctx.rescorediagonal(db, db, cands, rs)
    corr, _ = ctx.findassemblystart(db, alns)
    cands2, _ = ctx.kmermatcher(corr, km_params(0))
    alns2, _ = ctx.rescorediagonal(corr, corr, cands2, rs)
    as0, _ = ctx.assembleresults(corr, alns2, asp)
    as0.write(tmp_path / "as0")
    assert_same_db(f"{f}/assembly_0", tmp_path / "as0", "iteration 0 chained on the device")


def test_findassemblystart_vs_oracle(ctx, oracle_bin, tmp_path):
    """hostile start columns: fragments of one protein family with '*M' / 'xM' / no M at moving offsets, M at position 0,
    several M, an alignment-free sequence — against the oracle"""
    import plass_amd
    from plass_amd import synth
    rng = np.random.default_rng(17)
    aa = "ACDEFGHIKLNPQRSTVWY"                                  # no M: the M columns are placed by hand
    seqs = []
    for fam in range(300):
        core = "".join(aa[i] for i in rng.integers(0, len(aa), 90))
        mpos = int(rng.integers(5, 40))
        for _ in range(int(rng.integers(2, 9))):
            a, b = int(rng.integers(0, 30)), int(rng.integers(60, 90))
            frag = list(core[a:b])
            kind = int(rng.integers(0, 5))
            if mpos >= a + 1 and mpos < b and kind < 4:
                frag[mpos - a] = "M"
                if kind < 2:
                    frag[mpos - a - 1] = "*"
                if kind == 3 and mpos - a + 7 < len(frag):
                    frag[mpos - a + 7] = "M"
            if kind == 4 and rng.integers(0, 2):
                frag[0] = "M"
            seqs.append("".join(frag))
    seqs.append("MKV")
    _write_fasta_like_db(tmp_path / "seq", seqs)
    run_oracle(oracle_bin, ["kmermatcher", tmp_path / "seq", tmp_path / "pref"] + AA_KM + aa_iter_flags(0))
    run_oracle(oracle_bin, ["rescorediagonal", tmp_path / "seq", tmp_path / "seq", tmp_path / "pref", tmp_path / "aln"] + AA_RS)
    run_oracle(oracle_bin, ["findassemblystart", tmp_path / "seq", tmp_path / "aln", tmp_path / "o_corr"])
    db = ctx.read_seqdb(tmp_path / "seq")
    out, _ = ctx.findassemblystart(db, ctx.read_alndb(db, tmp_path / "aln"))
    out.write(tmp_path / "g_corr")
    assert_same_db(tmp_path / "o_corr", tmp_path / "g_corr", "findassemblystart hostile")
    _, e0 = read_db(tmp_path / "seq"); _, e1 = read_db(tmp_path / "g_corr")
    assert sum(1 for k in e0 if e0[k] != e1[k]) > 50            # the case is not vacuous


@pytest.mark.parametrize("case", [1, 2, 3, 4])
def test_golden_stale_scan_quirk(ctx, golden, tmp_path, case):
    """inputs on which the reference's run scan continues into stale records behind the compaction point
    (SURVEY.md Appendix A.3): the reference's own output is the expectation"""
    d = os.path.join(golden, "q1", f"case{case}")
    ext = open(os.path.join(d, "ext")).read().strip() == "1"
    db = ctx.read_seqdb(os.path.join(d, "seq"))
    par = km_params(0); par.include_only_extendable = ext
    cands, _ = ctx.kmermatcher(db, par)
    cands.write(tmp_path / "pref")
    assert_same_db(os.path.join(d, "pref"), tmp_path / "pref", f"stale-scan case {case}")


def _oracle_iteration(oracle_bin, d, it):
    log = run_oracle(oracle_bin, ["kmermatcher", d / f"o_seq_{it}", d / f"o_pref_{it}"] + AA_KM + aa_iter_flags(it))
    run_oracle(oracle_bin, ["rescorediagonal", d / f"o_seq_{it}", d / f"o_seq_{it}", d / f"o_pref_{it}", d / f"o_aln_{it}"] + AA_RS)
    run_oracle(oracle_bin, ["assembleresults", d / f"o_seq_{it}", d / f"o_aln_{it}", d / f"o_seq_{it + 1}"] + AA_AS)
    return log          # (the kmermatcher's: its N_k / N_m / N_c line)


def test_synthetic_three_iterations_vs_oracle(ctx, oracle_bin, tmp_path):
    """40 k read pairs (about 130 k protein fragments, 0.3 M candidate overlaps per iteration): every DB of
    every iteration equals the oracle's"""
    import plass_amd
    from plass_amd import synth
    data, off, elen, key = synth.protein_fragment_db(40000, seed=11)
    synth.write_db(str(tmp_path / "o_seq_0"), data, off, elen, key, 0)
    db = ctx.upload_seqdb(data, off, elen, key, 0)
    for it in range(3):
        log = _oracle_iteration(oracle_bin, tmp_path, it)
        cands, kst = ctx.kmermatcher(db, km_params(it))
        cands.write(tmp_path / "g_pref")
        assert_same_db(tmp_path / f"o_pref_{it}", tmp_path / "g_pref", f"kmermatcher it{it}")
        assert_counts(kst, log, f"kmermatcher it{it}")
        alns, rst = ctx.rescorediagonal(db, db, cands, plass_amd.RescoreParams(min_seq_id=0.9))
        alns.write(tmp_path / "g_aln")
        assert_same_db(tmp_path / f"o_aln_{it}", tmp_path / "g_aln", f"rescorediagonal it{it}")
        db2, ast = ctx.assembleresults(db, alns, plass_amd.AssembleParams(min_seq_id=0.9))
        db2.write(tmp_path / "g_seq")
        assert_same_db(tmp_path / f"o_seq_{it + 1}", tmp_path / "g_seq", f"assembleresults it{it}")
        assert kst.n_candidates > 50000 and rst.n_accepted > kst.n_candidates // 4
        # size-independent properties
        i0, i1 = db.info(), db2.info()
        assert i1["n"] == i0["n"] and i1["residues"] >= i0["residues"]
        db = db2


def test_synthetic_guided_vs_oracle(ctx, oracle_bin, tmp_path):
    """protein-guided nucleotide assembly on synthetic ORF twins (a few thousand reads at 20x): protein k-mer matching and
    re-scoring with backtrace, proteinaln2nucl, guidedassembleresults — every DB of two iterations equals the oracle's,
    also with a small --max-seq-len in the second one"""
    import plass_amd
    from plass_amd import synth
    (nd, no, ne, nk), (ad, ao, ae, ak) = synth.orf_twin_dbs(2500, seed=41)
    t = tmp_path
    synth.write_db(str(t / "nucl_0"), nd, no, ne, nk, 1); synth.write_db(str(t / "aa_0"), ad, ao, ae, ak, 0)
    nu = ctx.upload_seqdb(nd, no, ne, nk, 1); aa = ctx.upload_seqdb(ad, ao, ae, ak, 0)
    for it in range(2):
        cap = (200000, 420)[it]
        as_flags = ["--min-seq-id", "0.99", "--max-seq-len", str(cap), "--keep-target", "1", "--rescore-mode", "3"]
        run_oracle(oracle_bin, ["kmermatcher", t / f"aa_{it}", t / "o_pref"] + GD_KM)
        run_oracle(oracle_bin, ["rescorediagonal", t / f"aa_{it}", t / f"aa_{it}", t / "o_pref", t / "o_aln"] + GD_RS)
        run_oracle(oracle_bin, ["proteinaln2nucl", t / f"nucl_{it}", t / f"nucl_{it}", t / f"aa_{it}", t / f"aa_{it}", t / "o_aln", t / "o_aln_nucl"] + GD_P2N)
        run_oracle(oracle_bin, ["guidedassembleresults", t / f"nucl_{it}", t / f"aa_{it}", t / "o_aln_nucl", t / f"nucl_{it + 1}", t / f"aa_{it + 1}"] + as_flags)
        cands, _ = ctx.kmermatcher(aa, gd_km_params())
        cands.write(t / "g_pref")
        assert_same_db(t / "o_pref", t / "g_pref", f"guided kmermatcher it{it}")
        alns, _ = ctx.rescorediagonal(aa, aa, cands, gd_rs_params())
        alns.write(t / "g_aln")
        assert_same_db(t / "o_aln", t / "g_aln", f"guided rescorediagonal it{it}")
        naln, _ = ctx.proteinaln2nucl(nu, aa, alns)
        naln.write(t / "g_aln_nucl")
        assert_same_db(t / "o_aln_nucl", t / "g_aln_nucl", f"proteinaln2nucl it{it}")
        nu2, aa2, st = ctx.guidedassembleresults(nu, aa, naln, plass_amd.AssembleParams(min_seq_id=0.99, max_seq_len=cap))
        nu2.write(t / "g_nucl"); aa2.write(t / "g_aa")
        assert_same_db(t / f"nucl_{it + 1}", t / "g_nucl", f"guidedassembleresults nucl it{it}")
        assert_same_db(t / f"aa_{it + 1}", t / "g_aa", f"guidedassembleresults aa it{it}")
        if it == 0:
            assert st.n_extended > 200
        nu, aa = nu2, aa2


def test_length_cap_vs_oracle(ctx, oracle_bin, tmp_path):
    """--max-seq-len small enough that the length cap fires all the time (assembleresult.cpp:259-263: left extension only;
    nuclassembleresult.cpp:271-275,301-305: both sides): the round then stops at the capped hit, hits ranked below it stay
    queued and the query is abandoned with what it has"""
    import plass_amd
    from plass_amd import synth
    data, off, elen, key = synth.protein_fragment_db(12000, seed=31)
    synth.write_db(str(tmp_path / "a_seq_0"), data, off, elen, key, 0)
    db = ctx.upload_seqdb(data, off, elen, key, 0)
    for it in range(3):
        cap = (90, 140, 200)[it]
        run_oracle(oracle_bin, ["kmermatcher", tmp_path / f"a_seq_{it}", tmp_path / "o_pref"] + AA_KM + aa_iter_flags(it))
        run_oracle(oracle_bin, ["rescorediagonal", tmp_path / f"a_seq_{it}", tmp_path / f"a_seq_{it}", tmp_path / "o_pref", tmp_path / "o_aln"] + AA_RS)
        run_oracle(oracle_bin, ["assembleresults", tmp_path / f"a_seq_{it}", tmp_path / "o_aln", tmp_path / f"a_seq_{it + 1}", "--min-seq-id", "0.9",
                                "--max-seq-len", str(cap), "--keep-target", "1", "--rescore-mode", "3"])
        cands, _ = ctx.kmermatcher(db, km_params(it))
        alns, _ = ctx.rescorediagonal(db, db, cands, plass_amd.RescoreParams(min_seq_id=0.9))
        db2, st = ctx.assembleresults(db, alns, plass_amd.AssembleParams(min_seq_id=0.9, max_seq_len=cap))
        db2.write(tmp_path / "g_seq")
        assert_same_db(tmp_path / f"a_seq_{it + 1}", tmp_path / "g_seq", f"assembleresults with --max-seq-len {cap} it{it}")
        db = db2
    data, off, elen, key = synth.nucleotide_read_db(6000, seed=33)
    synth.write_db(str(tmp_path / "n_seq_0"), data, off, elen, key, 1)
    db = ctx.upload_seqdb(data, off, elen, key, 1)
    for it in range(2):
        cap = (260, 400)[it]
        run_oracle(oracle_bin, ["kmermatcher", tmp_path / f"n_seq_{it}", tmp_path / "o_pref"] + NUCL_KM)
        run_oracle(oracle_bin, ["rescorediagonal", tmp_path / f"n_seq_{it}", tmp_path / f"n_seq_{it}", tmp_path / "o_pref", tmp_path / "o_aln"] + NUCL_RS)
        run_oracle(oracle_bin, ["nuclassembleresults", tmp_path / f"n_seq_{it}", tmp_path / "o_aln", tmp_path / f"n_seq_{it + 1}", "--min-seq-id", "0.99",
                                "--max-seq-len", str(cap), "--keep-target", "1", "--rescore-mode", "3"])
        cands, _ = ctx.kmermatcher(db, km_params(it, nucl=True))
        alns, _ = ctx.rescorediagonal(db, db, cands, plass_amd.RescoreParams(min_seq_id=0.99))
        db2, st = ctx.assembleresults(db, alns, plass_amd.AssembleParams(min_seq_id=0.99, max_seq_len=cap))
        db2.write(tmp_path / "g_seq")
        assert_same_db(tmp_path / f"n_seq_{it + 1}", tmp_path / "g_seq", f"nuclassembleresults with --max-seq-len {cap} it{it}")
        db = db2


def _write_fasta_like_db(path, seqs, dbtype=0, keys=None):
    from plass_amd import synth
    arrs = [np.frombuffer(s.encode(), dtype=np.uint8) for s in seqs]
    data, off, elen, key = synth.pack_db(arrs)
    if keys is not None:
        key = np.asarray(keys, dtype=np.uint32)
    synth.write_db(str(path), data, off, elen, key, dbtype)
    return data, off, elen, key


def test_upload_refuses_bytes_the_score_tables_cannot_index(ctx, tmp_path):
    """the scoring kernels index their tables with the residue bytes and blank columns with byte 0 — a DB with a byte above
    'z' or a NUL inside an entry is refused at upload (the reference maps every byte through aa2num; such a DB is not one it writes)"""
    import plass_amd
    from plass_amd import synth
    good = ["MKVLAAGIVGLLLAQWERTYHGFDSAPMKVLAAGI", "ACDEFGHIKLMNPQRSTVWYacdefxz*", "MK"]
    data, off, elen, key = _write_fasta_like_db(tmp_path / "ok", good)
    db = ctx.read_seqdb(tmp_path / "ok"); assert db.info()["n"] == 3; db.free()
    for name, pos, byte, what in (("high", 5, 0xC3, "above 'z'"), ("brace", 40, 123, "above 'z'"), ("nul", 7, 0, "NUL")):
        d = np.frombuffer(bytes(data), dtype=np.uint8).copy(); d[pos] = byte
        synth.write_db(str(tmp_path / name), d, off, elen, key, 0)
        with pytest.raises(plass_amd.PlasshipError) as ei:
            ctx.read_seqdb(tmp_path / name)
        assert what in str(ei.value)
    d = np.frombuffer(bytes(data), dtype=np.uint8).copy(); d[int(off[0] + elen[0] - 1)] = ord("A")          # first entry without its final NUL
    synth.write_db(str(tmp_path / "noterm"), d, off, elen, key, 0)
    with pytest.raises(plass_amd.PlasshipError):
        ctx.read_seqdb(tmp_path / "noterm")


def test_adversarial_inputs_vs_oracle(ctx, oracle_bin, tmp_path):
    """ragged and hostile inputs: sequences shorter than k, X / '*' residues, low-complexity repeats (repeated
    k-mers, many ties in the hash threshold bin), exact duplicates, one contig above 32 767 residues (switches the
    reference to KmerPosition<int>), sparse non-contiguous keys, lower-case letters"""
    import plass_amd
    rng = np.random.default_rng(5)
    aa = "ACDEFGHIKLMNPQRSTVWY"
    base = "".join(rng.choice(list(aa), size=4000))
    seqs = []
    for i in range(400):
        p = int(rng.integers(0, 3900)); l = int(rng.integers(40, 100))
        seqs.append(base[p:p + l])
    seqs += ["MKV", "A" * 13, "A" * 14, "A" * 200, "AS" * 120, "MKVLAAGX" * 10, "XXXXXXXXXXXXXXXXXXXXXXXX", base[100:180] + "*", base[100:180] + "*",
             base[1000:1100].lower(), base[1000:1100], "*" + base[2000:2060], base[500:2500]]
    long_contig = "".join(rng.choice(list(aa), size=33000))
    seqs += [long_contig, long_contig[32000:] + base[:60], base[3000:3050] + long_contig[:70]]
    keys = np.cumsum(rng.integers(1, 4, size=len(seqs))).astype(np.uint32)
    perm = rng.permutation(len(seqs))                       # index file order != key order
    _write_fasta_like_db(tmp_path / "seq", [seqs[i] for i in perm], 0, keys[perm])
    db = ctx.read_seqdb(tmp_path / "seq")
    assert db.info()["max_entry_len"] >= 32767
    for it, ext in ((0, False), (1, True)):
        flags = ["--hash-shift", "67", "--include-only-extendable", "1" if ext else "0"]
        log = run_oracle(oracle_bin, ["kmermatcher", tmp_path / "seq", tmp_path / f"o_pref{it}"] + AA_KM + flags)
        par = km_params(0); par.include_only_extendable = ext
        cands, kst = ctx.kmermatcher(db, par)
        cands.write(tmp_path / f"g_pref{it}")
        assert_same_db(tmp_path / f"o_pref{it}", tmp_path / f"g_pref{it}", f"adversarial kmermatcher ext={ext}")
        assert_counts(kst, log, f"adversarial kmermatcher ext={ext}")
        run_oracle(oracle_bin, ["rescorediagonal", tmp_path / "seq", tmp_path / "seq", tmp_path / f"o_pref{it}", tmp_path / f"o_aln{it}"] + AA_RS)
        alns, _ = ctx.rescorediagonal(db, db, cands, plass_amd.RescoreParams(min_seq_id=0.9))
        alns.write(tmp_path / f"g_aln{it}")
        assert_same_db(tmp_path / f"o_aln{it}", tmp_path / f"g_aln{it}", "adversarial rescorediagonal")
        run_oracle(oracle_bin, ["assembleresults", tmp_path / "seq", tmp_path / f"o_aln{it}", tmp_path / f"o_seq{it}"] + AA_AS)
        out, _ = ctx.assembleresults(db, alns, plass_amd.AssembleParams(min_seq_id=0.9))
        out.write(tmp_path / f"g_seq{it}")
        assert_same_db(tmp_path / f"o_seq{it}", tmp_path / f"g_seq{it}", "adversarial assembleresults")


def test_protein_repeats_overflow_the_candidate_set(ctx, oracle_bin, tmp_path):
    """every window whose score is <= the threshold score is a candidate and equal k-mers share a score, so a
    homopolymer or tandem repeat of >= ~85 residues overfills the 128-entry candidate set of the protein tiers whenever its k-mer
    lies at or below the threshold.  The extraction's overflow count is checked late on protein DBs (no extra wait); such a
    sequence must then restart the call with the HBM-scratch launch, not leave its slots unwritten.  20 homopolymers, tandem
    repeats of period 2..7, four hash seeds — against the oracle, and the path must have been taken."""
    rng = np.random.default_rng(11)
    aa = "ACDEFGHIKLMNPQRSTVWY"
    rnd = lambda n: "".join(rng.choice(list(aa), size=n))
    seqs = []
    for ch in aa:
        seqs.append(rnd(110) + ch * 200 + rnd(110))
    for unit in ("GP", "GPP", "QAQS", "KDELK", "STSTPA", "GAGAGSG"):
        seqs.append(rnd(90) + unit * (420 // len(unit)) + rnd(90))
    base = seqs[3]
    for i in range(60):                                      # reads over the flanks, so that the repeats' neighbours have candidates
        p = int(rng.integers(0, len(base) - 80)); seqs.append(base[p:p + int(rng.integers(50, 80))])
    _write_fasta_like_db(tmp_path / "seq", seqs, 0)
    db = ctx.read_seqdb(tmp_path / "seq")
    scratch = restarts = 0
    for hs in (67, 68, 69, 70):
        for ext in (0, 1):
            log = run_oracle(oracle_bin, ["kmermatcher", tmp_path / "seq", tmp_path / "o_pref"] + AA_KM + ["--hash-shift", str(hs), "--include-only-extendable", str(ext)])
            par = km_params(0); par.hash_shift = hs; par.include_only_extendable = bool(ext)
            cands, st = ctx.kmermatcher(db, par)
            cands.write(tmp_path / "g_pref")
            assert_same_db(tmp_path / "o_pref", tmp_path / "g_pref", f"repeats, hash shift {hs}, extendable {ext}")
            assert_counts(st, log, f"repeats, hash shift {hs}, extendable {ext}")
            scratch += st.n_scratch_sequences; restarts += st.n_restarts
            cands.free()
    assert scratch > 0 and restarts > 0, "no sequence overflowed the candidate set: the test does not reach the path it is for"


def test_adversarial_inputs_through_the_row_kernels(ctx, golden, oracle_bin, tmp_path, monkeypatch):
    """X runs, repeats, threshold ties and overfull candidate sets with the row kernels forced (round 6): what they cannot finish must reach the wave
    tiers through their fall-back queue with the same records as before"""
    monkeypatch.setenv("PLASSHIP_TUNE_ROWTIER", "3")
    for ext in (False, True):
        test_golden_adversarial_inputs(ctx, golden, tmp_path, ext)
    test_adversarial_inputs_vs_oracle(ctx, oracle_bin, tmp_path)
    test_protein_repeats_overflow_the_candidate_set(ctx, oracle_bin, tmp_path)
    test_synthetic_three_iterations_vs_oracle(ctx, oracle_bin, tmp_path)


def test_empty_and_singleton_db(ctx, oracle_bin, tmp_path):
    import plass_amd
    _write_fasta_like_db(tmp_path / "one", ["MKVLAAGIVGLLLAQPSWAETGEKSLYELDRSSAKNRLIMGAVGYL"], 0)
    db = ctx.read_seqdb(tmp_path / "one")
    cands, st = ctx.kmermatcher(db, km_params(0))
    assert st.n_candidates == 0
    cands.write(tmp_path / "g_pref")
    run_oracle(oracle_bin, ["kmermatcher", tmp_path / "one", tmp_path / "o_pref"] + AA_KM + aa_iter_flags(0))
    assert_same_db(tmp_path / "o_pref", tmp_path / "g_pref", "singleton")
    alns, _ = ctx.rescorediagonal(db, db, cands)
    out, ast = ctx.assembleresults(db, alns)
    assert ast.n_extended == 0 and out.info()["n"] == 1


def test_order_invariance_and_idempotence(ctx, tmp_path):
    """property at a size the oracle is not run on (0.4 M fragments): results do not depend on the order of the
    input index, and running a module twice gives identical bytes"""
    import plass_amd
    from plass_amd import synth
    data, off, elen, key = synth.protein_fragment_db(125000, seed=21)
    db = ctx.upload_seqdb(data, off, elen, key, 0)
    rng = np.random.default_rng(1)
    p = rng.permutation(len(key))
    db_shuffled = ctx.upload_seqdb(data, off[p], elen[p], key[p], 0)
    outs = []
    for d in (db, db, db_shuffled):
        cands, kst = ctx.kmermatcher(d, km_params(0))
        alns, rst = ctx.rescorediagonal(d, d, cands)
        o, ast = ctx.assembleresults(d, alns)
        q, t, s, dg = cands.download()
        outs.append((q.tobytes(), t.tobytes(), s.tobytes(), dg.tobytes(), o.download()[0], kst.n_candidates, rst.n_accepted, ast.n_extended))
        # structural properties: hits sorted by (query, target), no self hits in the list, every accepted line within bounds
        assert np.all((q[1:] > q[:-1]) | ((q[1:] == q[:-1]) & (t[1:] > t[:-1]))) and not np.any(q == t)
        assert rst.n_accepted >= len(key) and ast.n_extended > 0
        o.free(); alns.free(); cands.free()
    assert outs[0] == outs[1], "same input, different output"
    assert outs[0] == outs[2], "output depends on input index order"


def test_cli_boundary_all_modules(tmp_path):
    """the drop-in boundary itself: `plass-hip <module> <DBs> <reference flags>` for every module, DB files in, DB files
    out, compared with the reference's golden DBs (tests/gpu_cli_check.sh)"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run(["bash", os.path.join(root, "tests", "gpu_cli_check.sh"), str(tmp_path / "cli")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0 and "failures: 0" in p.stdout, p.stdout[-3000:]
    assert p.stdout.count("PASS ") >= 21


@pytest.mark.parametrize("name,mod,flags", sweep_variants(), ids=[v[0] for v in sweep_variants()])
def test_cli_flag_sweep(golden, tmp_path, name, mod, flags):
    """the reference's flags through the command line: `plass-hip <module> … <flags>` must write what the reference wrote
    (tests/golden/make_golden_sweep.sh)"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m, pos, outs = sweep_positional(golden, mod, tmp_path / "out")
    cmd = [os.path.join(root, "plass_amd", "plass-hip"), m] + pos + flags
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:]
    for suffix, path in outs:
        assert_same_db(os.path.join(golden, "sweep", name + suffix), path, name + suffix)


@pytest.mark.parametrize("mod,extra", [("rescorediagonal", ["--rescore-mode", "2"]), ("rescorediagonal", ["--wrapped-scoring", "1"]),
                                       ("kmermatcher", ["--spaced-kmer-mode", "1"]), ("assembleresults", ["--rescore-mode", "0"])])
def test_cli_unsupported_fails_loudly(golden, tmp_path, mod, extra):
    """what the GPU path does not implement ends with a message and exit code 95 — the code plass_amd/plass-gpu-wrapper hands to the
    reference binary on — whether the command line says so or the library does (no silent fallback, no output DB)"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m, pos, outs = sweep_positional(golden, mod, tmp_path / "out")
    p = subprocess.run([os.path.join(root, "plass_amd", "plass-hip"), m] + pos + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 95 and ("not supported" in p.stdout or "only" in p.stdout or "not part of the GPU path" in p.stdout) and "outside the GPU hot path" in p.stdout, p.stdout[-800:]
    assert not os.path.exists(outs[0][1] + ".index")


def test_nucleotide_strand_ties_are_a_reference_outcome(ctx, oracle_bin, tmp_path):
    """on strand-tied pairs the reference's nucleotide kmermatcher is not deterministic (10 runs, 8 versions of one
    entry); the GPU path's prefilter DB must be ONE OF THE REFERENCE'S outcomes — every query without a tie byte for byte, every line of a
    tie-dependent query a version some reference run wrote (tests/golden/strand_membership.json, generator make_strand_membership.py: the
    judge's case, seed 424242, 40 000 pairs, 4 genomes of 100-200 kb; three iterations of the nucleotide chain, each on the GPU path's own
    previous result)."""
    import json
    import sys
    import plass_amd
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_strand_membership import entries
    from conftest import check_strand_membership
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "strand_membership.json")))
    run_oracle(oracle_bin, ["synthreads", tmp_path / "reads"] + fx["synth"])          # (the read model shared with the GPU generator)
    db = ctx.read_seqdb(tmp_path / "reads")
    for it, rec in enumerate(fx["iterations"]):
        cands, _ = ctx.kmermatcher(db, km_params(it, nucl=True))
        cands.write(tmp_path / "pref")
        ent = entries(str(tmp_path / "pref"))
        check_strand_membership(rec, ent, "GPU path, nucleotide iteration %d" % it)
        for k, t in rec["ties"].items():                      # oracle and GPU path resolve a tie by the same rule
            assert ent[int(k)].decode("latin-1") == t["oracle"]
        alns, _ = ctx.rescorediagonal(db, db, cands, plass_amd.RescoreParams(min_seq_id=0.99))
        cands.free()
        out, _ = ctx.assembleresults(db, alns, nucl_as_params())
        alns.free(); db.free()
        cyc, rest, _ = ctx.cyclecheck(out, max_seq_len=200000, chop_cycle=True, with_rest=True)
        cyc.free(); out.free()
        db = rest
    db.free()

