"""Sort #2 with one wavefront per bucket (aggSortWaveKernel) and its fall-back to the block kernel (aggSortKernel over the overflow
list): the same golden and oracle cases as test_gpu_parity / test_gpu_sharded, run with the wave path (default), the block kernel on
every bucket (PLASSHIP_TUNE_AGGWAVE=2) and the wave path with tiny caps (PLASSHIP_TUNE_AGGWAVE_CAP: most buckets overflow to the block
kernel).  Every mode must write the reference's bytes."""
import os
import re

import numpy as np
import pytest

from conftest import AA_KM, assert_same_db, run_oracle
import test_gpu_parity as P
import test_gpu_sharded as S

pytestmark = pytest.mark.gpu

MODES = {"wave": {}, "block": {"PLASSHIP_TUNE_AGGWAVE": "2"}, "tinycaps": {"PLASSHIP_TUNE_AGGWAVE_CAP": "24"}}


@pytest.fixture(params=sorted(MODES))
def mode(request, monkeypatch):
    for k in ("PLASSHIP_TUNE_AGGWAVE", "PLASSHIP_TUNE_AGGWAVE_CAP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in MODES[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


@pytest.fixture(scope="module")
def ctx():
    import plass_amd
    c = plass_amd.Context(0)
    yield c
    c.close()


ctxs = S.ctxs


def test_golden_protein_modules(ctx, golden, tmp_path, mode):
    for it in (0, 1, 2):
        P.test_golden_aa_modules(ctx, golden, tmp_path, it)
    P.test_golden_aa_chained_on_device(ctx, golden, tmp_path)


def test_golden_nucleotide_modules(ctx, golden, tmp_path, mode):
    for it in (0, 1):
        P.test_golden_nucl_kmermatcher_rescore(ctx, golden, tmp_path, it)
        P.test_golden_long_nucleotide_contigs(ctx, golden, tmp_path, it)
    P.test_golden_nucl_chained_on_device(ctx, golden, tmp_path)


def test_golden_stale_scan_quirk_cases(ctx, golden, tmp_path, mode):
    for case in (1, 2, 3, 4):
        P.test_golden_stale_scan_quirk(ctx, golden, tmp_path, case)


def test_golden_strand_ties(ctx, golden, tmp_path, mode):
    P.test_golden_nucleotide_strand_ties(ctx, golden, tmp_path)


def test_adversarial_inputs(ctx, golden, oracle_bin, tmp_path, mode):
    for ext in (False, True):
        P.test_golden_adversarial_inputs(ctx, golden, tmp_path, ext)
    P.test_adversarial_inputs_vs_oracle(ctx, oracle_bin, tmp_path)


def test_sharded_nucleotide_chain(ctxs, golden, tmp_path, mode, monkeypatch):
    """owner side of a sharded run: weighted triples (TripleX) merged, rank words carried (ORDOUT)"""
    monkeypatch.setenv("PLASSHIP_TUNE_SHARD_EXTRACT", "1")
    S.test_sharded_golden_nucl_chained(ctxs, golden, tmp_path)
    S.test_sharded_stale_scan_quirk(ctxs, golden, tmp_path, 2)


def test_hot_representative_takes_the_fallback(ctx, oracle_bin, tmp_path, mode, capfd, monkeypatch):
    """one long sequence is the representative of ~1000 fragments on distinct diagonals: its bucket holds more distinct keys than a
    wavefront sorts (AW_CAP = 512), so even the default caps send it to the block kernel; the candidates must equal the oracle's"""
    import plass_amd
    rng = np.random.default_rng(17)
    aa = list("ACDEFGHIKLMNPQRSTVWY")
    base = "".join(rng.choice(aa, size=8000))
    seqs = [base]
    for _ in range(3000):
        p = int(rng.integers(0, 7900)); n = int(rng.integers(50, 100))
        seqs.append(base[p:p + n])
    P._write_fasta_like_db(tmp_path / "seq", seqs, 0)
    db = ctx.read_seqdb(tmp_path / "seq")
    monkeypatch.setenv("PLASSHIP_DEBUG_AGGHIST", "1")
    capfd.readouterr()
    for it, ext in ((0, False), (1, True)):
        par = P.km_params(0); par.include_only_extendable = ext
        cands, st = ctx.kmermatcher(db, par)
        cands.write(tmp_path / f"g_pref{it}")
        run_oracle(oracle_bin, ["kmermatcher", tmp_path / "seq", tmp_path / f"o_pref{it}"] + AA_KM + ["--hash-shift", "67", "--include-only-extendable", "1" if ext else "0"])
        assert_same_db(tmp_path / f"o_pref{it}", tmp_path / f"g_pref{it}", f"hot representative, ext={ext}, mode {mode}")
    err = capfd.readouterr().err
    maxima = [int(m) for m in re.findall(r"distinct .*\(mean \d+, max (\d+)", err)]
    assert maxima and max(maxima) > 512, err
