"""assembleresults for queries of more than 64 alignments: the on-chip queue kernel (assembleQueueKernel, queues of up to 128 and up to
256 alignments in LDS) and its fall-back to the HBM-resident queue (assembleBigKernel over the overflow list).  The golden and oracle
protein cases of test_gpu_parity / test_gpu_sharded and a high-coverage synthetic case run with the on-chip queues (default), the HBM
queue for every such query (PLASSHIP_TUNE_ASMQ=2) and a tiny on-chip cap (PLASSHIP_TUNE_ASMQ_CAP: most queries overflow to the HBM
queue).  Every mode must write the reference's bytes."""
import re

import numpy as np
import pytest

from conftest import AA_AS, AA_KM, AA_RS, assert_same_db, run_oracle
import test_gpu_parity as P
import test_gpu_sharded as S

pytestmark = pytest.mark.gpu

MODES = {"onchip": {}, "hbm": {"PLASSHIP_TUNE_ASMQ": "2"}, "tinycap": {"PLASSHIP_TUNE_ASMQ_CAP": "80"}}


@pytest.fixture(params=sorted(MODES))
def mode(request, monkeypatch):
    for k in ("PLASSHIP_TUNE_ASMQ", "PLASSHIP_TUNE_ASMQ_CAP"):
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
    P.test_golden_aa_keep_target0(ctx, golden, tmp_path)


def test_adversarial_inputs(ctx, golden, oracle_bin, tmp_path, mode):
    for ext in (False, True):
        P.test_golden_adversarial_inputs(ctx, golden, tmp_path, ext)
    P.test_adversarial_inputs_vs_oracle(ctx, oracle_bin, tmp_path)


def test_sharded_protein_chain(ctxs, golden, tmp_path, mode):
    S.test_sharded_golden_aa_chained(ctxs, golden, tmp_path, 2)


@pytest.mark.parametrize("max_seq_len", [65535, 400])
def test_high_coverage_queues(ctx, oracle_bin, tmp_path, mode, capfd, monkeypatch, max_seq_len):
    """one short genome at high depth: many fragments align to more than 64 others and some to more than 128, so both queue kernels run
    (and the fall-back in the tiny-cap mode); with --max-seq-len 400 the extensions end at the length cap (the hits ranked below the left
    hit stay queued)"""
    import plass_amd
    rng = np.random.default_rng(23)
    aa = list("ACDEFGHIKLMNPQRSTVWY")
    base = "".join(rng.choice(aa, size=1500))
    seqs = []
    for _ in range(3000):
        p = int(rng.integers(0, 1450)); n = int(rng.integers(40, 110))
        seqs.append(base[p:p + n])
    P._write_fasta_like_db(tmp_path / "seq", seqs, 0)
    db = ctx.read_seqdb(tmp_path / "seq")
    monkeypatch.setenv("PLASSHIP_DEBUG_ASMHIST", "1")
    capfd.readouterr()
    par = P.km_params(0)
    cands, _ = ctx.kmermatcher(db, par)
    cands.write(tmp_path / "g_pref")
    run_oracle(oracle_bin, ["kmermatcher", tmp_path / "seq", tmp_path / "o_pref"] + AA_KM + ["--hash-shift", "67", "--include-only-extendable", "0"])
    assert_same_db(tmp_path / "o_pref", tmp_path / "g_pref", "high coverage kmermatcher")
    run_oracle(oracle_bin, ["rescorediagonal", tmp_path / "seq", tmp_path / "seq", tmp_path / "o_pref", tmp_path / "o_aln"] + AA_RS)
    alns, _ = ctx.rescorediagonal(db, db, cands, plass_amd.RescoreParams(min_seq_id=0.9))
    alns.write(tmp_path / "g_aln")
    assert_same_db(tmp_path / "o_aln", tmp_path / "g_aln", "high coverage rescorediagonal")
    flags = [x if x != "65535" else str(max_seq_len) for x in AA_AS]
    run_oracle(oracle_bin, ["assembleresults", tmp_path / "seq", tmp_path / "o_aln", tmp_path / "o_seq"] + flags)
    out, st = ctx.assembleresults(db, alns, plass_amd.AssembleParams(min_seq_id=0.9, max_seq_len=max_seq_len))
    out.write(tmp_path / "g_seq")
    assert_same_db(tmp_path / "o_seq", tmp_path / "g_seq", f"high coverage assembleresults, mode {mode}, max-seq-len {max_seq_len}")
    assert st.tier_alignments[2] > 0                       # alignments of the queries with more than 64
    err = capfd.readouterr().err
    m = re.findall(r"asmHist call \d+ big queries (\d+) \(max h (\d+), over cap (\d+): (\d+)\)", err)
    assert m, err
    nbig, maxh, cap, over = (int(x) for x in m[-1])
    assert nbig > 100 and maxh > 128, err
    if mode == "tinycap":
        assert cap == 80 and over > nbig // 2, err
