"""GPU tests of `plass-hip assemble-chain / nuclassemble-chain --write-intermediate DIR --resume 1` (`-m gpu`): a run that is interrupted and
started again with the same command — or extended with a larger --num-iterations — writes the bytes an uninterrupted run writes.  Every
comparison is byte for byte on the data, `.index` and `.dbtype` files (and on the FASTA / `_cycle.index` files of the tails).

Run A is the uninterrupted run, B1 the interrupted one (fewer iterations, same DIR), B2 its continuation.  A run without --resume keeps the last
iteration's DB out of DIR (it is the positional output), so A's `assembly_<last>` is A's output DB."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, assert_same_db

pytestmark = pytest.mark.gpu
HIP = os.path.join(ROOT, "plass_amd", "plass-hip")
DB_SUFFIXES = ("", ".index", ".dbtype")


def hip(args, ok=0, env=None):
    e = dict(os.environ); e.pop("PLASSHIP_CLI_DRYRUN", None); e.update(env or {})
    p = subprocess.run([HIP] + [str(a) for a in args], env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == ok, p.stdout[-3000:]
    assert ("Time for processing" in p.stdout) == (ok == 0), p.stdout[-3000:]
    return p.stdout


def same_files(a, b, suffixes=DB_SUFFIXES):
    for s in suffixes:
        x, y = open(str(a) + s, "rb").read(), open(str(b) + s, "rb").read()
        assert x == y, "%s%s and %s%s differ (%d / %d bytes)" % (a, s, b, s, len(x), len(y))
    return True


def iterations_run(out):
    return [int(l.split()[1].rstrip(":")) for l in out.splitlines() if l.startswith("iteration ")]


def run_dir(base, name):
    d = base / name; (d / "inter").mkdir(parents=True)
    return d


# ---- protein chain ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prot(golden, tmp_path_factory):
    """A: 4 iterations, uninterrupted.  B: 2 iterations, then resumed to 4 (crossing the hash shift's step 68 -> 69 between iterations 2 and 3,
    with findassemblystart's iteration in the stored part).  `b1`: a copy of B's files as the interrupted run left them."""
    t = tmp_path_factory.mktemp("resume_prot")
    inp = os.path.join(golden, "aa", "seq_0")
    tail = ["--filter-proteins", "0", "--fasta-out"]
    A, B = run_dir(t, "A"), run_dir(t, "B")
    r = {"t": t, "inp": inp, "A": A, "B": B, "tail": tail}
    r["outA"] = hip(["assemble-chain", inp, A / "out", "--num-iterations", "4", "--write-intermediate", A / "inter"] + tail + [A / "out.fasta"])
    r["outB1"] = hip(["assemble-chain", inp, B / "out", "--num-iterations", "2", "--resume", "1", "--write-intermediate", B / "inter"])
    r["b1_files"] = sorted(os.listdir(B / "inter"))
    shutil.copytree(B, t / "b1")
    r["outB2"] = hip(["assemble-chain", inp, B / "out", "--num-iterations", "4", "--resume", "1", "--write-intermediate", B / "inter"] + tail + [B / "out.fasta"])
    return r


def test_protein_chain_resumed_equals_uninterrupted(prot):
    A, B = prot["A"], prot["B"]
    assert iterations_run(prot["outA"]) == [0, 1, 2, 3] and "resuming" not in prot["outA"]
    # the interrupted run: a fresh run that leaves the manifest and, with --resume 1, its last iteration's DB as a resume point too
    assert iterations_run(prot["outB1"]) == [0, 1] and "resuming" not in prot["outB1"]
    assert prot["b1_files"] == sorted(["chain.manifest"] + ["assembly_%d%s" % (i, s) for i in (0, 1) for s in DB_SUFFIXES + (".done",)])
    # the continuation did not compute iterations 0-1 again
    assert "resuming at iteration 2" in prot["outB2"] and iterations_run(prot["outB2"]) == [2, 3]
    same_files(A / "out", B / "out")
    same_files(A / "inter" / "assembly_2", B / "inter" / "assembly_2")
    same_files(A / "out", B / "inter" / "assembly_3")          # (A, without --resume, writes iteration 3's DB as its output only)
    for i in (0, 1, 2):
        assert os.path.exists(A / "inter" / ("assembly_%d.done" % i)) and os.path.exists(B / "inter" / ("assembly_%d.done" % i))
        same_files(A / "inter" / ("assembly_%d" % i), B / "inter" / ("assembly_%d" % i))
    assert os.path.exists(B / "inter" / "assembly_3.done")
    # without --resume: the files a --write-intermediate run has always left, no manifest, no DB of the last iteration
    assert sorted(os.listdir(A / "inter")) == sorted("assembly_%d%s" % (i, s) for i in (0, 1, 2) for s in DB_SUFFIXES + (".done",))


def test_fasta_out_after_a_resume(prot):
    """SOURCE — the fragments before findassemblystart — is rebuilt on a resume: the tail selects and writes the same FASTA file"""
    assert os.path.getsize(prot["A"] / "out.fasta") > 0
    same_files(prot["A"] / "out.fasta", prot["B"] / "out.fasta", ("",))


def test_resume_behind_iteration_0_from_reads(golden, tmp_path):
    """j = 0, the boundary next to the findassemblystart iteration: 1 iteration, resumed to 3, against 3 uninterrupted iterations.  From the read DB,
    so that SOURCE of the tail comes out of the ORF preprocessing again."""
    inp = os.path.join(golden, "nucl", "seq_0")
    U, C = run_dir(tmp_path, "U"), run_dir(tmp_path, "C")
    flags = ["--from-reads", "1", "--filter-proteins", "0"]
    hip(["assemble-chain", inp, U / "out", "--num-iterations", "3", "--fasta-out", U / "out.fasta"] + flags)
    hip(["assemble-chain", inp, C / "out", "--num-iterations", "1", "--resume", "1", "--write-intermediate", C / "inter"] + flags)
    assert_same_db(os.path.join(golden, "fs", "assembly_0"), C / "inter" / "assembly_0", "the resume point behind iteration 0 is the reference's assembly_0")
    out = hip(["assemble-chain", inp, C / "out", "--num-iterations", "3", "--resume", "1", "--write-intermediate", C / "inter", "--fasta-out", C / "out.fasta"] + flags)
    assert "resuming at iteration 1" in out and iterations_run(out) == [1, 2]
    same_files(U / "out", C / "out")
    assert os.path.getsize(U / "out.fasta") > 0
    same_files(U / "out.fasta", C / "out.fasta", ("",))
    # already finished: no iteration left, the outputs are written from the stored DB
    out = hip(["assemble-chain", inp, C / "again", "--num-iterations", "3", "--resume", "1", "--write-intermediate", C / "inter"] + flags)
    assert "resuming at iteration 3" in out and iterations_run(out) == []
    same_files(U / "out", C / "again")


def test_crash_between_data_and_sentinel(prot):
    """the run died while it wrote assembly_2: half of its data file is there, its index even, but no sentinel — it is not a resume point and is written over"""
    t, A = prot["t"], prot["A"]
    D = t / "crash"; shutil.copytree(t / "b1", D)
    half = open(A / "inter" / "assembly_2", "rb").read()
    open(D / "inter" / "assembly_2", "wb").write(half[:len(half) // 2])
    shutil.copy(A / "inter" / "assembly_2.index", D / "inter" / "assembly_2.index")
    shutil.copy(A / "inter" / "assembly_2.dbtype", D / "inter" / "assembly_2.dbtype")
    out = hip(["assemble-chain", prot["inp"], D / "out", "--num-iterations", "4", "--resume", "1", "--write-intermediate", D / "inter"])
    assert "resuming at iteration 2" in out and iterations_run(out) == [2, 3]
    same_files(A / "out", D / "out")
    same_files(A / "inter" / "assembly_2", D / "inter" / "assembly_2")
    same_files(A / "out", D / "inter" / "assembly_3")


def test_mismatch_is_refused_on_the_device_path_too(prot):
    """the same refusals without the dry run: another -k, another input — exit 1, nothing computed, nothing written"""
    t = prot["t"]
    D = t / "refuse"; shutil.copytree(t / "b1", D)
    before = sorted(os.listdir(D / "inter"))
    base = ["assemble-chain", prot["inp"], D / "out2", "--num-iterations", "4", "--resume", "1", "--write-intermediate", D / "inter"]
    out = hip(base + ["-k", "13"], ok=1)
    assert ": -k differs" in out and iterations_run(out) == []
    out = hip(base[:1] + [os.path.join(os.path.dirname(os.path.dirname(prot["inp"])), "fs", "assembly_0")] + base[2:], ok=1)
    assert ": input.0.path differs" in out
    os.remove(D / "inter" / "chain.manifest")
    out = hip(base, ok=1)
    assert "chain.manifest" in out
    assert sorted(os.listdir(D / "inter")) == sorted(set(before) - {"chain.manifest"}) and not os.path.exists(D / "out2")


# ---- nucleotide chain ---------------------------------------------------------------------------------------------------------------
READ = 150
# (length, circular, coverage): the recipe of tests/golden/make_circular_chain.py — reads of both strands with 0.2 % substitutions, those of a
# circular replicon wrap around its origin — at the smallest size at which contigs close early: replicons of two to seven read lengths, which
# the CPU oracle's chain (kmermatcher -k 22, rescorediagonal, nuclassembleresults, cyclecheck --chop-cycle 1) finds circular in iterations 0-3
# (3 / 13 / 37 / 39 circular contigs)
COMMUNITY = [(300, True, 40.0), (450, True, 40.0), (700, True, 40.0), (1000, True, 40.0), (4000, False, 15.0)]


def write_small_circular_community(path):
    rng = np.random.default_rng(7)
    B = np.frombuffer(b"ACGT", dtype=np.uint8)
    comp = np.zeros(256, dtype=np.uint8); comp[B] = B[::-1]
    out = []
    for L, circular, cov in COMMUNITY:
        g = B[rng.integers(0, 4, L)]
        n = int(L * cov / READ)
        src = np.concatenate([g, g[:READ]]) if circular else g
        starts = rng.integers(0, L if circular else L - READ + 1, n)
        r = src[starts[:, None] + np.arange(READ)[None, :]].copy()
        err = rng.random(r.shape) < 0.002
        r[err] = B[(np.searchsorted(B, r[err]) + rng.integers(1, 4, int(err.sum()))) % 4]
        rev = rng.random(n) < 0.5
        r[rev] = comp[r[rev][:, ::-1]]
        out.append(r)
    r = np.concatenate(out)
    r = r[rng.permutation(len(r))]
    n = len(r)
    ent = np.empty((n, READ + 2), dtype=np.uint8); ent[:, :READ] = r; ent[:, READ] = 10; ent[:, READ + 1] = 0
    open(path, "wb").write(ent.tobytes())
    with open(path + ".index", "w") as f:
        for i in range(n):
            f.write("%d\t%d\t%d\n" % (i, i * (READ + 2), READ + 2))
    open(path + ".dbtype", "wb").write((1).to_bytes(4, "little"))
    return n


def cycle_files(d):
    return sorted(f for f in os.listdir(d) if f.startswith("out_cycle_"))


NUCL_TAIL = ["--min-contig-len", "200", "--db-mode", "1", "--db-out"]


@pytest.fixture(scope="module")
def nucl(tmp_path_factory):
    """the A / B1 / B2 pattern on nuclassemble-chain --chop-cycle 1: interrupted behind iteration 1, with circular contigs taken out before and after"""
    t = tmp_path_factory.mktemp("resume_nucl")
    inp = str(t / "reads")
    assert write_small_circular_community(inp) == 1052
    A, B = run_dir(t, "A"), run_dir(t, "B")
    r = {"t": t, "inp": inp, "A": A, "B": B}
    common = ["--chop-cycle", "1", "--write-intermediate"]
    r["outA"] = hip(["nuclassemble-chain", inp, A / "out", "--num-iterations", "4"] + common + [A / "inter"] + NUCL_TAIL + [A / "d"])
    r["outB1"] = hip(["nuclassemble-chain", inp, B / "out", "--num-iterations", "2", "--resume", "1"] + common + [B / "inter"])
    shutil.copytree(B, t / "b1")
    r["outB2"] = hip(["nuclassemble-chain", inp, B / "out", "--num-iterations", "4", "--resume", "1"] + common + [B / "inter"] + NUCL_TAIL + [B / "d"])
    return r


def check_nucl(A, D):
    same_files(A / "out", D / "out")
    assert cycle_files(A) == cycle_files(D)
    for f in cycle_files(A):
        if "." not in f:
            same_files(A / f, D / f)
    same_files(A / "d", D / "d")
    same_files(A / "d_cycle", D / "d_cycle", (".index",))
    same_files(A / "inter" / "assembly_2", D / "inter" / "assembly_2")
    same_files(A / "out", D / "inter" / "assembly_3")


def test_nucleotide_chain_resumed_equals_uninterrupted(nucl):
    A, B, b1 = nucl["A"], nucl["B"], nucl["t"] / "b1"
    # the test proves nothing unless cyclecheck took circular contigs out BEFORE the interruption (they reach RESULT through <o>_cycle_<i> only) and after it
    early = [f for f in cycle_files(b1) if "." not in f]
    assert early and set(early) <= {"out_cycle_0", "out_cycle_1"} and all(os.path.getsize(b1 / f) > 0 for f in early), cycle_files(b1)
    assert any(os.path.getsize(A / f) > 0 for f in ("out_cycle_2", "out_cycle_3") if os.path.exists(A / f)), cycle_files(A)
    assert iterations_run(nucl["outA"]) == [0, 1, 2, 3] and iterations_run(nucl["outB1"]) == [0, 1]
    assert "resuming at iteration 2" in nucl["outB2"] and iterations_run(nucl["outB2"]) == [2, 3]
    check_nucl(A, B)
    # circular contigs among the selected ones: DB_cycle.index has lines, all of them lines of DB.index
    cyc = open(str(A / "d_cycle") + ".index").read().splitlines()
    assert cyc and set(cyc) <= set(open(str(A / "d") + ".index").read().splitlines())
    # the stored DB is the rest AFTER cyclecheck: no key of a circular contig of iterations 0-1 is in assembly_1
    keys = lambda p: {int(l.split()[0]) for l in open(str(p) + ".index")}
    assert not (keys(B / "inter" / "assembly_1") & set().union(*(keys(b1 / f) for f in early)))


# ---- the library's caches start cold on a resume; none of them changes a result ------------------------------------------------------------
def test_resumed_runs_with_the_window_cache_off(prot, nucl):
    off = {"PLASSHIP_TUNE_KMCACHE": "2"}
    P = prot["t"] / "cold"; shutil.copytree(prot["t"] / "b1", P)
    out = hip(["assemble-chain", prot["inp"], P / "out", "--num-iterations", "4", "--resume", "1", "--write-intermediate", P / "inter"] + prot["tail"] + [P / "out.fasta"], env=off)
    assert iterations_run(out) == [2, 3]
    same_files(prot["A"] / "out", P / "out")
    same_files(prot["A"] / "out.fasta", P / "out.fasta", ("",))
    same_files(prot["A"] / "inter" / "assembly_2", P / "inter" / "assembly_2")
    N = nucl["t"] / "cold"; shutil.copytree(nucl["t"] / "b1", N)
    out = hip(["nuclassemble-chain", nucl["inp"], N / "out", "--num-iterations", "4", "--resume", "1", "--chop-cycle", "1", "--write-intermediate", N / "inter"] + NUCL_TAIL + [N / "d"], env=off)
    assert iterations_run(out) == [2, 3]
    check_nucl(nucl["A"], N)


# ---- guided chain --------------------------------------------------------------------------------------------------------------------
def test_guided_chain_refuses_resume(golden, tmp_path):
    """--write-intermediate stores assembly_nucl_<i> without the protein twins guidedassembleresults extends next to it: not enough to restart.
    --resume 1 ends with a message and exit 1 before anything is read; nothing is written."""
    d = tmp_path / "inter"; d.mkdir()
    out = hip(["guidedassemble-chain", os.path.join(golden, "nucl", "seq_0"), tmp_path / "n", tmp_path / "a", "--num-iterations", "2", "--resume", "1", "--write-intermediate", d], ok=1)
    assert "--resume" in out and iterations_run(out) == []
    assert os.listdir(d) == [] and sorted(os.listdir(tmp_path)) == ["inter"]
