"""createdb for reads on the device (plass_amd/csrc/createdb.hip): `plass-hip createdb-reads`, Context.createdb and the chains' --single-end 1.
Yardsticks: the files the unmodified reference's createdb wrote (tests/golden/createdb.tar.gz, createdb_example.tar.gz) and, for inputs
generated here, the plain-Python restatement tests/tools/createdb_check.py, which tests/test_createdb_host.py pins against the same files."""
import filecmp
import gzip
import os
import subprocess
import sys
import tarfile

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import createdb_check as cc  # noqa: E402

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "plass_amd", "plass-hip")
R1 = os.path.join(ROOT, "tests", "golden", "example_reads", "reads_1.fastq.gz")
OK_CASES = ["n1", "n31", "n32", "n33", "n64", "n65", "mixed_fq", "mixed_fa", "wrapped", "fq_then_fa", "long40k", "nonl_fq", "nonl_fa", "crlf_fq",
            "crlf_fa", "gz"]


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    d = tmp_path_factory.mktemp("createdb_fixture")
    for name in ("createdb.tar.gz", "createdb_example.tar.gz"):
        with tarfile.open(os.path.join(ROOT, "tests", "golden", name)) as t:
            t.extractall(d)
    cases = {}
    for line in open(d / "createdb" / "in" / "CASES").read().splitlines():
        name, expect, files = line.split("\t")
        cases[name] = (expect, [str(d / "createdb" / "in" / f) for f in files.split()])
    assert set(OK_CASES) == {k for k, v in cases.items() if v[0] == "ok"}
    return d, cases


@pytest.fixture(scope="module")
def ctx():
    import plass_amd
    with plass_amd.Context(0) as c:
        yield c


def cli(*args, env=None, check=True):
    e = dict(os.environ)
    e.pop("PLASSHIP_CLI_DRYRUN", None)
    e.update(env or {})
    p = subprocess.run([EXE] + [str(a) for a in args], env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    if check:
        assert p.returncode == 0, p.stdout
    return p


def assert_db_equal(got_prefix, want, what):
    got = cc.read_db(got_prefix)
    for suffix in cc.SUFFIXES:
        assert got[suffix] == want[suffix], "%s: db%s differs" % (what, suffix)


@pytest.mark.parametrize("case", OK_CASES)
def test_fixture_case_command_line_and_python(case, fx, ctx, tmp_path, monkeypatch):
    """every file createdb writes, byte for byte the reference's: through the command, through Context.createdb (both shuffle modes the
    fixture holds), and with the input cut into 1 KB and 3 KB chunks — lines, '\\r\\n' pairs and records then straddle the chunk ends"""
    d, cases = fx
    files = cases[case][1]
    ref = d / "createdb" / "ref" / case
    want = cc.read_db(ref / "s1" / "db")
    cli("createdb-reads", *files, tmp_path / "c")
    assert_db_equal(tmp_path / "c", want, case + " (command)")
    for mode in ("s1", "s0"):
        if not (ref / mode / "db").exists():
            continue
        w = cc.read_db(ref / mode / "db")
        for kb in (0, 1, 3):
            if kb:
                monkeypatch.setenv("PLASSHIP_TUNE_FASTQ_CHUNK_KB", str(kb))
            else:
                monkeypatch.delenv("PLASSHIP_TUNE_FASTQ_CHUNK_KB", raising=False)
            out = tmp_path / ("p_%s_%d" % (mode, kb))
            reads, st = ctx.createdb(files, shuffle=mode == "s1", out=out)
            assert_db_equal(out, w, "%s/%s chunk %d KB (python)" % (case, mode, kb))
            assert st.entries == w[".index"].count(b"\n") and st.files == len(files)
            total = sum(len(cc.read_file(f)) for f in files)
            if kb and total > 3 * 1024:
                assert st.chunks > len(files), "the input was never split"
            if kb == 0:
                assert st.chunks == len(files)
            # the handle is the DB that was written
            reads.write(str(out) + "_again")
            for s in ("", ".index", ".dbtype"):
                assert open(str(out) + "_again" + s, "rb").read() == w[s]
            reads.free()


def test_chunked_command_line(fx, tmp_path):
    d, cases = fx
    files = cases["mixed_fq"][1]
    p = cli("createdb-reads", *files, tmp_path / "c", env={"PLASSHIP_TUNE_FASTQ_CHUNK_KB": "7"})
    assert_db_equal(tmp_path / "c", cc.read_db(d / "createdb" / "ref" / "mixed_fq" / "s1" / "db"), "7 KB chunks")
    chunks = int(p.stdout.split("chunks: ")[1].split()[0])
    assert chunks > 10


def test_refusals_come_before_any_output(fx, ctx, tmp_path):
    import plass_amd
    d, cases = fx
    for name in ("protein", "noplus", "qlen", "q200"):
        expect, files = cases[name]
        out = tmp_path / name
        p = cli("createdb-reads", *files, out, check=False)
        if expect == "95":
            assert p.returncode == 95, p.stdout
        else:
            assert p.returncode == 1 and ": record %s: " % expect.split(":")[1] in p.stdout, p.stdout
        assert [f for f in os.listdir(tmp_path) if f.startswith(name)] == [], "something was written"
        with pytest.raises(plass_amd.PlasshipError) as e:
            ctx.createdb(files)
        assert ("(-4)" if expect == "95" else "(-2)") in str(e.value)
        # the chains refuse the same file the same way
        pc = cli("nuclassemble-chain", *files, tmp_path / (name + "_o"), "--single-end", "1", check=False)
        assert pc.returncode == p.returncode, pc.stdout
    assert os.listdir(tmp_path) == []


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    """20 000 reads of 36..250 nt generated here, as FASTQ (plain and .gz) and what the restatement makes of them"""
    d = tmp_path_factory.mktemp("generated")
    rng = np.random.default_rng(7)
    acgt = np.frombuffer(b"ACGTN", dtype=np.uint8)
    parts = []
    for i in range(20000):
        n = int(rng.integers(36, 251))
        s = acgt[rng.choice(5, size=n, p=[0.245, 0.245, 0.245, 0.245, 0.02])].tobytes()
        parts.append(b"@read%d%s\n%s\n+\n%s\n" % (i, b" 1:N:0" if i % 3 else b"", s, b"F" * n))
    text = b"".join(parts)
    (d / "g.fastq").write_bytes(text)
    with open(d / "g.fastq.gz", "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, compresslevel=1) as f:
        f.write(text)
    return d, cc.createdb([d / "g.fastq"]), cc.createdb([d / "g.fastq.gz"])


@pytest.mark.parametrize("ext", ["fastq", "fastq.gz"])
def test_generated_reads_against_the_restatement(ext, generated, ctx, tmp_path):
    d, want_plain, want_gz = generated
    reads, st = ctx.createdb([d / ("g." + ext)], out=tmp_path / "db")
    reads.free()
    assert st.entries == 20000 and st.lines == 80000
    assert_db_equal(tmp_path / "db", want_gz if ext.endswith(".gz") else want_plain, ext)


@pytest.fixture(scope="module")
def example_db(fx, tmp_path_factory):
    """mate 1 of the bundled example as a single-end library: our DB of it (which must be the reference's) and the reference's own"""
    d, _ = fx
    out = tmp_path_factory.mktemp("example") / "db"
    cli("createdb-reads", R1, out)
    want = cc.read_db(d / "createdb_example" / "db")
    assert_db_equal(out, want, "example reads")
    return out, d / "createdb_example" / "db"


def same_files(a, b, suffixes=("", ".index", ".dbtype")):
    for s in suffixes:
        assert filecmp.cmp(str(a) + s, str(b) + s, shallow=False), "%s%s differs from %s%s" % (a, s, b, s)


def test_assemble_chain_single_end_equals_the_db_forms(example_db, tmp_path):
    ours, refs = example_db
    p = cli("assemble-chain", R1, tmp_path / "a", "--single-end", "1", "--num-iterations", "2")
    assert "createdb: " in p.stdout
    cli("assemble-chain", ours, tmp_path / "b", "--from-reads", "1", "--num-iterations", "2")
    cli("assemble-chain", refs, tmp_path / "c", "--from-reads", "1", "--num-iterations", "2")
    same_files(tmp_path / "a", tmp_path / "b")
    same_files(tmp_path / "a", tmp_path / "c")
    assert os.path.getsize(tmp_path / "a") > 100000


def test_nuclassemble_chain_single_end_equals_the_db_form(example_db, tmp_path):
    ours, _ = example_db
    cli("nuclassemble-chain", R1, tmp_path / "a", "--single-end", "1", "--num-iterations", "1")
    cli("nuclassemble-chain", ours, tmp_path / "b", "--num-iterations", "1")
    same_files(tmp_path / "a", tmp_path / "b")
    assert sorted(f[1:] for f in os.listdir(tmp_path) if f.startswith("a")) == sorted(f[1:] for f in os.listdir(tmp_path) if f.startswith("b"))


def test_guidedassemble_chain_single_end_equals_the_db_form(example_db, tmp_path):
    ours, _ = example_db
    cli("guidedassemble-chain", R1, tmp_path / "an", tmp_path / "aa", "--single-end", "1", "--num-iterations", "1")
    cli("guidedassemble-chain", ours, tmp_path / "bn", tmp_path / "ba", "--num-iterations", "1")
    same_files(tmp_path / "an", tmp_path / "bn")
    same_files(tmp_path / "aa", tmp_path / "ba")


def test_single_end_fasta_out_equals_the_db_form(example_db, tmp_path):
    ours, _ = example_db
    flags = ["--num-iterations", "2", "--filter-proteins", "0"]
    cli("assemble-chain", R1, tmp_path / "a", "--single-end", "1", "--fasta-out", tmp_path / "a.fasta", *flags)
    cli("assemble-chain", ours, tmp_path / "b", "--from-reads", "1", "--fasta-out", tmp_path / "b.fasta", *flags)
    assert filecmp.cmp(tmp_path / "a.fasta", tmp_path / "b.fasta", shallow=False)
    same_files(tmp_path / "a", tmp_path / "b")


def test_odd_count_without_the_flag_is_answered_as_before(tmp_path):
    p = cli("assemble-chain", R1, R1, R1, tmp_path / "o", check=False)
    assert p.returncode == 1 and "assemble-chain: one DB or pairs of FASTQ files before the output" in p.stdout
    assert os.listdir(tmp_path) == []
