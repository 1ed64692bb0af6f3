"""CPU tests of the workflows' tail: tests/tools/contigcheck.py (the numpy restatement the GPU's plasship_select_contigs /
plasship_fasta_write are compared with) against the FASTA files the unmodified reference wrote (tests/golden/fasta_tail_*.tar.gz, made by
tests/golden/make_fasta_tail.sh), and the command-line refusals of --fasta-out, which end before a device is opened."""
import os
import subprocess
import sys
import tarfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import contigcheck  # noqa: E402

HIP = os.path.join(ROOT, "plass_amd", "plass-hip")
CASES = ["case1", "case2", "case3", "case4", "case5"]


def extract_case(case, dest):
    with tarfile.open(os.path.join(ROOT, "tests", "golden", "fasta_tail_%s.tar.gz" % case)) as t:
        t.extractall(dest)
    return os.path.join(str(dest), "fasta_tail", case)


@pytest.mark.parametrize("case", CASES)
def test_checker_reproduces_reference_fasta(case, tmp_path):
    d = extract_case(case, tmp_path)
    ok, mode, flags, result, source, cyc, ids, sets = contigcheck.check_case(d)
    assert len(ids) > 0
    assert ok, "%s: the checker's FASTA differs from the reference's" % case


def test_fixture_is_not_vacuous(tmp_path):
    """the conditions make_fasta_tail.sh asserted at generation time: S2 \\ S1 is reached, case 5 has circular contigs, mode 0 keeps more"""
    for c in CASES:
        extract_case(c, tmp_path)
    contigcheck.assert_fixture(os.path.join(str(tmp_path), "fasta_tail"))


def run_cli(args):
    return subprocess.run([HIP] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)


def test_fasta_out_needs_filter_proteins_0(tmp_path):
    """plass assemble filters with filternoncoding by default (--filter-proteins 1): not on the GPU path, exit 95 before anything is read"""
    out = tmp_path / "out.fasta"
    for extra in ([], ["--filter-proteins", "1"]):
        p = run_cli(["assemble-chain", tmp_path / "missing_in", tmp_path / "db", "--fasta-out", out] + extra)
        assert p.returncode == 95, p.stdout
        assert "filternoncoding" in p.stdout
        assert not out.exists() and not (tmp_path / "db").exists()


def test_fasta_out_not_on_guided_chain(tmp_path):
    p = run_cli(["guidedassemble-chain", tmp_path / "in", tmp_path / "n", tmp_path / "a", "--fasta-out", tmp_path / "o.fasta"])
    assert p.returncode != 0 and "Unrecognized parameter" in p.stdout, p.stdout


def test_fasta_out_existing_file_refused(tmp_path):
    out = tmp_path / "out.fasta"
    out.write_bytes(b"keep me\n")
    for args in (["assemble-chain", tmp_path / "in", tmp_path / "db", "--filter-proteins", "0"], ["nuclassemble-chain", tmp_path / "in", tmp_path / "db"]):
        p = run_cli(args + ["--fasta-out", out])
        assert p.returncode == 1 and "exists already" in p.stdout, p.stdout
        assert out.read_bytes() == b"keep me\n" and not (tmp_path / "db").exists()


def test_workflow_flags_parse():
    """the flag set of the workflows' own tail parses (nothing is read in a dry run)"""
    env = dict(os.environ, PLASSHIP_CLI_DRYRUN="1")
    for args in (["assemble-chain", "in", "db", "--fasta-out", "o.fasta", "--filter-proteins", "0", "--protein-filter-threshold", "0.2"],
                 ["nuclassemble-chain", "in", "db", "--fasta-out", "o.fasta", "--min-contig-len", "200", "--contig-output-mode", "0"]):
        p = subprocess.run([HIP] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60, env=env)
        assert p.returncode == 96, p.stdout
