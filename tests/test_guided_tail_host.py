"""The command lines of the workflows' --db-mode end, without a GPU (PLASSHIP_CLI_DRYRUN=1: parsed and validated, nothing read or computed):
`plass-hip nuclassemble-chain --db-mode 1 --db-out DB` and `plass-hip guidedassemble-chain --nuclassembly-out DB`
(data/nuclassemble.sh:200-207, data/guidedNuclAssemble.sh:135-170)."""
import os
import subprocess

from conftest import ROOT

EXE = os.path.join(ROOT, "plass_amd", "plass-hip")


def cli(*args):
    p = subprocess.run([EXE] + [str(a) for a in args], env=dict(os.environ, PLASSHIP_CLI_DRYRUN="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return p.returncode, p.stdout


def test_new_flags_parse(tmp_path):
    o = tmp_path / "out"
    assert cli("nuclassemble-chain", "in", "asm", "--db-mode", "1", "--db-out", o)[0] == 96
    assert cli("nuclassemble-chain", "in", "asm", "--db-mode", "--db-out", o)[0] == 96                     # a bool flag without a value toggles its default
    assert cli("nuclassemble-chain", "r1.fastq", "r2.fastq", "asm", "--db-mode", "1", "--db-out", o, "--min-contig-len", "200", "--contig-output-mode", "0")[0] == 96
    assert cli("guidedassemble-chain", "reads", "nucl", "aa", "--nuclassembly-out", o)[0] == 96
    assert cli("guidedassemble-chain", "r1.fastq.gz", "r2.fastq.gz", "nucl", "aa", "--num-iterations", "aa:2,nucl:3", "-k", "aa:14,nucl:22",
               "--min-seq-id", "aa:0.97,nucl:0.99", "--nuclassembly-out", o, "--min-contig-len", "500", "--contig-output-mode", "1", "--chop-cycle", "1")[0] == 96
    # every combination that parsed before still does
    assert cli("nuclassemble-chain", "in", "asm", "--fasta-out", tmp_path / "f.fasta")[0] == 96
    assert cli("nuclassemble-chain", "in", "asm", "--num-iterations", "2")[0] == 96
    assert cli("guidedassemble-chain", "reads", "nucl", "aa", "--num-iterations", "2")[0] == 96


def test_db_mode_and_fasta_out_exclude_each_other(tmp_path):
    rc, out = cli("nuclassemble-chain", "in", "asm", "--db-mode", "1", "--fasta-out", tmp_path / "x")
    assert rc == 1 and "--fasta-out" in out
    rc, out = cli("nuclassemble-chain", "in", "asm", "--db-mode", "1", "--db-out", tmp_path / "d", "--fasta-out", tmp_path / "x")
    assert rc == 1 and "--fasta-out" in out
    assert not os.listdir(tmp_path)
    # the two halves of db-mode go together, and an output that exists is refused like the script's OUT_FILE (nuclassemble.sh:69)
    assert cli("nuclassemble-chain", "in", "asm", "--db-mode", "1")[0] == 1
    assert cli("nuclassemble-chain", "in", "asm", "--db-out", tmp_path / "d")[0] == 1
    assert cli("nuclassemble-chain", "in", "asm", "--db-mode", "1", "--db-out", tmp_path / "d", "--contig-output-mode", "2")[0] == 1
    (tmp_path / "there").write_bytes(b"")
    for args in (["nuclassemble-chain", "in", "asm", "--db-mode", "1", "--db-out", tmp_path / "there"],
                 ["guidedassemble-chain", "reads", "nucl", "aa", "--nuclassembly-out", tmp_path / "there"]):
        rc, out = cli(*args)
        assert rc == 1 and "exists already" in out


def test_unknown_flags_and_modules_as_before():
    for args in (["nuclassemble-chain", "in", "asm", "--db-mode", "1", "--db-out", "o", "--no-such-flag", "1"],
                 ["guidedassemble-chain", "reads", "nucl", "aa", "--nuclassembly-out", "o", "--no-such-flag", "1"],
                 ["guidedassemble-chain", "reads", "nucl", "aa", "--db-out", "o"],          # nuclassemble-chain's flag
                 ["nuclassemble-chain", "in", "asm", "--nuclassembly-out", "o"],             # guidedassemble-chain's flag
                 ["assemble-chain", "in", "asm", "--db-mode", "1"]):
        rc, out = cli(*args)
        assert rc == 1 and "Unrecognized parameter" in out, (args, out)
    # no new module name: the rest of the guided workflow's tail stays with the reference (exit 95 -> plass-gpu-wrapper)
    for mod in ("linclust", "result2repseq", "createsubdb", "nuclassemble", "guided_nuclassemble"):
        assert cli(mod, "a", "b", "c")[0] == 95
    assert cli("rescorediagonal", "q", "t", "p", "o", "--rescore-mode", "0", "--wrapped-scoring", "1")[0] == 95
