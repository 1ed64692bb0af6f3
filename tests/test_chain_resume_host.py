"""`plass-hip assemble-chain / nuclassemble-chain --resume 1` without a GPU: what is refused before anything is read (PLASSHIP_CLI_DRYRUN=1:
the command line is parsed and validated, an accepted call ends with 96), and plass_amd.resume_point(), the driver's rule for where a run goes on."""
import os
import subprocess

from conftest import ROOT

EXE = os.path.join(ROOT, "plass_amd", "plass-hip")


def cli(*args):
    p = subprocess.run([EXE] + [str(a) for a in args], env=dict(os.environ, PLASSHIP_CLI_DRYRUN="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return p.returncode, p.stdout


def resume_point_files(d, i, done=True, db=True):
    if db:
        for s in ("", ".index", ".dbtype"):
            (d / ("assembly_%d%s" % (i, s))).write_bytes(b"")
    if done:
        (d / ("assembly_%d.done" % i)).write_bytes(b"")


def listing(d):
    return sorted(os.listdir(d))


def test_resume_needs_write_intermediate(tmp_path):
    for mod in ("assemble-chain", "nuclassemble-chain"):
        rc, out = cli(mod, "in", tmp_path / "asm", "--resume", "1")
        assert rc == 1 and "--write-intermediate" in out, out
        # with the directory: a fresh run (no sentinel), accepted; the dry run writes nothing, not the manifest either
        assert cli(mod, "in", tmp_path / "asm", "--resume", "1", "--write-intermediate", tmp_path)[0] == 96
        assert cli(mod, "in", tmp_path / "asm", "--resume", "0")[0] == 96
    assert listing(tmp_path) == []
    # the flag belongs to the chains only
    rc, out = cli("kmermatcher", "in", "out", "-k", "14", "--kmer-per-seq", "60", "--resume", "1")
    assert rc == 1 and "Unrecognized parameter" in out


def test_guided_chain_refuses_resume(tmp_path):
    """--write-intermediate stores assembly_nucl_<i> without the protein twins: not enough to restart, so the flag is refused by name"""
    rc, out = cli("guidedassemble-chain", "reads", tmp_path / "n", tmp_path / "a", "--resume", "1", "--write-intermediate", tmp_path)
    assert rc == 1 and "--resume" in out and "guidedassemble-chain" in out, out
    assert listing(tmp_path) == []
    assert cli("guidedassemble-chain", "reads", tmp_path / "n", tmp_path / "a", "--write-intermediate", tmp_path)[0] == 96


def test_manifest_is_checked_before_anything_is_read(tmp_path):
    d = tmp_path / "inter"; d.mkdir()
    inp = tmp_path / "in"
    for s in ("", ".index", ".dbtype"):
        (tmp_path / ("in" + s)).write_bytes(b"x")
    base = ["assemble-chain", inp, tmp_path / "asm", "--write-intermediate", d, "--resume", "1"]
    resume_point_files(d, 0)
    before = listing(d)
    # sentinels without a manifest
    rc, out = cli(*base)
    assert rc == 1 and "chain.manifest" in out and "assembly_0.done" in out, out
    # a manifest of another -k: the key is named (the first line of the file is the module, the second -k)
    (d / "chain.manifest").write_text("module assemble-chain\n-k 13\n")
    rc, out = cli(*base)
    assert rc == 1 and ": -k differs" in out and "13" in out and "14" in out, out
    rc, out = cli(*(base + ["-k", "13"]))
    assert rc == 1 and ": --alph-size differs" in out, out                # -k agrees now; the next key the file lacks
    (d / "chain.manifest").write_text("module nuclassemble-chain\n-k 14\n")
    rc, out = cli(*base)
    assert rc == 1 and ": module differs" in out, out
    assert listing(d) == before + ["chain.manifest"] and not os.path.exists(tmp_path / "asm")
    # a limit below the sentinel: nothing to resume from, a fresh run, the manifest is not looked at
    resume_point_files(d, 1); os.remove(d / "assembly_0.done")
    assert cli(*(base + ["--num-iterations", "1"]))[0] == 96
    assert cli(*(base + ["--num-iterations", "2"]))[0] == 1
    # without --resume the directory is not looked at at all
    assert cli("assemble-chain", inp, tmp_path / "asm", "--write-intermediate", d)[0] == 96


def test_resume_point(tmp_path):
    import plass_amd
    rp = plass_amd.resume_point
    assert rp(tmp_path, 12) is None and rp(tmp_path / "missing", 12) is None
    resume_point_files(tmp_path, 0); resume_point_files(tmp_path, 1)
    assert rp(tmp_path, 12) == 1 and rp(str(tmp_path), 2) == 1 and rp(tmp_path, 1) == 0 and rp(tmp_path, 0) is None
    resume_point_files(tmp_path, 3)
    assert rp(tmp_path, 3) == 1 and rp(tmp_path, 4) == 3 and rp(tmp_path, 12) == 3
    # a sentinel without its DB is no resume point (nor is a DB without its sentinel: it may be half written)
    resume_point_files(tmp_path, 5, db=False)
    resume_point_files(tmp_path, 4, done=False)
    assert rp(tmp_path, 12) == 3
    os.remove(tmp_path / "assembly_3.index")
    assert rp(tmp_path, 12) == 1
    # the guided chain's name for its intermediate DBs
    assert rp(tmp_path, 12, name="assembly_nucl_") is None


def test_driver_and_helper_agree(tmp_path):
    """the same directories through the driver: it resumes (and then asks for the manifest) exactly where resume_point() finds a resume point"""
    import plass_amd
    d = tmp_path / "inter"; d.mkdir()
    base = ["nuclassemble-chain", "in", tmp_path / "asm", "--write-intermediate", d, "--resume", "1"]
    resume_point_files(d, 2, db=False); resume_point_files(d, 1, done=False)
    assert plass_amd.resume_point(d, 8) is None and cli(*base)[0] == 96
    resume_point_files(d, 0); resume_point_files(d, 1); resume_point_files(d, 3)
    for limit in (1, 2, 3, 4, 8):
        j = plass_amd.resume_point(d, limit)
        rc, out = cli(*(base + ["--num-iterations", limit]))
        assert rc == 1 and ("assembly_%d.done" % j) in out, (limit, out)
