"""createdb for reads, the checks that need no GPU: the plain-Python restatement (tests/tools/createdb_check.py) against the files the
unmodified reference wrote (tests/golden/createdb.tar.gz, made by tests/golden/make_createdb.sh), the C-ABI symbols, the README's table of
switches against the build, and the dry-run exit codes of the new command-line forms."""
import os
import re
import subprocess
import sys
import tarfile

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import createdb_check as cc  # noqa: E402


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    d = tmp_path_factory.mktemp("createdb_fixture")
    with tarfile.open(os.path.join(ROOT, "tests", "golden", "createdb.tar.gz")) as t:
        t.extractall(d)
    return d / "createdb"


def cases(fx):
    for line in open(fx / "in" / "CASES").read().splitlines():
        name, expect, files = line.split("\t")
        yield name, expect, [str(fx / "in" / f) for f in files.split()]


def test_restatement_equals_the_reference_byte_for_byte(fixture):
    seen = 0
    for name, expect, files in cases(fixture):
        if expect != "ok":
            continue
        for mode in ("s1", "s0"):
            ref = fixture / "ref" / name / mode / "db"
            if not ref.exists():
                continue
            want, got = cc.read_db(ref), cc.createdb(files, shuffle=mode == "s1")
            for suffix in cc.SUFFIXES:
                assert got[suffix] == want[suffix], "%s/%s: db%s differs from the reference's" % (name, mode, suffix)
            seen += 1
    assert seen >= 20


def test_fixture_covers_what_it_is_for(fixture):
    """the fixture cannot pass vacuously: split boundaries, two files, both formats, '\\r\\n', a missing last '\\n', tabs, a long entry"""
    by = {name: (expect, files) for name, expect, files in cases(fixture)}
    assert {"n1", "n31", "n32", "n33", "n64", "n65"} <= set(by) and len(by["mixed_fq"][1]) == 2
    assert len(cc.kseq_records(cc.read_file(by["mixed_fq"][1][0])) + cc.kseq_records(cc.read_file(by["mixed_fq"][1][1]))) > 700
    assert cc.read_file(by["crlf_fa"][1][0]).count(b"\r\n") > 100 and not cc.read_file(by["nonl_fq"][1][0]).endswith(b"\n")
    assert any(b"\t" in cc.read_file(f) for f in by["mixed_fa"][1])
    assert max(len(s) for _, _, s in cc.kseq_records(cc.read_file(by["long40k"][1][0]))) > 40000
    assert by["protein"][0] == "95" and {by[k][0][0] for k in ("noplus", "qlen", "q200")} == {"1"}
    # the header DB of the reference really turns the tab behind a name into a blank and keeps the ones inside the comment
    h = cc.read_db(fixture / "ref" / "mixed_fq" / "s1" / "db")["_h"]
    assert b"\tlen=" not in h and b" len=" in h and b" tab\n" in h


def test_shuffle_keys_formula():
    """the closed form of the device (createdb.hip, keyRank) against the construction by splits"""
    for n in (1, 31, 32, 33, 64, 65, 703):
        for o in (0, 5, 37):
            pos = cc.shuffle_keys(n, True, o)
            cnt = [sum(1 for j in range(n) if (o + j) % 32 == s) for s in range(32)]
            for i in range(n):
                s = (o + i) % 32
                i0 = (s - o) % 32
                assert pos[i] == sum(cnt[:s]) + (i - i0) // 32
            assert sorted(pos) == list(range(n))


def test_c_abi_symbols_and_binding():
    from plass_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "plasship.h")).read()
    bound = {s[0] for s in _lib.SYMBOLS}
    for name in ("plasship_createdb", "plasship_createdb_write"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in bound
    import plass_amd
    if os.path.exists(plass_amd.lib_path()):
        lib = plass_amd.load_library()
        assert hasattr(lib, "plasship_createdb") and hasattr(lib, "plasship_createdb_write")
    import ctypes as C
    assert C.sizeof(_lib._CreatedbParams) == 12 and C.sizeof(_lib.CreatedbStats) == 72


def test_readme_switch_table_lists_the_switches_of_the_build():
    core = open(os.path.join(ROOT, "plass_amd", "csrc", "core.hip")).read()
    names = set(re.findall(r'"([A-Z0-9_]+)"', re.search(r"TUNE_NAMES\[\] = \{(.*?)\};", core, re.S).group(1)))
    table = set(re.findall(r"^\| `PLASSHIP_TUNE_([A-Z0-9_]+)`", open(os.path.join(ROOT, "README.md")).read(), re.M))
    assert "FASTQ_CHUNK_KB" in names and names == table


def test_dry_run_exit_codes_of_the_new_forms():
    exe = os.path.join(ROOT, "plass_amd", "plass-hip")
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build()
    env = dict(os.environ, PLASSHIP_CLI_DRYRUN="1")

    def run(*args):
        p = subprocess.run([exe] + list(args), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        return p.returncode, p.stdout

    rc = lambda *a: run(*a)[0]
    assert rc("createdb-reads", "r.fastq", "db") == 96 and rc("createdb-reads", "a.fq.gz", "b.fasta", "c.fq", "db", "--shuffle", "0", "--id-offset", "7") == 96
    assert rc("createdb-reads", "r.fastq", "db", "--dbtype", "2", "--threads", "4", "-v", "1") == 96
    assert rc("createdb-reads", "db") == 1 and rc("createdb-reads", "r.fastq", "db", "--no-such-flag", "1") == 1
    assert rc("createdb-reads", "stdin", "db") == 95 and rc("createdb-reads", "r.fastq.bz2", "db") == 95
    assert rc("createdb-reads", "r.fastq", "db", "--createdb-mode", "1") == 95 and rc("createdb-reads", "r.fastq", "db", "--compressed", "1") == 95
    assert rc("createdb-reads", "r.fastq", "db", "--write-lookup", "0") == 95 and rc("createdb-reads", "r.fastq", "db", "--dbtype", "1") == 95
    assert rc("createdb", "r.fastq", "db") == 95                      # the reference's own module name stays with the reference
    for chain, outs in (("assemble-chain", ["o"]), ("nuclassemble-chain", ["o"]), ("guidedassemble-chain", ["on", "oa"])):
        assert rc(chain, "r.fastq", *outs, "--single-end", "1") == 96
        assert rc(chain, "a.fastq", "b.fasta.gz", "c.fastq", *outs, "--single-end", "1") == 96
        assert rc(chain, "stdin", *outs, "--single-end", "1") == 95 and rc(chain, "a.fq", "b.bz2", *outs, "--single-end", "1") == 95
        assert rc(chain, *outs, "--single-end", "1") == 1
        # without the flag nothing changed: an odd number of read files is answered as before
        code, text = run(chain, "a.fastq", "b.fastq", "c.fastq", *outs)
        assert code == 1 and "%s: one DB or pairs of FASTQ files before the output" % chain in text
        assert rc(chain, "a.fastq", "b.fastq", *outs) == 96 and rc(chain, "db", *outs) == 96
