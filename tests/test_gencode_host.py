"""Genetic codes other than the standard one, without a GPU: the sequential restatement (tests/tools/gencode_ref.py) against every DB the unmodified
reference wrote (tests/golden/gencode.tar.gz, made by tests/golden/make_gencode.sh), the tables the library states, the exported symbols of the new
extension library, the new command lines in dry run and the wrapper's opt-in routing."""
import ctypes as C
import os
import subprocess
import sys
import tarfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gencode_ref as G  # noqa: E402

CLI = os.path.join(ROOT, "plass_amd", "plass-hip")
WRAPPER = os.path.join(ROOT, "plass_amd", "plass-gpu-wrapper")
ERR_ARG = -1


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    d = tmp_path_factory.mktemp("gencode")
    with tarfile.open(os.path.join(ROOT, "tests", "golden", "gencode.tar.gz")) as t:
        t.extractall(d)
    return os.path.join(str(d), "gencode")


def runs(fixture):
    return [l.rstrip("\n").split("\t") for l in open(os.path.join(fixture, "RUNS"))]


def flag_kw(flags):
    """the reference's flag string -> keyword arguments of gencode_ref.extractorfs / translatenucs"""
    names = {"--min-length": "min_length", "--max-length": "max_length", "--max-gaps": "max_gaps", "--contig-start-mode": "contig_start_mode", "--contig-end-mode": "contig_end_mode",
             "--orf-start-mode": "orf_start_mode", "--translation-table": "table", "--translate": "translate", "--use-all-table-starts": "use_all_table_starts", "--add-orf-stop": "add_orf_stop"}
    kw, w = {}, flags.split()
    for k, v in zip(w[0::2], w[1::2]):
        if k in names:
            kw[names[k]] = int(v)
        elif k in ("--forward-frames", "--reverse-frames"):
            kw[k[2:].replace("-", "_")] = sum(1 << (int(f) - 1) for f in v.split(","))
        else:
            assert k in ("--id-offset", "--create-lookup"), k
    return kw


def same_files(fixture, name, entries, what):
    data, index = G.db_files(entries)
    assert open(os.path.join(fixture, name), "rb").read() == data, what
    assert open(os.path.join(fixture, name + ".index"), "rb").read() == index, what


def test_restatement_equals_every_db_of_the_fixture(fixture):
    reads = G.read_seqs(os.path.join(fixture, "in"))
    assert len(reads) >= 200 and max(len(s) for _, s in reads) <= 200
    seen = set()
    for name, module, src, dst, flags, status in runs(fixture):
        kw = flag_kw(flags)
        if status == "fail":
            assert kw["table"] in G.INVALID and not os.path.exists(os.path.join(fixture, dst))
            continue
        if module == "extractorfs":
            assert src == "in" and kw["table"] in G.TABLES
            orfs, hdrs = G.extractorfs(reads, **kw)
            same_files(fixture, dst, orfs, name)
            same_files(fixture, dst + "_h", hdrs, name + " headers")
        elif module == "translatenucs":
            add = kw.pop("add_orf_stop")
            aa = G.translatenucs(G.read_entries(os.path.join(fixture, src)), G.read_entries(os.path.join(fixture, src + "_h")) if add else None, add_orf_stop=bool(add), **kw)
            same_files(fixture, dst, aa, name)
        else:
            assert module == "concatdbs"
            a, b = (G.read_entries(os.path.join(fixture, s)) for s in src.split())
            same_files(fixture, dst, G.concat(a, b), name)
        seen.add((module, kw.get("table"), kw.get("use_all_table_starts"), kw.get("translate", 0)))
    # every accepted id, with and without the table's starts, with and without --translate; the four refused ids are in RUNS as "fail"
    for t in G.VALID:
        assert all(("extractorfs", t, s, tr) in seen for s in (0, 1) for tr in (0, 1)) and ("translatenucs", t, None, 0) in seen, t
    assert {flag_kw(r[4])["table"] for r in runs(fixture) if r[5] == "fail"} == set(G.INVALID)


def test_the_fixture_tells_the_tables_apart(fixture):
    """what makes the other tables other: stops that translate (27, 28, 31 end no ORF), table-specific stops, the eight starts of table 4"""
    n = {r[0]: sum(1 for _ in open(os.path.join(fixture, r[3] + ".index"))) for r in runs(fixture) if r[5] == "ok"}
    assert n["t27_s0_tr"] == n["t28_s0_tr"] == n["t31_s0_tr"] == 0 < n["t6_s0_tr"] < n["t1_s0_tr"] < n["t2_s0_tr"]
    assert n["t1_s0_orfs"] == n["t11_s0_orfs"] < n["t1_s1_orfs"] < n["t11_s1_orfs"] != n["t4_s1_orfs"] != n["t4_s0_orfs"]
    assert G.codons(27, True) == (set(), {"ATG"}) and len(G.codons(4, True)[1]) == 8 and len(G.codons(11, True)[1]) == 7 and len(G.codons(1, True)[1]) == 3
    lut1, lut6 = G.residue_lut(1), G.residue_lut(6)
    tar = (G.BASE[ord("T")] << 8) | (G.BASE[ord("A")] << 4) | G.BASE[ord("R")]
    assert chr(lut1[tar]) == "*" and chr(lut6[tar]) == "Q"


def test_gencode_info_states_the_same_tables():
    import plass_amd
    for t in G.VALID:
        assert plass_amd.gencode_info(t) == G.TABLES[t], t
    lib = plass_amd.load_library()
    res, sta = C.create_string_buffer(65), C.create_string_buffer(65)
    for t in tuple(G.INVALID) + (-1, 8, 18, 19, 20, 33, 1000):
        assert lib.gencode.plasship_gencode_info(t, res, sta) == ERR_ARG, t
        with pytest.raises(plass_amd.PlasshipError):
            plass_amd.gencode_info(t)
    assert lib.gencode.plasship_gencode_info(11, None, sta) == 0 and sta.value.decode() == G.TABLES[11][1]


def test_library_exports_the_new_entries():
    import plass_amd
    from plass_amd import _lib

    def exports(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
        return {l.split()[-1] for l in out.splitlines() if l.split()[-1].startswith("plasship_") and l.split()[-2] == "T"}

    new = {"plasship_extract_orfs_gc", "plasship_translate_nucs_gc", "plasship_gencode_info"}
    assert exports(plass_amd.gencode_lib_path()) == {s[0] for s in _lib.GENCODE_SYMBOLS} == new
    # the other five libraries' sets stay what their headers declare
    assert exports(plass_amd.lib_path()) == {s[0] for s in _lib.SYMBOLS + _lib.SYNTH_SYMBOLS + _lib.RCCL_SYMBOLS}
    assert exports(plass_amd.clust_lib_path()) == {s[0] for s in _lib.CLUST_SYMBOLS}
    assert exports(plass_amd.linclust_lib_path()) == {s[0] for s in _lib.LINCLUST_SYMBOLS}
    assert exports(plass_amd.subst_lib_path()) == {s[0] for s in _lib.SUBST_SYMBOLS}
    assert exports(plass_amd.cc_lib_path()) == {s[0] for s in _lib.CC_SYMBOLS}
    lib = plass_amd.load_library()
    ext = _lib.load_gencode_library()
    assert ext is lib.gencode and all(hasattr(ext, s) for s in new)
    header = open(os.path.join(ROOT, "include", "plasship_ext", "gencode.h")).read()
    assert all("int %s(" % s in header for s in new)
    assert hasattr(plass_amd.Context, "extractorfs_gencode") and hasattr(plass_amd.Context, "translatenucs_gencode")


def _cli(*args, level="1"):
    p = subprocess.run([CLI] + list(args), env=dict(os.environ, PLASSHIP_CLI_DRYRUN=level), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return p.returncode, p.stdout


START = "--min-length 20 --max-length 45 --max-gaps 0 --contig-start-mode 1 --contig-end-mode 0 --orf-start-mode 0 --forward-frames 1,2,3 --reverse-frames 1,2,3".split()
TAIL = "--translate 0 --id-offset 0 --create-lookup 0 --threads 4 --compressed 0 -v 3".split()


def test_command_lines_in_dry_run():
    # the workflows' calls with a table (data/assemble.sh:41-77), under the new names
    rc, out = _cli("extractorfs-gencode", "reads", "orfs", *START, "--translation-table", "4", "--use-all-table-starts", "0", *TAIL, level="2")
    assert rc == 96 and "extractorfs-gencode accepted (2 positional arguments" in out and "flag.translationTable 4\n" in out and "flag.allStarts 0\n" in out
    rc, out = _cli("extractorfs-gencode", "reads", "orfs", *START, "--translation-table", "11", "--use-all-table-starts", "1", *TAIL, level="2")
    assert rc == 96 and "flag.translationTable 11\n" in out and "flag.allStarts 1\n" in out
    rc, out = _cli("translatenucs-gencode", "orfs", "aa", "--translation-table", "4", "--add-orf-stop", "1", "-v", "3", "--compressed", "0", "--threads", "4", level="2")
    assert rc == 96 and "translatenucs-gencode accepted" in out and "flag.translationTable 4\n" in out and "flag.addOrfStop 1\n" in out
    for t in G.VALID:
        assert _cli("extractorfs-gencode", "a", "b", "--translation-table", str(t))[0] == 96 and _cli("translatenucs-gencode", "a", "b", "--translation-table", str(t))[0] == 96
    # an id the reference refuses is an error of the call, not a fall-back
    for t in G.INVALID:
        for mod in ("extractorfs-gencode", "translatenucs-gencode"):
            rc, out = _cli(mod, "a", "b", "--translation-table", str(t))
            assert rc == 1 and "Invalid translation table selected" in out, (mod, t)
    assert _cli("extractorfs-gencode", "a", "b", "--translation-table", "4", "--no-such-flag", "1")[0] == 1
    assert _cli("translatenucs-gencode", "a", "b", "--use-all-table-starts", "1")[0] == 1        # extractorfs' flag
    assert _cli("extractorfs-gencode", "a", "b", "--translation-table", "4", "--compressed", "1")[0] == 95
    # the chain drivers take the two flags, as the workflows do
    for driver, dbs in (("assemble-chain", ("reads", "out")), ("guidedassemble-chain", ("reads", "nucl", "aa"))):
        rc, out = _cli(driver, *dbs, "--translation-table", "4", "--num-iterations", "1", level="2")
        assert rc == 96 and "flag.translationTable 4\n" in out, driver
        rc, out = _cli(driver, *dbs, "--translation-table", "11", "--use-all-table-starts", "1", level="2")
        assert rc == 96 and "flag.translationTable 11\n" in out and "flag.allStarts 1\n" in out, driver
        rc, out = _cli(driver, *dbs, "--translation-table", "7")
        assert rc == 1 and "Invalid translation table selected" in out, driver
    assert _cli("nuclassemble-chain", "reads", "out", "--translation-table", "4")[0] == 1            # the nucleotide workflow translates nothing
    # the same flags on the reference's names answer what they answered (tests/golden/cli_dryrun_corpus.json: accepted by the parser; the
    # library then refuses another table, exit code 95)
    assert _cli("extractorfs", "reads", "orfs", *START, "--translation-table", "1", "--use-all-table-starts", "0", *TAIL)[0] == 96
    assert _cli("translatenucs", "s", "o", "--translation-table", "3")[0] == 96


def test_wrapper_routes_only_when_asked(tmp_path):
    ref = tmp_path / "ref"
    ref.write_text("#!/bin/bash\necho \"REF argv0=$0 args=$*\"\n")
    ref.chmod(0o755)
    log = tmp_path / "log"
    base = dict(os.environ, PLASSHIP_CLI_DRYRUN="1", PLASS_REF_BIN=str(ref), PLASS_WRAPPER_LOG=str(log))
    for v in ("PLASS_GPU_GENCODE", "PLASS_GPU_CLUST", "PLASS_GPU_CC", "PLASS_GPU_HAMMING", "PLASS_GPU_LOCAL", "PLASS_GPU_SUBST", "PLASS_GPU_REPSEQ"):
        base.pop(v, None)
    ex = ["extractorfs", "reads", "orfs"] + START + ["--translation-table", "4", "--use-all-table-starts", "0"] + TAIL
    tr = ["translatenucs", "orfs", "aa", "--translation-table", "4", "--add-orf-stop", "1"]

    def run(args, **env):
        return subprocess.run([WRAPPER] + args, env=dict(base, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)

    for call, mod in ((ex, "extractorfs-gencode"), (tr, "translatenucs-gencode")):
        out = run(call, PLASS_GPU_GENCODE="1")
        assert out.returncode == 0 and mod + " accepted" in out.stdout and "args=" + " ".join(call[:3]) in out.stdout, out.stdout
        # not opted in (unset, anything but 1, another module's switch): the call goes where it went
        for env in ({}, {"PLASS_GPU_GENCODE": "0"}, {"PLASS_GPU_CC": "1"}):
            out = run(call, **env)
            assert out.returncode == 0 and "gencode" not in out.stdout and "dry run: %s accepted" % call[0] in out.stdout, (env, out.stdout)
    out = run(tr + ["--no-such-flag", "1"], PLASS_GPU_GENCODE="1")
    assert out.returncode == 1 and "REF" not in out.stdout
    out = run(ex + ["--compressed", "1"], PLASS_GPU_GENCODE="1")             # 95 from the new command: on to the old one, whose 95 goes to the reference
    assert out.returncode == 0 and "accepted" not in out.stdout and "REF" in out.stdout
    out = run(["kmermatcher", "db", "pref", "-k", "22", "--kmer-per-seq", "60"], PLASS_GPU_GENCODE="1")
    assert "dry run: kmermatcher accepted" in out.stdout
    lines = log.read_text().splitlines()
    assert lines[0].startswith("GPU path   (dry run: extractorfs-gencode accepted, the reference computes) : extractorfs reads")
    assert sum(l.startswith("GPU path   (dry run: translatenucs-gencode accepted") for l in lines) == 1


def test_resume_is_refused_with_another_table(tmp_path):
    """chain.manifest records the two values; a --resume with other ones would splice two runs"""
    d = tmp_path / "inter"; d.mkdir()
    for s in ("", ".index", ".dbtype"):
        (tmp_path / ("in" + s)).write_bytes(b"x")
        (d / ("assembly_0" + s)).write_bytes(b"")
    (d / "assembly_0.done").write_bytes(b"")
    head = ("module assemble-chain\n-k 14\n--alph-size 13\n--kmer-per-seq 60\n--kmer-per-seq-scale 0\n--hash-shift 67\n--min-seq-id 0.899999976\n-e 1.0000000000000001e-05\n-c 0\n--cov-mode 0\n"
            "--min-aln-len 0\n--seq-id-mode 0\n--rescore-mode 3\n--ignore-multi-kmer 1\n--include-only-extendable 0\n--keep-target 1\n--max-seq-len 65535\n--chop-cycle 1\n--from-reads 0\n--single-end 0\n")
    base = ["assemble-chain", str(tmp_path / "in"), str(tmp_path / "asm"), "--write-intermediate", str(d), "--resume", "1"]
    (d / "chain.manifest").write_text(head)                    # a manifest from before the flags existed
    rc, out = _cli(*base)
    assert rc == 1 and ": --translation-table differs" in out, out
    (d / "chain.manifest").write_text(head + "--translation-table 1\n--use-all-table-starts 0\n")
    rc, out = _cli(*base, "--translation-table", "4")
    assert rc == 1 and ": --translation-table differs" in out and "4" in out, out
    rc, out = _cli(*base, "--use-all-table-starts", "1")
    assert rc == 1 and ": --use-all-table-starts differs" in out, out
    rc, out = _cli(*base)
    assert rc == 1 and ": inputs differs" in out, out           # both agree: the next key the file lacks
