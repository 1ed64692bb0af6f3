"""GPU tests of the genetic codes other than the standard one (`-m gpu`): plasship_extract_orfs_gc / plasship_translate_nucs_gc (libplasship_gencode.so)
against the DBs the unmodified reference wrote for every table (tests/golden/gencode.tar.gz), against the narrow entry points for the standard code,
against the sequential restatement (tests/tools/gencode_ref.py, itself pinned on that fixture by tests/test_gencode_host.py) on generated reads, and
`assemble-chain --translation-table` against the same steps called one by one.  Bit-exact."""
import os
import subprocess
import sys
import tarfile

import pytest

from conftest import assert_same_db, read_db

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gencode_ref as G  # noqa: E402
from test_gencode_host import flag_kw  # noqa: E402

pytestmark = pytest.mark.gpu
HIP = os.path.join(ROOT, "plass_amd", "plass-hip")


@pytest.fixture(scope="module")
def ctx():
    import plass_amd
    c = plass_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    d = tmp_path_factory.mktemp("gencode")
    with tarfile.open(os.path.join(ROOT, "tests", "golden", "gencode.tar.gz")) as t:
        t.extractall(d)
    return os.path.join(str(d), "gencode")


@pytest.fixture(scope="module")
def synth(ctx, tmp_path_factory):
    """20 000 generated reads of 150 nt, as a handle, as DB files and as the restatement's list"""
    import plass_amd
    reads, _ = ctx.synth_read_pairs(plass_amd.SynthParams(n_pairs=10000, seed=5, n_genomes=6, genome_min_len=40000, genome_max_len=90000, abundance_sigma=1.0))
    path = str(tmp_path_factory.mktemp("synth") / "reads")
    reads.write(path)
    return reads, path, G.read_seqs(path)


def orf_params(kw):
    import plass_amd
    frames = lambda m: ",".join(str(i + 1) for i in range(3) if m >> i & 1)      # noqa: E731
    p = {k: v for k, v in kw.items() if k not in ("table", "forward_frames", "reverse_frames", "translate", "use_all_table_starts")}
    return plass_amd.OrfParams(translation_table=kw["table"], use_all_table_starts=bool(kw.get("use_all_table_starts", 0)), translate=bool(kw.get("translate", 0)),
                               forward_frames=frames(kw.get("forward_frames", 7)), reverse_frames=frames(kw.get("reverse_frames", 7)), **p)


def write_entries(path, entries, dbtype):
    data, index = G.db_files(entries)
    open(path, "wb").write(data)
    open(path + ".index", "wb").write(index)
    open(path + ".dbtype", "wb").write(dbtype.to_bytes(4, "little"))


def same_as_files(got, want, what):
    """a DB this library wrote against one the reference wrote: dbtype and every entry under its key (conftest), the data file byte for byte and the
    index line for line (key, offset, length)"""
    assert_same_db(want, got, what)
    assert open(str(got), "rb").read() == open(str(want), "rb").read(), what
    assert [l.split()[:3] for l in open(str(got) + ".index", "rb")] == [l.split()[:3] for l in open(str(want) + ".index", "rb")], what


@pytest.mark.parametrize("table", G.VALID + list(G.INVALID))
def test_every_table_equals_the_reference(ctx, fixture, tmp_path, table):
    """extractorfs (with and without --translate 1, --use-all-table-starts 0 and 1), translatenucs (--add-orf-stop 0 and 1) and, for tables 4 and 11,
    the workflow's preprocessing: every DB of the fixture that was made with this table.  An id the reference refuses is an argument error"""
    import plass_amd
    reads = ctx.read_seqdb(os.path.join(fixture, "in"))
    mine = [r for r in (l.rstrip("\n").split("\t") for l in open(os.path.join(fixture, "RUNS"))) if r[1] != "concatdbs" and flag_kw(r[4])["table"] == table]
    assert len(mine) >= 6
    for name, module, src, dst, flags, status in mine:
        kw, out = flag_kw(flags), str(tmp_path / dst)
        if module == "extractorfs":
            if status == "fail":
                with pytest.raises(plass_amd.PlasshipError, match="invalid translation table"):
                    ctx.extractorfs_gencode(reads, orf_params(kw))
                continue
            orfs, hdr, st = ctx.extractorfs_gencode(reads, orf_params(kw))
            orfs.write(out); hdr.write(out + "_h")
            same_as_files(out, os.path.join(fixture, dst), name)
            same_as_files(out + "_h", os.path.join(fixture, dst + "_h"), name + " headers")
            assert st.n_out == hdr.count()
        else:
            orfs, hdr = ctx.read_seqdb(os.path.join(fixture, src)), ctx.read_orfhdr(os.path.join(fixture, src + "_h"))
            if status == "fail":
                with pytest.raises(plass_amd.PlasshipError, match="invalid translation table"):
                    ctx.translatenucs_gencode(orfs, hdr, add_orf_stop=bool(kw["add_orf_stop"]), translation_table=table)
            else:
                aa, _ = ctx.translatenucs_gencode(orfs, hdr if kw["add_orf_stop"] else None, add_orf_stop=bool(kw["add_orf_stop"]), translation_table=table)
                aa.write(out)
                same_as_files(out, os.path.join(fixture, dst), name)
                aa.free()
        for x in (orfs, hdr):
            x.free()
    for wf, t, s in (("wf11", 11, True), ("wf4", 4, False)):
        if t == table:       # data/assemble.sh:41-77 as one call
            frag = ctx.plass_fragments(reads, translation_table=t, use_all_table_starts=s)
            frag.write(tmp_path / wf)
            same_as_files(tmp_path / wf, os.path.join(fixture, wf + "_aa_6f_start_long"), wf)


def test_standard_code_equals_the_narrow_entry_points(ctx, golden, tmp_path):
    """table 1 with ATG through the new entry points: what plasship_extract_orfs / plasship_translate_nucs answer"""
    import plass_amd
    reads = ctx.read_seqdb(os.path.join(golden, "orf", "in_small"))
    for i, kw in enumerate((dict(), dict(orf_start_mode=0, min_length=1, max_gaps=3), dict(orf_start_mode=2, contig_start_mode=1, translate=True), plass_amd._lib.PLASS_ORFS_START)):
        a, ah, _ = ctx.extractorfs(reads, plass_amd.OrfParams(**kw))
        b, bh, _ = ctx.extractorfs_gencode(reads, plass_amd.OrfParams(**kw))
        for x, n in ((a, "a"), (ah, "a_h"), (b, "b"), (bh, "b_h")):
            x.write(str(tmp_path / f"{n}{i}"))
        same_as_files(tmp_path / f"b{i}", tmp_path / f"a{i}", f"extractorfs_gencode, table 1, {kw}")
        same_as_files(tmp_path / f"b_h{i}", tmp_path / f"a_h{i}", f"extractorfs_gencode headers, table 1, {kw}")
        if not kw.get("translate"):
            for stop in (False, True):
                x, _ = ctx.translatenucs(a, ah, add_orf_stop=stop); y, _ = ctx.translatenucs_gencode(b, bh, add_orf_stop=stop, translation_table=1)
                x.write(tmp_path / f"x{i}"); y.write(tmp_path / f"y{i}")
                same_as_files(tmp_path / f"y{i}", tmp_path / f"x{i}", f"translatenucs_gencode, table 1, add_orf_stop {stop}")
    # the narrow entry points keep refusing everything else
    with pytest.raises(plass_amd.PlasshipError):
        ctx.extractorfs(reads, plass_amd.OrfParams(use_all_table_starts=True))


@pytest.mark.parametrize("table,all_starts", [(4, False), (11, True), (27, False)])
def test_generated_reads_equal_the_restatement(ctx, synth, tmp_path, table, all_starts):
    """20 000 reads (more than one block per kernel, 150 nt: 19 eight-byte words per strand): ORF DB, header DB and the translation with
    --add-orf-stop 1, for ORFs of 20 codons and more, starts and stops of the table"""
    import plass_amd
    reads, _, seqs = synth
    kw = dict(min_length=20, max_gaps=0, orf_start_mode=0)
    want, want_h = G.extractorfs(seqs, table=table, use_all_table_starts=all_starts, **kw)
    want_aa = G.translatenucs(want, want_h, table=table, add_orf_stop=True)
    orfs, hdr, st = ctx.extractorfs_gencode(reads, plass_amd.OrfParams(translation_table=table, use_all_table_starts=all_starts, **kw))
    aa, _ = ctx.translatenucs_gencode(orfs, hdr, add_orf_stop=True, translation_table=table)
    assert st.n_out == len(want) > 20000
    for h, entries, name, dbtype in ((orfs, want, "orfs", 1), (hdr, want_h, "orfs_h", 12), (aa, want_aa, "aa", 0)):
        h.write(str(tmp_path / name)); write_entries(str(tmp_path / ("want_" + name)), entries, dbtype)
        same_as_files(tmp_path / name, tmp_path / ("want_" + name), "%s, table %d" % (name, table))
    if table == 27:          # no codon of this table ends an ORF: every ORF runs to the end of its read
        assert all(e.endswith(b"\t2\n") or e.endswith(b"\t3\n") for _, e in want_h)


def test_assemble_chain_with_a_table_equals_the_module_calls(ctx, synth, tmp_path):
    """assemble-chain from the read DB with --translation-table 4: the preprocessing with that table, then one iteration — the same steps on handles"""
    import plass_amd
    reads, path, _ = synth
    rs, asp = plass_amd.RescoreParams(min_seq_id=0.9), plass_amd.AssembleParams(min_seq_id=0.9)
    db = ctx.plass_fragments(reads, translation_table=4)
    std = ctx.plass_fragments(reads)
    assert db.download()[0] != std.download()[0]                # TGA is tryptophan here: other fragments than the standard code's
    kp = plass_amd.KmermatchParams(hash_shift=67, include_only_extendable=False)
    c, _ = ctx.kmermatcher(db, kp); a, _ = ctx.rescorediagonal(db, db, c, rs)
    db, _ = ctx.findassemblystart(db, a)
    c, _ = ctx.kmermatcher(db, kp); a, _ = ctx.rescorediagonal(db, db, c, rs)
    db, _ = ctx.assembleresults(db, a, asp)
    db.write(tmp_path / "want")
    p = subprocess.run([HIP, "assemble-chain", path, str(tmp_path / "got"), "--translation-table", "4", "--num-iterations", "1"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and "chain: 1 iterations" in p.stdout, p.stdout[-3000:]
    assert_same_db(tmp_path / "want", tmp_path / "got", "assemble-chain --translation-table 4")
    assert read_db(tmp_path / "got")[0] == 0
