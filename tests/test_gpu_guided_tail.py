"""GPU tests (`-m gpu`) of the workflows' --db-mode end: `plass-hip guidedassemble-chain --nuclassembly-out DB`
(data/guidedNuclAssemble.sh:135-170: the extended ORFs + the reads through `nuclassemble --db-mode 1`), `plass-hip nuclassemble-chain
--db-mode 1 --db-out DB` (data/nuclassemble.sh:138-176, 200-207) and plasship_subdb_write (Context.write_subdb, Context.guided_tail).

No golden holds `guided_assembly.merged` or `nuclassembly`, so the fused tail is pinned by composition: every module of the tail is run through
the plass-hip command line on DB files (each of them pinned on reference-written DBs by tests/test_gpu_parity.py and friends), and every awk /
ln / cat / mv line of the two scripts between the modules is restated here on the .index files, with the script line next to it.  Every
comparison is exact."""
import os
import shutil
import subprocess
import tarfile
import time

import numpy as np
import pytest

from conftest import NUCL_AS, NUCL_KM, NUCL_RS, ROOT, assert_same_db

pytestmark = pytest.mark.gpu
HIP = os.path.join(ROOT, "plass_amd", "plass-hip")
EXAMPLE = [os.path.join(ROOT, "tests", "golden", "example_reads", "reads_%d.fastq.gz" % i) for i in (1, 2)]

# The guided loop runs 2 iterations (what tests/test_gpu_chain_cli.py runs) and the nested nuclassemble NUCL_IT = 2: the smallest count at
# which an iteration starts from the `_noneCycle` DB of the one before, the script's chaining (on these reads it also finds circular
# contigs, so PREV_CYCLE_ALL and the concatdbs --preserve-keys of nuclassemble.sh:145 are on the path).  With so few iterations the bundled
# example reads (2 x 150 nt pairs) grow no contig beyond the workflow's --min-contig-len 1000 (the longest is 823 nt), so BOTH sides run with
# MIN_LEN instead: the fused driver gets `--min-contig-len MIN_LEN`, the replay's awk filter thr = MIN_LEN.  The test asserts that this
# threshold splits the contigs of the module-by-module side (0 < kept < total).
NUCL_IT = 2
MIN_LEN = 300
EXTRACTORFS_LONG = ["--min-length", "45", "--max-length", "32734", "--max-gaps", "0", "--contig-start-mode", "2", "--contig-end-mode", "2", "--orf-start-mode", "0"]
EXTRACTORFS_START = ["--min-length", "20", "--max-length", "45", "--max-gaps", "0", "--contig-start-mode", "1", "--contig-end-mode", "0", "--orf-start-mode", "0"]
CYCLECHECK = ["--max-seq-len", "200000", "--chop-cycle", "1"]


def hip(args, ok=0):
    p = subprocess.run([HIP] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == ok, p.stdout[-3000:]
    return p.stdout


def chain_seconds(out, what):
    """a figure of the driver's `chain:` line, e.g. `nuclassembly (2 iterations) 0.123s`"""
    line = [l for l in out.splitlines() if l.startswith("chain:")][-1]
    return float(line.split(what)[1].split("s")[0].split()[-1])


# ---- the scripts' glue on .index files --------------------------------------------------------------------------------------------
def index_lines(db):
    return [l.rstrip("\n") for l in open(str(db) + ".index")]


def write_lines(path, lines):
    with open(str(path), "w") as f:
        f.write("".join(l + "\n" for l in lines))


def awk_join(first, second):
    """awk 'NR == FNR { f[$1] = $0; next } $1 in f { print f[$1], $0 }' first second"""
    f = {l.split()[0]: l for l in first}
    return [f[l.split()[0]] + " " + l for l in second if l.split()[0] in f]


def awk_gt_3_6(lines):
    """awk '$3 > $6 { print }'   (numeric strings compare as numbers)"""
    return [l for l in lines if int(l.split()[2]) > int(l.split()[5])]


def link_db(src, dst, index=True):
    """ln -s <src> <dst>; ln -s <src>.dbtype <dst>.dbtype [; ln -s <src>.index <dst>.index]"""
    os.symlink(str(src), str(dst)); os.symlink(str(src) + ".dbtype", str(dst) + ".dbtype")
    if index:
        os.symlink(str(src) + ".index", str(dst) + ".index")


def createsubdb_mode0(order_lines, db, out):
    """`createsubdb <list> <db> <out> --subdb-mode 0` (lib/mmseqs/src/util/createsubdb.cpp:41-92): the listed entries copied in list order,
    under their keys; the dbtype file is the DB's.  (A list that is not ascending would have its index sorted on close: the lists here are.)"""
    data = open(str(db), "rb").read()
    ent = {l.split()[0]: (int(l.split()[1]), int(l.split()[2])) for l in index_lines(db)}
    keys = [int(l.split()[0]) for l in order_lines]
    assert keys == sorted(keys)
    blob, idx = b"", []
    for l in order_lines:
        k = l.split()[0]
        o, n = ent[k]
        idx.append("%s\t%d\t%d" % (k, len(blob), n))
        blob += data[o:o + n]
    open(str(out), "wb").write(blob)
    write_lines(str(out) + ".index", idx)
    shutil.copy(str(db) + ".dbtype", str(out) + ".dbtype")


def same_files(a, b, names=("", ".index", ".dbtype")):
    for s in names:
        x, y = open(str(a) + s, "rb").read(), open(str(b) + s, "rb").read()
        assert x == y, "%s%s differs from %s%s (%d / %d bytes)" % (a, s, b, s, len(x), len(y))


def nuclassemble_db_mode_replay(T, merged, thr, only_extended=True):
    """data/nuclassemble.sh with DB_MODE, module by module in the directory T -> (OUT_FILE, PREV_CYCLE_ALL or None, kept, total)"""
    inp = source = str(merged)                                                     # :73,91  INPUT="$1"; SOURCE=${INPUT}
    prev_cycle_all = None
    for step in range(NUCL_IT):                                                    # :97  while [ $STEP -lt $NUM_IT ]
        hip(["kmermatcher", inp, T / ("pref_%d" % step)] + NUCL_KM)                # :103
        hip(["rescorediagonal", inp, inp, T / ("pref_%d" % step), T / ("aln_%d" % step)] + NUCL_RS)      # :113
        asm = T / ("assembly_%d" % step)
        hip(["nuclassembleresults", inp, T / ("aln_%d" % step), asm] + NUCL_AS)    # :123
        hip(["cyclecheck", asm, str(asm) + "_cycle"] + CYCLECHECK)                 # :23  (the function cyclecheck, :19-61, called at :132)
        none_cycle = str(asm) + "_noneCycle"
        if os.path.getsize(str(asm) + "_cycle") > 0:                               # :27  if [ -s "${1}_cycle" ]
            cyc = {l.split()[0] for l in index_lines(str(asm) + "_cycle")}         # :30-31  awk 'NR==FNR { a[$1]=$0; next } !($1 in a) {print $0}'
            write_lines(none_cycle + ".index", [l for l in index_lines(asm) if l.split()[0] not in cyc])
            link_db(asm, none_cycle, index=False)                                  # :32-33
            cycle_all = str(asm) + "_cycle_all"
            if prev_cycle_all is None:                                             # :38  mvdb "${1}_cycle" "${1}_cycle_all"
                for s in ("", ".index", ".dbtype"):
                    os.rename(str(asm) + "_cycle" + s, cycle_all + s)
            else:                                                                  # :41
                hip(["concatdbs", prev_cycle_all, str(asm) + "_cycle", cycle_all, "--preserve-keys"])
        else:                                                                      # :45-47
            link_db(asm, none_cycle)
        if os.path.exists(str(asm) + "_cycle_all") and os.path.getsize(str(asm) + "_cycle_all") > 0:     # :54-56
            prev_cycle_all = str(asm) + "_cycle_all"
        inp = none_cycle                                                           # :59,134  PREV_ASSEMBLY="${1}_noneCycle"; INPUT="${PREV_ASSEMBLY}"
    result = str(T / ("assembly_%d" % (NUCL_IT - 1)))                              # :138
    if prev_cycle_all is not None:                                                 # :140-146
        result = str(T / "assembly_merged")
        hip(["concatdbs", inp, prev_cycle_all, result, "--preserve-keys"])
    if only_extended:                                                              # :155-156
        only = awk_gt_3_6(awk_join(index_lines(result), index_lines(source)))
    else:                                                                          # :160  cat "${RESULT}.index"
        only = index_lines(result)
    filtered = [l for l in only if int(l.split()[2]) > thr + 1]                    # :166  awk -v thr="${MIN_CONTIG_LEN}" '$3 > (thr+1) { print }'
    createsubdb_mode0(filtered, result, T / "assembly")                            # :171
    if prev_cycle_all is not None:                                                 # :174  awk 'NR == FNR { f[$1] = $0; next } $1 in f { print $0 }'
        f = {l.split()[0] for l in index_lines(prev_cycle_all)}
        write_lines(T / "assembly_cycle.index", [l for l in index_lines(T / "assembly") if l.split()[0] in f])
    out = T / "OUT_FILE"
    for s in ("", ".index", ".dbtype"):                                            # :201  mvdb "${TMP_PATH}/assembly" "$OUT_FILE"
        os.rename(str(T / "assembly") + s, str(out) + s)
    if os.path.exists(T / "assembly_cycle.index"):                                 # :204-205
        os.rename(T / "assembly_cycle.index", str(out) + "_cycle.index")
    return out, prev_cycle_all, len(filtered), len(index_lines(result))


@pytest.fixture(scope="module")
def guided_run(tmp_path_factory):
    """the fused driver on the bundled pairs, once for the tests of this file"""
    W = tmp_path_factory.mktemp("guided_tail")
    t0 = time.time()
    out = hip(["guidedassemble-chain"] + EXAMPLE + [W / "nucl", W / "aa", "--num-iterations", "aa:2,nucl:%d" % NUCL_IT, "--nuclassembly-out", W / "out",
               "--min-contig-len", MIN_LEN])
    return W, out, time.time() - t0


def test_guided_tail_equals_modules_one_by_one(guided_run, tmp_path):
    W, stdout, wall = guided_run
    T = tmp_path
    # what the workflow has on disk when its loop ends: the reads, nucl_6f_start_long and the last assembly_nucl_<i> (the driver's first output)
    hip(["mergereads"] + EXAMPLE + [T / "nucl_reads"])                                                        # guidedNuclAssemble.sh:32
    hip(["extractorfs", T / "nucl_reads", T / "nucl_6f_long"] + EXTRACTORFS_LONG)                             # :54
    hip(["extractorfs", T / "nucl_reads", T / "nucl_6f_start"] + EXTRACTORFS_START)                           # :48
    hip(["concatdbs", T / "nucl_6f_long", T / "nucl_6f_start", T / "nucl_6f_start_long"])                      # :59
    result_nucl = W / "nucl"                                                                                  # :132  RESULT_NUCL
    t0 = time.time()
    # :136-139  the `_only_assembled` index
    only = awk_gt_3_6(awk_join(index_lines(result_nucl), index_lines(T / "nucl_6f_start_long")))
    write_lines(T / "assembly_nucl_only_assembled.index", only)
    n_result = len(index_lines(result_nucl))
    assert 0 < len(only) < n_result
    os.symlink(str(result_nucl), str(T / "assembly_nucl_only_assembled"))                                      # :142
    os.symlink(str(result_nucl) + ".dbtype", str(T / "assembly_nucl_only_assembled.dbtype"))                   # :146
    hip(["concatdbs", T / "assembly_nucl_only_assembled", T / "nucl_reads", T / "guided_assembly.merged"])     # :163
    # :169  nuclassemble guided_assembly.merged nuclassembly tmp ${NUCL_ASM_PAR}   (--db-mode 1)
    N = T / "nuclassembly_tmp"; N.mkdir()
    want, cyc_all, kept, total = nuclassemble_db_mode_replay(N, T / "guided_assembly.merged", MIN_LEN)
    replay = time.time() - t0
    lens = sorted(int(l.split()[2]) - 2 for l in index_lines(want))
    print("guided tail on the example reads: %d of %d ORFs extended; merged DB %d entries; %d of %d contigs kept at --min-contig-len %d (longest %s); "
          "circular: %s" % (len(only), n_result, len(index_lines(T / "guided_assembly.merged")), kept, total, MIN_LEN, lens[-3:], cyc_all is not None))
    print([l for l in stdout.splitlines() if l.startswith(("chain:", "guided tail:", "db-mode:"))])
    print("timing (one run each, nothing depends on it): fused tail %.3f s of the driver's %.3f s wall; module-by-module replay of the tail %.3f s"
          % (chain_seconds(stdout, "nuclassembly (%d iterations)" % NUCL_IT), wall, replay))
    assert 0 < kept < total          # a condition on the input: the threshold keeps some contigs and drops others
    same_files(W / "out", want)
    assert os.path.exists(str(W / "out") + "_cycle.index") == (cyc_all is not None)
    if cyc_all is not None:
        same_files(W / "out", want, names=("_cycle.index",))
    for s in ("_h", "_h.index", ".fasta"):                                         # db-mode writes no header DB and no FASTA file
        assert not os.path.exists(str(W / "out") + s)


def test_python_guided_tail_equals_the_driver(guided_run, tmp_path):
    """Context.guided_tail on handles chained by the per-module calls: the driver's DB"""
    import plass_amd
    from test_gpu_parity import gd_km_params, gd_rs_params
    W, _, _ = guided_run
    with plass_amd.Context(0) as ctx:
        reads, hdr, _ = ctx.mergereads(EXAMPLE)
        hdr.free()
        source, aa = ctx.penguin_guided_inputs(reads)
        nu = source
        for it in range(2):
            c, _ = ctx.kmermatcher(aa, gd_km_params()); a, _ = ctx.rescorediagonal(aa, aa, c, gd_rs_params())
            na, _ = ctx.proteinaln2nucl(nu, aa, a)
            nu2, aa2, _ = ctx.guidedassembleresults(nu, aa, na)
            na.free(); a.free(); c.free(); aa.free()
            if nu is not source:
                nu.free()
            nu, aa = nu2, aa2
        ss, ds = ctx.guided_tail(nu, source, reads, tmp_path / "py", num_iterations=NUCL_IT, min_contig_len=MIN_LEN)
        assert ds.n_entries == ss.n_selected > 0
        for x in (nu, aa, source, reads):
            x.free()
    same_files(W / "out", tmp_path / "py")
    assert os.path.exists(str(tmp_path / "py") + "_cycle.index") == os.path.exists(str(W / "out") + "_cycle.index")


# ---- the selection rule and the gather ---------------------------------------------------------------------------------------------
def upload(ctx, seqs, keys):
    ent = [s + b"\n\0" for s in seqs]
    elen = np.array([len(e) for e in ent], dtype=np.uint32)
    off = np.zeros(len(ent), dtype=np.uint64)
    if len(ent) > 1:
        off[1:] = np.cumsum(elen[:-1], dtype=np.uint64)
    return ctx.upload_seqdb(b"".join(ent), off, elen, np.asarray(keys, dtype=np.uint32), 1)


def seq(n, salt):
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[(np.arange(n) * 7 + salt + np.arange(n) // 5) % 4])


def expected_subdb(r_seqs, r_keys, s_seqs, s_keys, cyc_keys):
    """the awk rule of guidedNuclAssemble.sh:136-139 on the two indices (entry length = sequence + 2), then createsubdb --subdb-mode 0 and
    the cycle filter of nuclassemble.sh:174"""
    o = np.argsort(r_keys, kind="stable")                    # an index is written in key order
    rl = ["%d\t0\t%d" % (r_keys[i], len(r_seqs[i]) + 2) for i in o]
    so = np.argsort(s_keys, kind="stable")
    sl = ["%d\t0\t%d" % (s_keys[i], len(s_seqs[i]) + 2) for i in so]
    kept = [int(l.split()[0]) for l in awk_gt_3_6(awk_join(rl, sl))]
    by_key = dict(zip(r_keys, r_seqs))
    blob, idx, cyc = b"", [], []
    for k in kept:
        e = by_key[k] + b"\n\0"
        line = "%d\t%d\t%d\n" % (k, len(blob), len(e))
        idx.append(line)
        if cyc_keys is not None and k in set(cyc_keys):
            cyc.append(line)
        blob += e
    return kept, blob, "".join(idx).encode(), "".join(cyc).encode()


def check_select(ctx, tmp_path, name, r_seqs, r_keys, s_seqs, s_keys, cyc_keys=None):
    r = upload(ctx, r_seqs, r_keys); s = upload(ctx, s_seqs, s_keys)
    c = upload(ctx, [b"A"] * len(cyc_keys), cyc_keys) if cyc_keys is not None else None
    sel, st = ctx.select_contigs(r, s, "nucleotide", only_extended=True, min_contig_len=0)
    out = tmp_path / name
    ds = ctx.write_subdb(sel, out, cycles=c)
    kept, blob, idx, cyc = expected_subdb(r_seqs, r_keys, s_seqs, s_keys, cyc_keys)
    print("%s: %d of %d kept, %d bytes, gather %.3f ms" % (name, len(kept), len(r_keys), len(blob), ds.ms_kernel))
    assert st.n_selected == len(kept) == ds.n_entries and ds.bytes == len(blob)
    assert open(out, "rb").read() == blob, name
    assert open(str(out) + ".index", "rb").read() == idx, name
    assert open(str(out) + ".dbtype", "rb").read() == (1).to_bytes(4, "little")
    assert os.path.exists(str(out) + "_cycle.index") == (cyc_keys is not None)
    if cyc_keys is not None:
        assert open(str(out) + "_cycle.index", "rb").read() == cyc and ds.n_cycle == cyc.count(b"\n")
    sel.free(); r.free(); s.free()
    if c is not None:
        c.free()
    return kept


def test_guided_select_rule(tmp_path):
    import plass_amd
    # RESULT: 42 entries under non-contiguous keys, each with what SOURCE holds under its key: nothing ("missing"), a sequence shorter by one
    # or half as long (kept: `$3 > $6`), an equal or a longer one (dropped).  Sequence lengths around the entry lengths 255 / 256 / 65 535, one
    # entry of 70 000 bytes kept and one dropped, lengths that are and are not multiples of 16; the first and the last entry are dropped
    plan = [(0, "missing"), (1, "shorter"), (13, "half"), (14, "equal"), (15, "shorter"), (16, "longer"), (17, "half"), (30, "shorter"), (31, "equal"), (32, "half"),
            (33, "missing"), (46, "shorter"), (47, "half"), (48, "longer"), (62, "shorter"), (63, "equal"), (64, "half"), (100, "missing"), (150, "shorter"), (252, "half"),
            (253, "shorter"), (253, "equal"), (254, "shorter"), (254, "longer"), (255, "half"), (256, "shorter"), (300, "missing"), (1009, "shorter"), (1022, "half"),
            (1024, "equal"), (4096, "shorter"), (65532, "shorter"), (65533, "shorter"), (65533, "equal"), (65534, "half"), (65535, "shorter"), (65535, "longer"),
            (65536, "missing"), (69998, "shorter"), (69998, "equal"), (777, "longer"), (500, "equal")]
    lens = [n for n, _ in plan]
    assert 69998 + 2 == 70000 and len(plan) == 42
    r_keys = [3 * i + (i % 2) for i in range(len(plan))]
    r_seqs = [seq(n, i) for i, n in enumerate(lens)]
    s_keys, s_seqs = [], []
    for k, (n, how) in zip(r_keys, plan):
        if how != "missing":
            s_keys.append(k); s_seqs.append(b"A" * {"shorter": n - 1, "half": n // 2, "equal": n, "longer": n + 1}[how])
    s_keys += [2, 5000, 5001]; s_seqs += [b"", b"ACGT", b"A" * 300]            # keys RESULT does not hold
    assert not set(s_keys[-3:]) & set(r_keys)
    want_kept = [k for k, (n, how) in zip(r_keys, plan) if how in ("shorter", "half")]
    with plass_amd.Context(0) as ctx:
        kept = check_select(ctx, tmp_path, "mixed", r_seqs, r_keys, s_seqs, s_keys)
        assert kept == want_kept and 0 < len(kept) < len(r_keys) and r_keys[0] not in kept and r_keys[-1] not in kept
        # the same with circular keys: some kept, some dropped, one unknown to RESULT
        check_select(ctx, tmp_path, "mixed_cycles", r_seqs, r_keys, s_seqs, s_keys, cyc_keys=sorted([kept[0], kept[-1], r_keys[0], 999999]))
        check_select(ctx, tmp_path, "no_cycle_selected", r_seqs, r_keys, s_seqs, s_keys, cyc_keys=[r_keys[0]])
        # RESULT uploaded in another order: the handle is key-ordered whatever the input order
        p = np.random.default_rng(3).permutation(len(lens))
        assert check_select(ctx, tmp_path, "shuffled", [r_seqs[i] for i in p], [r_keys[i] for i in p], s_seqs, s_keys) == kept
        # every entry kept (SOURCE empty sequences under every key; an empty RESULT sequence is not longer than an empty SOURCE one: lens > 0 here)
        nz = [i for i, n in enumerate(lens) if n > 0]
        allk = check_select(ctx, tmp_path, "all", [r_seqs[i] for i in nz], [r_keys[i] for i in nz], [b""] * len(nz), [r_keys[i] for i in nz])
        assert len(allk) == len(nz)
        # nothing kept: SOURCE holds the same lengths; and no common key at all
        assert check_select(ctx, tmp_path, "none", r_seqs, r_keys, [b"A" * n for n in lens], r_keys, cyc_keys=[r_keys[1]]) == []
        assert check_select(ctx, tmp_path, "disjoint", r_seqs, r_keys, [b""], [1000000]) == []


# ---- nuclassemble-chain --db-mode 1 --------------------------------------------------------------------------------------------------
def parse_fasta(path):
    """[(rank, len, cycle or None, sequence)] of a file plasship_fasta_write / convert2fasta wrote: ">rank len:L[ cycle:c]" + one sequence line"""
    rec = []
    lines = open(path, "rb").read().split(b"\n")
    assert lines[-1] == b""
    for h, s in zip(lines[0:-1:2], lines[1:-1:2]):
        assert h.startswith(b">")
        f = h[1:].split()
        cyc = int(f[2].split(b":")[1]) if len(f) > 2 else None
        rec.append((int(f[0]), int(f[1].split(b":")[1]), cyc, s))
    return rec


def db_mode_inputs(golden, tmp_path):
    with tarfile.open(os.path.join(ROOT, "tests", "golden", "fasta_tail_reads.tar.gz")) as t:
        t.extractall(tmp_path)
    R = tmp_path / "fasta_tail" / "reads"
    return {"seq_0": ([os.path.join(golden, "nucl", "seq_0")], ["--num-iterations", "3", "--min-contig-len", "300"]),
            "seq_0_all": ([os.path.join(golden, "nucl", "seq_0")], ["--num-iterations", "2", "--min-contig-len", "200", "--contig-output-mode", "0"]),
            "circular": ([R / "circ_1.fastq.gz", R / "circ_2.fastq.gz"], [])}          # fasta_tail_case3: 153 circular contigs among the selected


@pytest.mark.parametrize("case", ["seq_0", "seq_0_all", "circular"])
def test_nuclassemble_chain_db_mode(case, golden, tmp_path):
    inp, flags = db_mode_inputs(golden, tmp_path)[case]
    hip(["nuclassemble-chain"] + inp + [tmp_path / "a_f"] + flags + ["--fasta-out", tmp_path / "f.fasta"])
    out = hip(["nuclassemble-chain"] + inp + [tmp_path / "a_d"] + flags + ["--db-mode", "1", "--db-out", tmp_path / "d"])
    same_files(tmp_path / "a_f", tmp_path / "a_d")                                  # the positional output is the same either way
    fa = parse_fasta(tmp_path / "f.fasta")
    idx = [tuple(int(x) for x in l.split()) for l in index_lines(tmp_path / "d")]
    data = open(tmp_path / "d", "rb").read()
    print(case, [l for l in out.splitlines() if l.startswith("db-mode:")], "FASTA records", len(fa))
    assert len(fa) == len(idx) > 0
    assert [k for k, _, _ in idx] == sorted(k for k, _, _ in idx)
    pos = 0
    for (rank, L, cyc, s), (k, o, n) in zip(fa, idx):
        assert o == pos and n == L + 2 and data[o:o + n] == s + b"\n\0", (rank, k)
        pos += n
    assert pos == len(data)
    assert open(str(tmp_path / "d") + ".dbtype", "rb").read() == (1).to_bytes(4, "little")
    # `_cycle.index`: exactly the contigs the FASTA header marks circular, as their lines of the index; the file exists when the FASTA has the field
    has_cycle = fa[0][2] is not None
    assert os.path.exists(str(tmp_path / "d") + "_cycle.index") == has_cycle
    if has_cycle:
        want = ["%d\t%d\t%d" % e for e, r in zip(idx, fa) if r[2] == 1]
        assert index_lines(str(tmp_path / "d") + "_cycle") == want
    if case == "circular":
        assert has_cycle and sum(r[2] for r in fa) > 0
    for s in ("_h", "_h.index", ".fasta"):
        assert not os.path.exists(str(tmp_path / "d") + s)


def test_db_mode_with_fasta_out_is_refused(golden, tmp_path):
    out = hip(["nuclassemble-chain", os.path.join(golden, "nucl", "seq_0"), tmp_path / "a", "--db-mode", "1", "--fasta-out", tmp_path / "f.fasta"], ok=1)
    assert "--fasta-out" in out and "Time for processing" not in out
    out = hip(["nuclassemble-chain", os.path.join(golden, "nucl", "seq_0"), tmp_path / "a", "--db-mode", "1", "--db-out", tmp_path / "d", "--fasta-out", tmp_path / "f.fasta"], ok=1)
    assert os.listdir(tmp_path) == []


# ---- nothing changes without the flag ----------------------------------------------------------------------------------------------
def test_without_flag_nothing_changes(golden, tmp_path):
    """guidedassemble-chain on the golden read DB, 2 iterations: the two DBs tests/test_gpu_chain_cli.py expects (the per-module calls on the
    same inputs), byte for byte the same files with and without --nuclassembly-out"""
    import plass_amd
    from test_gpu_parity import gd_km_params, gd_rs_params
    s = os.path.join(golden, "nucl", "seq_0")
    with plass_amd.Context(0) as ctx:
        reads = ctx.read_seqdb(s)
        nu, aa = ctx.penguin_guided_inputs(reads)
        for it in range(2):
            c, _ = ctx.kmermatcher(aa, gd_km_params()); a, _ = ctx.rescorediagonal(aa, aa, c, gd_rs_params())
            na, _ = ctx.proteinaln2nucl(nu, aa, a)
            nu, aa, _ = ctx.guidedassembleresults(nu, aa, na)
        nu.write(tmp_path / "e_gn"); aa.write(tmp_path / "e_ga")
    plain = hip(["guidedassemble-chain", s, tmp_path / "gn", tmp_path / "ga", "--num-iterations", "2"])
    flagged = hip(["guidedassemble-chain", s, tmp_path / "gn2", tmp_path / "ga2", "--num-iterations", "aa:2,nucl:1", "--nuclassembly-out", tmp_path / "out",
                   "--min-contig-len", MIN_LEN])
    assert "Time for processing" in plain and "Time for processing" in flagged
    assert "nuclassembly" not in plain and "db-mode:" not in plain and "db-mode:" in flagged
    assert_same_db(tmp_path / "e_gn", tmp_path / "gn", "guidedassemble-chain, nucleotide ORFs")
    assert_same_db(tmp_path / "e_ga", tmp_path / "ga", "guidedassemble-chain, protein twins")
    same_files(tmp_path / "gn", tmp_path / "gn2")
    same_files(tmp_path / "ga", tmp_path / "ga2")
    made = sorted(os.listdir(tmp_path))
    assert [f for f in made if f.startswith("out")] == ["out", "out.dbtype", "out.index"] + (["out_cycle.index"] if os.path.exists(tmp_path / "out_cycle.index") else [])
    assert not [f for f in made if f.startswith("gn_") or f.startswith("gn2_")]      # no <o>_cycle_<i> next to the guided outputs
