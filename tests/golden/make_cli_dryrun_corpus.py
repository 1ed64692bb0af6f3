#!/usr/bin/env python3
"""tests/golden/cli_dryrun_corpus.json: what `plass-hip` makes of a command line, recorded from the binary itself with PLASSHIP_CLI_DRYRUN=2
(no GPU: an accepted call prints the "accepted" line and one `flag.<member> <value>` line per parsed value, a refused one its refusal).
tests/test_cli_dryrun_corpus.py replays every case against the built binary, so a change to the parser that moves a value, a refusal, an
exit code or the order of two refusals shows.  Deterministic; resume and manifest cases are not here (their output holds absolute paths
and mtimes: tests/test_chain_resume_host.py).
    python3 make_cli_dryrun_corpus.py <plass-hip> [<out.json>]      (default: cli_dryrun_corpus.json next to this script)

The file holds {args, rc, stdout} of every case, written compactly (as plain text it would be several MB): load() gives them back in full and
record() checks that it does.  Paths under the scratch directory read TMP/... in args and output.
  "baseline": {module: [dump line, ...]}     the dump of the module's first accepted case
  "stdout":   [text, ...]                    every distinct output before the dump lines
  "cases":    [[call, [[rest, rc, i, dump], ...]], ...]    consecutive cases whose command lines start with the same words `call` (the module and
              its positionals); a case's command line is shlex.split(call + " " + rest), its output stdout[i] and then, unless `dump` is null, the
              module's baseline with the members in `dump` ({member: value}) replaced"""
import glob
import itertools
import json
import os
import shlex
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
TMP = "TMP"
HELPER_DBTYPES = {"aa": 0, "nucl": 1, "aln": 5, "hdr": 12}      # TMP/<name>.dbtype, what concatdbs probes before the dry-run exit
EXISTING = "exists.out"                                          # TMP/exists.out: an output that exists already

COMMON = ["--threads", "-v", "--compressed"]
ASM = ["--min-seq-id", "--max-seq-len", "--keep-target", "--rescore-mode"]
CHAIN = ["--num-iterations", "--write-intermediate", "--from-reads", "-k", "--alph-size", "--kmer-per-seq", "--kmer-per-seq-scale", "--min-seq-id", "-e", "-c",
         "--cov-mode", "--max-seq-len", "--keep-target", "--hash-shift", "--ignore-multi-kmer", "--rescore-mode", "--min-aln-len", "--seq-id-mode", "--single-end", "--resume"]
# module -> (positionals, flags that make the bare call an accepted one, the flags it owns)
MODULES = {
    "kmermatcher": (["s", "p"], ["-k", "14", "--kmer-per-seq", "60"],
                    ["--sub-mat", "--alph-size", "--min-seq-id", "--kmer-per-seq", "--spaced-kmer-mode", "--spaced-kmer-pattern", "--kmer-per-seq-scale", "--adjust-kmer-len",
                     "--mask", "--mask-lower-case", "--cov-mode", "-k", "-c", "--max-seq-len", "--hash-shift", "--split-memory-limit", "--include-only-extendable",
                     "--ignore-multi-kmer"]),
    "rescorediagonal": (["q", "t", "p", "o"], ["--rescore-mode", "3"],
                        ["--sub-mat", "--rescore-mode", "--wrapped-scoring", "--filter-hits", "-e", "-c", "-a", "--cov-mode", "--min-seq-id", "--min-aln-len", "--seq-id-mode",
                         "--add-self-matches", "--sort-results", "--db-load-mode"]),
    "assembleresults": (["s", "a", "o"], [], ASM),
    "nuclassembleresults": (["s", "a", "o"], [], ASM),
    "guidedassembleresults": (["n", "a", "aln", "on", "oa"], [], ASM),
    "proteinaln2nucl": (["n", "n", "a", "a", "aln", "o"], [], ["--sub-mat", "--gap-open", "--gap-extend"]),
    "findassemblystart": (["s", "a", "o"], [], []),
    "cyclecheck": (["s", "o"], [], ["--max-seq-len", "--chop-cycle"]),
    "extractorfs": (["s", "o"], [], ["--min-length", "--max-length", "--max-gaps", "--contig-start-mode", "--contig-end-mode", "--orf-start-mode", "--forward-frames",
                                     "--reverse-frames", "--translation-table", "--translate", "--use-all-table-starts", "--id-offset", "--create-lookup"]),
    "translatenucs": (["s", "o"], [], ["--translation-table", "--add-orf-stop"]),
    "concatdbs": (["a", "b", "o"], [], ["--preserve-keys", "--take-larger-entry"]),
    "assemble-chain": (["in", "asm"], [], CHAIN + ["--fasta-out", "--filter-proteins", "--protein-filter-threshold"]),
    "nuclassemble-chain": (["in", "asm"], [], CHAIN + ["--chop-cycle", "--fasta-out", "--min-contig-len", "--contig-output-mode", "--db-mode", "--db-out"]),
    "guidedassemble-chain": (["in", "nucl", "aa"], [], CHAIN + ["--nuclassembly-out", "--chop-cycle", "--min-contig-len", "--contig-output-mode"]),
    "createdb-reads": (["r.fastq", "o"], [], ["--shuffle", "--id-offset", "--dbtype", "--createdb-mode", "--write-lookup"]),
    "mergereads": (["r1.fastq", "r2.fastq", "o"], [], []),
}
BOOLS = {"-a", "--add-self-matches", "--wrapped-scoring", "--filter-hits", "--include-only-extendable", "--ignore-multi-kmer", "--keep-target", "--chop-cycle", "--adjust-kmer-len",
         "--use-all-table-starts", "--add-orf-stop", "--preserve-keys", "--take-larger-entry", "--db-mode", "--shuffle"}
# typical values; every other flag takes "3"
VALUES = {
    "--sub-mat": ["blosum62.out", "/share/nucleotide.out", "VTML80.out", "aa:blosum62.out,nucl:nucleotide.out", "nucl:/m/nucleotide.out,aa:/m/blosum62.out",
                  "aa:VTML80.out,nucl:nucleotide.out", "aa:blosum62.out,nucl:other.out", "nucl:nucleotide.out", "aa:blosum62.out"],
    "--min-seq-id": ["0.9", "0"], "-c": ["0.8", "0"], "-e": ["1e-05", "0.001"], "--kmer-per-seq-scale": ["0.100", "0"],
    "--forward-frames": ["1,2,3", "2", "1,4", ""], "--reverse-frames": ["1,2,3", "3,1", "0", ""],
    "--spaced-kmer-pattern": ["", "1101"], "--max-seq-len": ["200000", "65535"], "--id-offset": ["0", "7", "4294967294", "4294967295"],
    "--dbtype": ["0", "1", "2", "3"], "--write-intermediate": [TMP + "/wi"], "--fasta-out": [TMP + "/f.fasta"], "--db-out": [TMP + "/d"],
    "--nuclassembly-out": [TMP + "/n"], "--protein-filter-threshold": ["0.2"], "--num-iterations": ["3", "0"], "-k": ["14", "0"],
}
FLOATS = {"--min-seq-id", "-c", "-e", "--kmer-per-seq-scale", "--protein-filter-threshold"}
for b in BOOLS:
    VALUES[b] = ["1", "false", "2", "-1"]                         # ("-1" starts with '-': the flag toggles and -1 is a positional)
FOREIGN = ["--no-such-flag", "--fasta-out", "--rescore-mode", "-a", "--shuffle", "--num-iterations", "-k", "--id-offset", "--db-mode", "--min-seq-id", "--add-orf-stop"]


def enumerate_cases():
    cases = []
    add = lambda *a: cases.append([str(x) for x in a])
    # 1. the calls the unmodified workflows make (tools/workflow_dropin_check.sh's routing logs: what went to plass-hip, accepted or answered with 95)
    for log in sorted(glob.glob(os.path.join(HERE, "..", "..", "profiles", "r05_workflow_dropin", "*.routing.log"))):
        for line in open(log):
            if line.startswith("GPU path") or "plass-hip exit" in line:
                add(*line.split(" : ", 1)[1].split())
    # 2. every module: every flag it owns in every form, and a few it does not own
    for mod, (pos, base, flags) in MODULES.items():
        call = [mod] + pos + base
        add(*call)
        for fl in flags + COMMON:
            aa, nu = ("0.5", "0.25") if fl in FLOATS else ("7", "9")
            for v in VALUES.get(fl, ["3"]) + ["aa:%s,nucl:%s" % (aa, nu), "nucl:%s" % nu]:
                add(*call, fl, v)
            add(*call, fl)                                       # bare, the last token
            add(*call, fl, "--threads", "4")                     # bare, before another flag
        for fl in [x for x in FOREIGN if x not in flags][:3]:
            add(*call, fl, "1")
            add(*call, fl)
    # 3. tests/test_host.py::test_cli_exit_codes_separate_unsupported_from_failed
    P = lambda n: TMP + "/" + n
    for c in (["rescorediagonal", "q", "t", "p", "o", "--rescore-mode", "0", "--wrapped-scoring", "1", "-e", "0.001", "--min-seq-id", "0.9"],
              ["rescorediagonal", "q", "t", "p", "o", "--rescore-mode", "3", "--filter-hits", "1"],
              ["kmermatcher", "s", "p", "--kmer-per-seq", "21", "--mask", "1", "-k", "14"], ["kmermatcher", "s", "p", "--kmer-per-seq", "21"],
              ["linclust", "a", "b", "c"], ["clust", "a", "b", "c"],
              ["rescorediagonal", "q", "t", "p", "o", "--rescore-mode", "3", "-e", "1e-5", "--min-seq-id", "0.9", "-c", "0", "--threads", "4"],
              ["kmermatcher", "s", "p", "-k", "22", "--kmer-per-seq", "60", "--alph-size", "nucl:5,aa:13", "--spaced-kmer-mode", "0", "--mask", "0",
               "--sub-mat", "nucl:nucleotide.out,aa:blosum62.out", "--cov-mode", "1", "-c", "0.99", "--min-seq-id", "0.97"],
              ["kmermatcher", "s", "p", "-k", "14", "--kmer-per-seq", "60", "--no-such-flag", "1"],
              ["concatdbs", "a", "b", "c", "--preserve-keys"], ["concatdbs", "a", "b", "c", "--take-larger-entry"],
              ["proteinaln2nucl", "qn", "tn", "qa", "ta", "aln", "out"], ["proteinaln2nucl", "n", "n", "a", "a", "aln", "out"],
              ["proteinaln2nucl", "n", "n", "qa", "ta", "aln", "out"], ["proteinaln2nucl", "qn", "tn", "a", "a", "aln", "out"], []):
        add(*c)
    for ty in HELPER_DBTYPES:
        for extra in ([], ["--preserve-keys"], ["--preserve-keys", "0"], ["--take-larger-entry"], ["--preserve-keys", "--take-larger-entry", "1"]):
            add("concatdbs", P(ty), P(ty), P("o"), *extra)
    add("concatdbs", P(EXISTING), P("aa"), P("o"))               # a .dbtype that is not there
    add("concatdbs", P("aln"), P("aln"))                         # the probe looks at three positionals only
    # 4. the outputs of the chains
    opt = lambda flag, vals: [[]] + [[flag] + ([v] if v is not None else []) for v in vals]
    single = opt("--single-end", ["1"])
    for fo, dm, do, com, se in itertools.product(opt("--fasta-out", [P("f.fasta"), P(EXISTING)]), opt("--db-mode", ["1", None]), opt("--db-out", [P("d"), P(EXISTING)]),
                                                 opt("--contig-output-mode", ["0", "2"]), single):
        add("nuclassemble-chain", "in", "asm", *fo, *do, *com, *se, *dm)       # (a bare --db-mode last: it toggles)
    for fo, fp, se in itertools.product(opt("--fasta-out", [P("f.fasta"), P(EXISTING)]), opt("--filter-proteins", ["0", "1"]), single):
        add("assemble-chain", "in", "asm", *fo, *fp, *se)
    for no, com, ni, se in itertools.product(opt("--nuclassembly-out", [P("n"), P(EXISTING)]), opt("--contig-output-mode", ["0", "2"]),
                                             opt("--num-iterations", ["aa:3,nucl:0", "nucl:2", "aa:0"]), single):
        add("guidedassemble-chain", "in", "nucl", "aa", *no, *com, *ni, *se)
    add("guidedassemble-chain", "r1.fastq.gz", "r2.fastq.gz", "nucl", "aa", "--num-iterations", "aa:2,nucl:3", "-k", "aa:14,nucl:22", "--min-seq-id", "aa:0.97,nucl:0.99",
        "--min-aln-len", "aa:30,nucl:100", "--nuclassembly-out", P("n"), "--min-contig-len", "500", "--contig-output-mode", "1", "--chop-cycle", "1")
    add("assemble-chain", "in", "asm", "-k", "aa:14,nucl:22")    # not a MultiParam here: 0, accepted
    # 5. read files as positionals: FASTQ pairs, odd counts, stdin, .bz2
    files = ["a_1.fastq", "a_2.fastq.gz", "b_1.fastq", "b_2.fastq", "c.fasta"]
    for mod in ("assemble-chain", "nuclassemble-chain", "guidedassemble-chain"):
        outs = MODULES[mod][0][1:]
        for n in range(0, 6):
            for se in single:
                add(mod, *files[:n], *outs, *se)
        for bad in ("stdin", "x.fastq.bz2", "bz2", ".bz2"):
            for se in single:
                add(mod, "a_1.fastq", bad, *outs, *se)
                add(mod, bad, *outs, *se)
        add(mod, *outs[1:])
        add(mod)
    for n in range(0, 6):
        add("mergereads", *files[:n], "o")
        add("createdb-reads", *files[:n], "o")
        add("createdb-reads", *files[:n], "o", "--dbtype", "2", "--shuffle", "0", "--id-offset", "100")
    for bad in ("stdin", "x.fastq.bz2"):
        add("mergereads", "a_1.fastq", bad, "o")
        add("mergereads", bad, "a_2.fastq", "b_1.fastq", "b_2.fastq", "o")
        add("createdb-reads", bad, "o")
        add("createdb-reads", "a_1.fastq", bad, "o", "--dbtype", "1")
    for extra in (["--createdb-mode", "1"], ["--write-lookup", "0"], ["--write-lookup", "2", "--createdb-mode", "1"], ["--dbtype", "-1"], ["--dbtype", "1", "--id-offset", "4294967295"],
                  ["--id-offset", "-1"], ["--id-offset", "4294967295", "--write-lookup", "0"]):
        add("createdb-reads", "r.fastq", "o", *extra)
    # 6. a token that starts with '-' and a digit is a positional: behind a bool flag it leaves the flag without a value, behind another it is the value
    add("rescorediagonal", "q", "t", "p", "o", "--rescore-mode", "3", "-a", "-1", "-c", "-0.5", "-e", "-1e-3")
    add("rescorediagonal", "q", "t", "p", "o", "--rescore-mode", "3", "--add-self-matches", "-0", "-a")
    add("kmermatcher", "s", "p", "-k", "14", "--kmer-per-seq", "60", "--ignore-multi-kmer", "-3", "--include-only-extendable", "-2", "--hash-shift", "-5")
    add("kmermatcher", "-7", "s", "p", "-k", "-14", "--kmer-per-seq", "60")
    add("cyclecheck", "s", "o", "--chop-cycle", "-1", "--max-seq-len", "-1")
    add("nuclassemble-chain", "in", "asm", "--db-mode", "-1", "--db-out", P("d"), "--keep-target", "-9")
    add("assemble-chain", "in", "asm", "--keep-target", "-1", "--num-iterations", "-2")
    seen, out = set(), []
    for c in cases:
        if tuple(c) not in seen:
            seen.add(tuple(c))
            out.append(c)
    return out


def prepare(scratch):
    """the helper files the cases name: .dbtype files of four types and one existing output"""
    for name, ty in HELPER_DBTYPES.items():
        with open(os.path.join(scratch, name + ".dbtype"), "wb") as f:
            f.write(ty.to_bytes(4, "little"))
    with open(os.path.join(scratch, EXISTING), "wb"):
        pass


def run_case(exe, scratch, args):
    """-> (rc, stdout) of one call at dry-run level 2, run in the scratch directory, its name replaced by TMP"""
    real = [a.replace(TMP + "/", scratch + "/") for a in args]
    env = dict(os.environ, PLASSHIP_CLI_DRYRUN="2")
    p = subprocess.run([exe] + real, cwd=scratch, env=env, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return p.returncode, p.stdout.replace(scratch, TMP)


def split_dump(stdout):
    """-> (the text before the dump, ["member value", ...] or None)"""
    lines = stdout.split("\n")
    first = next((i for i, l in enumerate(lines) if l.startswith("flag.")), None)
    if first is None:
        return stdout, None
    assert lines[-1] == "" and all(l.startswith("flag.") for l in lines[first:-1]), stdout
    return "\n".join(lines[:first] + [""]), [l[len("flag."):] for l in lines[first:-1]]


def call_of(args):
    """the words before the first flag: the module and its positionals"""
    n = next((i for i, a in enumerate(args) if len(a) > 1 and a[0] == "-" and not a[1].isdigit()), len(args))
    return args[:n]


def load(path):
    """-> [{"args", "rc", "stdout"}], every case in full"""
    corpus, cases = json.load(open(path)), []
    for call, group in corpus["cases"]:
        for rest, rc, i, dump in group:
            args = shlex.split(call + " " + rest)
            out = corpus["stdout"][i]
            if dump is not None:
                out += "".join("flag.%s %s\n" % (m, dump.get(m, v)) for m, v in (l.split(" ", 1) for l in corpus["baseline"][args[0]]))
            cases.append({"args": args, "rc": rc, "stdout": out})
    return cases


def run_all(exe, scratch, cases):
    prepare(scratch)
    with ThreadPoolExecutor(8) as pool:
        return list(pool.map(lambda args: run_case(exe, scratch, args), cases))


def record(exe, path):
    cases = enumerate_cases()
    with tempfile.TemporaryDirectory() as scratch:
        results = run_all(exe, os.path.realpath(scratch), cases)
    baseline, texts, groups = {}, {}, []
    for args, (rc, stdout) in zip(cases, results):
        head, dump = split_dump(stdout)
        if dump is not None:
            base = baseline.setdefault(args[0], dump)
            assert [l.split(" ", 1)[0] for l in base] == [l.split(" ", 1)[0] for l in dump]
            dump = dict(l.split(" ", 1) for l, b in zip(dump, base) if l != b)
        call = shlex.join(call_of(args))
        if not groups or groups[-1][0] != call:
            groups.append([call, []])
        groups[-1][1].append([shlex.join(args[len(call_of(args)):]), rc, texts.setdefault(head, len(texts)), dump])
    dumps = lambda x: json.dumps(x, separators=(",", ":"))
    with open(path, "w") as f:
        f.write("{\n\"made_by\":%s,\n\"baseline\":{\n%s\n},\n\"stdout\":[\n%s\n],\n\"cases\":[\n%s\n]\n}\n" % (
            dumps("tests/golden/make_cli_dryrun_corpus.py: plass-hip itself, PLASSHIP_CLI_DRYRUN=2"), ",\n".join("%s:%s" % (dumps(m), dumps(l)) for m, l in baseline.items()),
            ",\n".join(dumps(t) for t in texts), ",\n".join(dumps(g) for g in groups)))
    back = load(path)
    assert [(c["args"], c["rc"], c["stdout"]) for c in back] == [(a, rc, out) for a, (rc, out) in zip(cases, results)], "the file does not give the cases back"
    return back


if __name__ == "__main__":
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "cli_dryrun_corpus.json")
    rcs = [c["rc"] for c in record(os.path.abspath(sys.argv[1]), path)]
    print("%d cases: %s -> %s" % (len(rcs), ", ".join("%d x exit %d" % (rcs.count(r), r) for r in sorted(set(rcs))), path))
