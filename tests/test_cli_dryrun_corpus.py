"""`plass-hip`'s command-line parser against tests/golden/cli_dryrun_corpus.json, without a GPU: every recorded command line is run again
with PLASSHIP_CLI_DRYRUN=2 (parsed and validated; an accepted call prints one `flag.<member> <value>` line per parsed value) and has to
give the recorded exit code and the recorded output, byte for byte.  The corpus was written by the binary itself before its parser became
tables (tests/golden/make_cli_dryrun_corpus.py, which also holds the enumeration and the helper files the cases name)."""
import importlib.util
import os

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "plass_amd", "plass-hip")


def test_every_recorded_command_line_parses_as_recorded(tmp_path):
    spec = importlib.util.spec_from_file_location("make_cli_dryrun_corpus", os.path.join(GOLDEN, "make_cli_dryrun_corpus.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    cases = rec.load(os.path.join(GOLDEN, "cli_dryrun_corpus.json"))
    assert len(cases) > 1500 and [c["args"] for c in cases] == rec.enumerate_cases()      # the corpus is the whole enumeration, no case left out
    results = rec.run_all(EXE, os.path.realpath(str(tmp_path)), [c["args"] for c in cases])
    wrong = [(c, rc, out) for c, (rc, out) in zip(cases, results) if (rc, out) != (c["rc"], c["stdout"])]
    assert not wrong, "%d of %d cases differ, the first: %s\nrecorded (exit %d):\n%s\nnow (exit %d):\n%s" % (
        len(wrong), len(cases), " ".join(wrong[0][0]["args"]), wrong[0][0]["rc"], wrong[0][0]["stdout"], wrong[0][1], wrong[0][2])
    assert sorted(os.listdir(tmp_path)) == sorted([n + ".dbtype" for n in rec.HELPER_DBTYPES] + [rec.EXISTING])      # a dry run writes nothing
