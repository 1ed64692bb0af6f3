"""A PLASSHIP_TUNE_<x> that is no switch of this build is named on stderr, once per process, when a context is created (core.hip:
TUNE_NAMES); a kept switch is not.  Run in a child process: the report is made once per process, so in-process capture would depend on
which test created the first context."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_unknown_tune_name_is_reported_once():
    code = "import sys; sys.path.insert(0, %r)\nimport plass_amd\nfor _ in range(2):\n    plass_amd.Context(0).close()\nprint('CTX_OK')\n" % ROOT
    env = dict(os.environ, PLASSHIP_TUNE_ASM16="6", PLASSHIP_TUNE_KMCACHE="2")
    p = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, env=env)
    assert p.returncode == 0 and "CTX_OK" in p.stdout, p.stderr[-3000:]
    assert p.stderr.count("ASM16") == 1, p.stderr
    assert "[plasship] PLASSHIP_TUNE_ASM16 is not a switch of this build (ignored)" in p.stderr
    assert "KMCACHE" not in p.stderr, p.stderr
