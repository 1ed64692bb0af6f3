"""plasship_mergereads on hand-made read pairs at every kernel edge (run with `-m gpu` on an MI355X).

The pairs are the rungs of tests/tools/merge_ladder.py; what they must give was decided by the reference's own FLASH
(tests/golden/mergereads_ladder.tar.gz: make_mergereads_ladder.sh, oracle/tools/flash_pin.cpp) and not by a restatement.  Per rung,
`plass-hip mergereads` and Context.mergereads must write the fixture's entries under keys 0 .. n-1 and the mate names as the header DB;
the whole ladder in one call must give the same DBs whatever PLASSHIP_MERGE_BATCH is (1, 15, 16, 17, 64: a pair for the wave kernel
first, last and alone in a batch, pair counts that are no multiple of 16 or 4), and as two file pairs the keys continue.  That every rung
reaches its edge is tests/test_merge_ladder_host.py (CPU).

14 rungs, 296 pairs, a fixture of 125 KiB.  On an MI355X this file's 35 tests take about 9 s together (the slowest, the hand-over rung
through the command line, 1.6 s; every other under 0.5 s) beside 16.4 s for test_mergereads_synthetic_against_the_checker in the same run.

Defects found: none, on either side: mergecheck.py and the kernels write what FLASH writes for every pair.

Mutations tried on scratch copies of mergereads.hip (none committed), each once through this module on an MI355X; the 7 tests of the
whole ladder fail with every mutation that changes a result (counted below):
  - `rem >= 4` changed to `rem > 4`: 17 fail (overlap_len, threshold, mask, ties_keys, quality: every overlap that is a multiple of 4);
  - the `& ~un` dropped from `mm`: 11 fail (n_rule, writer);
  - `key <= best` for the tie, in both kernels: 13 fail (ties_repeat, ties_keys, long_mates);
  - `MIN_OVERLAP` 14: 11 fail (overlap_len, n_rule);
  - `MAX_OVERLAP` 64: 9 fail (ties_keys).  No single overlap can tell 64 from 65, since no count m has m / 64 > 0.10f >= m / 65; the pair
    `score_len_65_decides_between_two_offsets` (6 / 65 < 5 / 54 < 6 / 64) was added for it after a first ladder let this mutation pass;
  - `qx >= qy` in the writer: 21 fail (batch_slots, mask, n_rule, ties_keys, quality, writer, long_mates);
  - `y == 'N'` changed to `x == 'N'`: 13 fail (n_rule, writer, long_mates);
  - `l1 < MR_MAX_SMALL` in place of `<=`, in the kernel and in the host's big list: nothing fails, and nothing should: the two kernels
    compute the same key for every pair, the constant only says which of them does; the hand-over rungs make sure each sees both sides;
  - `S1[w1 + 1]` not zeroed: nothing fails, and nothing can: the highest word read is S1[base + k + 1] with base + k + 1 <=
    (i >> 2) + ((l1 - i + 3) >> 2) = (l1 - (i & 3) + 3) >> 2 <= w1, so S1[w1 + 1] is never read, and the bytes of S1[w1] lie at positions
    >= l1, which `vm` masks out of `mm`, `un` and the quality sum.
None of the nine reads out of bounds (shorter loops, other comparisons, or LDS words inside the row's own array)."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT, assert_same_db, read_db

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import merge_ladder as L  # noqa: E402

pytestmark = pytest.mark.gpu
HIP = os.path.join(ROOT, "plass_amd", "plass-hip")
NAMES = [r[0] for r in L._RUNGS]


def run(args, env=None):
    p = subprocess.run([HIP] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120,
                       env=dict(os.environ, **(env or {})))
    assert p.returncode == 0 and "Time for processing" in p.stdout, p.stdout[-3000:]
    return p.stdout


@pytest.fixture(scope="module")
def ctx():
    import plass_amd
    c = plass_amd.Context(0)
    yield c
    c.close()


class _Ladder:
    """the fixture unpacked once: per rung and for the whole ladder the two FASTQ paths and the DBs FLASH expects"""

    def __init__(self, d):
        self.fx = L.fixture()
        assert list(self.fx) == NAMES
        self.rung = {n: self._put(d, n, [n]) for n in NAMES}
        self.whole = self._put(d, "whole", NAMES)
        self.halves = [self._put(d, "half%d" % k, part) for k, part in enumerate((NAMES[:6], NAMES[6:]))]

    def _put(self, d, tag, names):
        paths = [str(d / ("%s_%d.fastq" % (tag, m + 1))) for m in (0, 1)]
        for m in (0, 1):
            with open(paths[m], "wb") as f:
                f.write(b"".join(self.fx[n][m] for n in names))
        seqs, hdrs, comb, pairs = [], [], 0, 0
        for n in names:
            s, h, c = L.expected_dbs(*self.fx[n])
            seqs += s; hdrs += h; comb += c; pairs += len(self.fx[n][2])
        return paths, seqs, hdrs, comb, pairs


@pytest.fixture(scope="module")
def ladder(tmp_path_factory):
    return _Ladder(tmp_path_factory.mktemp("merge_ladder"))


def check_against(out, seqs, hdrs, what):
    t, ent = read_db(out)
    assert t == 1 and sorted(ent) == list(range(len(seqs))), "%s: keys are not 0 .. n-1" % what
    bad = [k for k in range(len(seqs)) if ent[k] != seqs[k] + b"\0"]
    assert not bad, "%s: %d entries differ (keys %s), first:\n%r\n%r" % (what, len(bad), bad[:10], ent[bad[0]][:400], seqs[bad[0]][:400])
    th, hent = read_db(str(out) + "_h")
    assert th == 12 and sorted(hent) == list(range(len(hdrs))), "%s: header keys are not 0 .. n-1" % what
    bad = [k for k in range(len(hdrs)) if hent[k] != hdrs[k] + b"\0"]
    assert not bad, "%s: %d header entries differ, first key %d: %r %r" % (what, len(bad), bad[0], hent[bad[0]], hdrs[bad[0]])


@pytest.mark.parametrize("name", NAMES)
def test_rung_cli_against_flash(ladder, tmp_path, name):
    paths, seqs, hdrs, comb, pairs = ladder.rung[name]
    out = run(["mergereads"] + paths + [tmp_path / "r"])
    check_against(tmp_path / "r", seqs, hdrs, name)
    assert "combined: %d " % comb in out, out


@pytest.mark.parametrize("name", NAMES)
def test_rung_context_against_flash(ctx, ladder, tmp_path, monkeypatch, name):
    monkeypatch.delenv("PLASSHIP_MERGE_BATCH", raising=False)
    paths, seqs, hdrs, comb, pairs = ladder.rung[name]
    reads, hdr, st = ctx.mergereads(paths)
    reads.write(tmp_path / "r"); hdr.write(str(tmp_path / "r") + "_h")
    check_against(tmp_path / "r", seqs, hdrs, name)
    assert (st.pairs, st.combined, st.not_combined) == (pairs, comb, pairs - comb)
    assert reads.info()["n"] == len(seqs) and hdr.info()["dbtype"] == 12
    reads.free(); hdr.free()


@pytest.fixture(scope="module")
def unbatched(ladder, tmp_path_factory):
    d = tmp_path_factory.mktemp("merge_ladder_whole")
    paths, seqs, hdrs, comb, _ = ladder.whole
    out = run(["mergereads"] + paths + [d / "w"])
    check_against(d / "w", seqs, hdrs, "the whole ladder in one batch")
    assert "combined: %d " % comb in out, out
    return str(d / "w")


@pytest.mark.parametrize("batch", [1, 15, 16, 17, 64])
def test_whole_ladder_in_batches(ladder, unbatched, tmp_path, batch):
    paths, seqs, hdrs, comb, _ = ladder.whole
    out = run(["mergereads"] + paths + [tmp_path / "b"], env={"PLASSHIP_MERGE_BATCH": str(batch)})
    check_against(tmp_path / "b", seqs, hdrs, "the whole ladder, batches of %d" % batch)
    assert "combined: %d " % comb in out, out
    assert_same_db(unbatched, tmp_path / "b", "the whole ladder, batches of %d against one batch" % batch)
    assert_same_db(unbatched + "_h", str(tmp_path / "b") + "_h", "the whole ladder's header DB, batches of %d against one batch" % batch)


@pytest.mark.parametrize("batch", [None, 17])
def test_two_file_pairs_keys_continue(ctx, ladder, unbatched, tmp_path, monkeypatch, batch):
    if batch:
        monkeypatch.setenv("PLASSHIP_MERGE_BATCH", str(batch))
    else:
        monkeypatch.delenv("PLASSHIP_MERGE_BATCH", raising=False)
    (pa, _, _, ca, na), (pb, _, _, cb, nb) = ladder.halves
    _, seqs, hdrs, comb, pairs = ladder.whole
    assert (ca + cb, na + nb) == (comb, pairs)
    reads, hdr, st = ctx.mergereads(pa + pb)
    reads.write(tmp_path / "t"); hdr.write(str(tmp_path / "t") + "_h")
    check_against(tmp_path / "t", seqs, hdrs, "the ladder as two file pairs")
    assert (st.pairs, st.combined, st.not_combined) == (pairs, comb, pairs - comb)
    assert_same_db(unbatched, tmp_path / "t", "the ladder as two file pairs against one")
    reads.free(); hdr.free()
