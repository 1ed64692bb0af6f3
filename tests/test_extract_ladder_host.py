"""Host tests (`-m "not gpu"`) of the extraction ladders (tests/tools/extract_ladder.py): the conditions tests/test_gpu_extract_ladder.py
checks on the oracle's output before it compares a GPU result with it, on the oracle alone -- the oracle accepts every flag set, the ladders
hold a rung on every edge, and under the default flags every hand-over class is reached by sequences that have overlap partners."""
import os
import sys

import pytest

from conftest import ROOT, run_oracle

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import extract_ladder as X  # noqa: E402


def test_edges_are_rungs():
    """every length on an edge of the default flags, and its neighbours, is a rung"""
    k, kps = 14, 60
    Ls = set(X.ladder_lengths(False, k, kps, 0.0))
    for w in (1, 48, 49, kps - 1, kps, 64, 65, 96, 97, 128, 129, 192, 193, 256, 257, 992, 1024, 1025, 3072, 3073):
        assert {w + k - 1 + d for d in X.DELTAS} <= Ls
    assert {k - 1, k, k + 1, 127, 128, 129, 130, 8159, 8160, 8161, 8162, 9000} <= Ls
    Ln = set(X.ladder_lengths(True, 22, 60, 0.1))
    assert {8159, 8160, 8161, 8162, 12000} <= Ln and {256 + 21, 257 + 21, 1024 + 21, 1025 + 21, 3072 + 21, 3073 + 21} <= Ln
    # consideredRaw = 59 + 0.1 L crosses CAP 128, CAP48 512 and CAP2 1024 at L = 700, 4540 and 9660
    for L in (700, 4540, 9660):
        assert {L - 1, L, L + 1} <= Ln and int(X.considered_raw(L, 60, 0.1)) == 59 + L // 10 and int(X.considered_raw(L - 1, 60, 0.1)) == 58 + L // 10
    # the model of the launch chain the classes come from
    assert [X.tier_class(L, 14, 60, 0.0, False) for L in (61, 62, 128, 129, 269, 270, 1037, 1038, 3085, 3086, 8160, 8161)] == \
        ["short", "w256", "w256", "w256", "w256", "w1024", "w1024", "w3072", "w3072", "lds", "lds", "beyond"]
    assert X.tier_class(72, 14, 60, 0.0, False, multi=False) == "short" and X.tier_class(73, 14, 60, 0.0, False, multi=False) == "w256"
    assert [X.tier_class(L, 22, 60, 0.1, True) for L in (277, 278, 699, 700, 3093, 3094, 4539, 4540, 8160, 8161)] == \
        ["w256", "w1024", "w1024", "w3072", "w3072", "lds", "lds", "lds", "lds", "beyond"]
    assert not X.goes_to_scratch(9659, 22, 60, 0.1, True) and X.goes_to_scratch(9660, 22, 60, 0.1, True)


@pytest.mark.parametrize("name", sorted(X.CASES))
def test_ladder_conditions_on_the_oracle(oracle_bin, tmp_path, name):
    case = X.CASES[name]
    lad = X.case_ladder(case)
    assert lad.is_rung.sum() >= 180 and len(set(int(k) for k in lad.keys)) == len(lad.seqs)
    assert lad.lengths.sum() < (1 << 20)                                     # the ladders stay under 1 MB
    seq = lad.write(tmp_path / "seq")
    log = run_oracle(oracle_bin, ["kmermatcher", seq, tmp_path / "pref"] + X.oracle_flags(case))
    cov = X.check_conditions(lad, case, tmp_path / "pref", log)
    if name in ("default", "nucl_default"):
        assert cov is not None and set(X.expected_classes(case)) <= set(cov)
    # rungs that are queries with a candidate other than themselves: more than a hundred under the default flags
    pref = X.read_pref(tmp_path / "pref")
    rung_queries = sum(1 for k, r in zip(lad.keys, lad.is_rung) if r and pref[int(k)])
    if name == "default":
        assert rung_queries >= 100
    elif case["kps"] == 1:
        assert rung_queries == 0


def test_layout_switch_and_all_work_dbs(oracle_bin, tmp_path):
    case = X.CASES["default"]
    for L in (X.LAYOUT_SWITCH_L - 1, X.LAYOUT_SWITCH_L):
        lad = X.layout_switch_db(L)
        assert int(lad.lengths.max()) == L and int((lad.lengths == L).sum()) == 2
        seq = lad.write(tmp_path / ("sw%d" % L))
        log = run_oracle(oracle_bin, ["kmermatcher", seq, tmp_path / ("sw%d_pref" % L)] + X.oracle_flags(case))
        X.check_conditions(lad, case, tmp_path / ("sw%d_pref" % L), log, main=False)
        pref = X.read_pref(tmp_path / ("sw%d_pref" % L))
        assert all(pref[int(k)] for k, r in zip(lad.keys, lad.is_rung) if r)        # both rungs have partners
    a, b = X.all_work_dbs()
    assert int(X.windows(a.lengths, 14).max()) <= 59 and int(b.lengths.max()) == 300 and list(a.keys) == list(b.keys[:-1])
