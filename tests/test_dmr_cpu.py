"""The region (DMR) pass on a host without a GPU: the numpy restatement
(tests/dmr_model.py) against the hand-worked example, the statistics of its
sticky generator, `hygeia get_dmrs`' flag handling, and the argument checks of
hyg_dmr_* (HYG_EINVAL with a message naming the entry, before any device is
touched; HYG_EDEVICE for valid arguments without a device)."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from hygeia_amd import _lib
from tests import dmr_model as dm

STICKY_CASES = dm.STICKY_CASES


# ------------------------------------------------------------ the restatement
def _example():
    pos = np.array([100, 110, 120, 500, 510, 520, 530, 2000], dtype=np.int64)
    D = np.array([[int(ch) for ch in row] for row in
                  ("1110", "1100", "1111", "1011", "0001", "1110", "1101", "1111")], dtype=np.int8)
    return pos, D


def test_hand_worked_example():
    pos, D = _example()
    c = D.sum(axis=1)
    assert list(c) == [3, 2, 4, 3, 1, 3, 3, 4]
    reg = dm.find_regions(c, pos, 2, 300, 2)
    assert reg.tolist() == [[0, 3], [5, 7]]
    assert dm.region_counts(D, reg, 2, 3).tolist() == [[2, 3], [2, 2]]
    assert dm.region_sums(c.reshape(-1, 1), reg).tolist() == [[9], [6]]
    assert dm.region_counts(D, reg, 1, 2).tolist() == [[2, 3], [2, 4]]
    # sites 3 and 7 are seed sites cut off by gaps of 380 and 1470: single-site runs
    assert dm.find_regions(c, pos, 2, 300, 1).tolist() == [[0, 3], [3, 4], [5, 7], [7, 8]]


def test_restatement_edges():
    c = np.array([5, 5, 5, 5, 5])
    # a restart of the positions (non-positive difference) never links
    assert dm.find_regions(c, np.array([10, 20, 20, 5, 9]), 1, 100, 1).tolist() == [[0, 2], [2, 3], [3, 5]]
    assert dm.find_regions(c, np.array([10, 20, 30, 40, 50]), 6, 100, 1).shape == (0, 2)
    assert dm.find_regions(c, np.array([10, 20, 30, 40, 50]), 0, 10, 1).tolist() == [[0, 5]]
    assert dm.find_regions(c, np.array([10, 20, 30, 40, 50]), 0, 0, 1).tolist() == [[i, i + 1] for i in range(5)]
    D = np.ones((5, 3), dtype=np.int8)
    assert dm.region_counts(D, np.array([[0, 5]]), 0, 1).tolist() == [[3, 3]]


@pytest.mark.parametrize("T,P", list(STICKY_CASES))
def test_sticky_generator_statistics(T, P):
    """The generator gives regions that are neither empty nor full, so a kernel
    that returned 0 or P everywhere could not pass the GPU comparison."""
    r_ctrl, r_case, pos = dm.sticky_trajectories(T, P, 6, STICKY_CASES[(T, P)])
    assert r_ctrl.shape == r_case.shape == (T, P) and pos.shape == (T,)
    assert r_ctrl.min() >= 0 and r_case.min() >= 0 and r_ctrl.max() < 6 and r_case.max() < 6
    assert set(np.unique(np.diff(pos))) <= {2, 10, 40, 200, 900} and pos[0] > 10_000
    D = r_ctrl != r_case
    c = D.sum(axis=1)
    for min_sites in (1, 3):
        reg = dm.find_regions(c, pos, dm.min_count(0.5, P), 300, min_sites)
        cnt = dm.region_counts(D, reg, 4, 5)
        n, longest = len(reg), int((reg[:, 1] - reg[:, 0]).max())
        mid = float(((cnt[:, 0] > 0) & (cnt[:, 0] < P)).mean())
        differ = float((cnt[:, 0] != cnt[:, 1]).mean())
        print(T, P, min_sites, n, longest, mid, differ)
        assert 40 <= n <= 116
        assert 56 <= longest <= 77
        assert 0.94 <= mid <= 1.0
        assert 0.25 <= differ <= 0.91


# ------------------------------------------------------------------ flags
@pytest.mark.parametrize("P", [1, 3, 50, 250])
@pytest.mark.parametrize("tau", [0.0, 0.5, 1 / 3, 1.0])
def test_min_count_from_site_prob(P, tau):
    from hygeia_amd import dmr

    c = dmr.min_count_of(tau, P)
    assert c == dm.min_count(tau, P)
    assert 0 <= c <= P + 1 and c / P >= tau and (c == 0 or (c - 1) / P < tau)


def test_min_count_values():
    from hygeia_amd import dmr

    assert [dmr.min_count_of(0.5, P) for P in (1, 3, 50, 250)] == [1, 2, 25, 125]
    assert [dmr.min_count_of(1 / 3, P) for P in (1, 3, 50, 250)] == [1, 1, 17, 84]
    assert [dmr.min_count_of(1.0, P) for P in (1, 3, 50, 250)] == [1, 3, 50, 250]
    assert [dmr.min_count_of(0.0, P) for P in (1, 3, 50, 250)] == [0, 0, 0, 0]


def test_min_fraction_parsing():
    from hygeia_amd import cli, dmr

    assert dmr.parse_min_fraction("0.8") == Fraction(4, 5)
    assert dmr.parse_min_fraction("4/5") == Fraction(4, 5)
    assert dmr.parse_min_fraction("1") == Fraction(1, 1)
    assert dmr.parse_min_fraction("0") == Fraction(0, 1)
    assert dmr.parse_min_fraction("0.125") == Fraction(1, 8)
    assert dmr.parse_min_fraction("0.999") == Fraction(999, 1000)
    for bad in ("0.8001", "1/1001", "1.5", "-0.1", "x", "1/0"):
        with pytest.raises(cli.FlagError):
            dmr.parse_min_fraction(bad)


def test_min_fraction_flag_error_exits_1(tmp_path, capsys):
    from hygeia_amd import cli

    rc = cli.main(["get_dmrs", "--results_dir", str(tmp_path), "--output_dir", str(tmp_path / "o"),
                   "--min_fraction", "0.12345"])
    assert rc == 1
    assert "min_fraction" in capsys.readouterr().err


def test_get_dmrs_is_a_command():
    from hygeia_amd import cli, dmr

    assert "get_dmrs" in cli.COMMANDS.split() and "get_dmrs" in cli._SUBCOMMANDS
    assert cli._SUBCOMMANDS["get_dmrs"][:2] == ("dmr", "get_dmrs_main") and callable(dmr.get_dmrs_main)
    d = {n: v for n, _, v, _ in dmr.GET_DMRS_FLAGS}
    assert d["fdr_thresholds"] == [.01, .05] and d["site_prob"] == 0.5 and d["max_gap_bp"] == 300
    assert d["min_sites"] == 3 and dmr.parse_min_fraction(d["min_fraction"]) == Fraction(4, 5)
    for name in ("hyg_dmr_find_regions", "hyg_dmr_region_counts", "hyg_dmr_region_sums"):
        assert name in _lib.EXPORTS


# ------------------------------------------------------- argument checks
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


DUMMY = 0x1000  # never dereferenced: the checks come before any device work


def _err(lib):
    return lib.hyg_last_error().decode()


def _find(lib, counts=DUMMY, stride=3, column=1, n_sites=10, min_count=1, positions=DUMMY, max_gap=300,
          min_sites=1, regions=DUMMY, capacity=10, n_out=True):
    n = C.c_int64(-7)
    rc = lib.hyg_dmr_find_regions(counts, stride, column, n_sites, min_count, positions, max_gap, min_sites, regions,
                                  capacity, C.byref(n) if n_out else None, None)
    return rc, n.value


@pytest.mark.parametrize("kw,word", [
    (dict(min_sites=0), "min_sites"), (dict(min_count=-1), "min_count"), (dict(max_gap=-1), "max_gap"),
    (dict(column=3), "column"), (dict(column=-1), "column"), (dict(stride=0, column=0), "column"),
    (dict(counts=None), "null"), (dict(positions=None), "null"), (dict(n_out=False), "n_regions"),
    (dict(regions=None, capacity=4), "regions"), (dict(capacity=-1), "capacity"), (dict(n_sites=-1), "n_sites"),
    (dict(n_sites=(1 << 31) + 1), "n_sites"),
])
def test_find_regions_argument_errors(lib, kw, word):
    rc, n = _find(lib, **kw)
    assert rc == _lib.HYG_EINVAL
    assert _err(lib).startswith("hyg_dmr_find_regions:") and word in _err(lib)
    if kw.get("n_out", True):
        assert n == 0


def _groups(pairs):
    return (_lib.DmpGroup * max(len(pairs), 1))(*[_lib.DmpGroup(a, b) for a, b in pairs])


def _counts(lib, control=DUMMY, kase=DUMMY, B=5, groups=((0, 10), (10, 20)), block_rows=(0, 40, 10, 50), n_seeds=2,
            n_sites=30, regions=DUMMY, n_regions=3, num=4, den=5, out=DUMMY, n_groups=None):
    g = _groups(groups) if groups is not None else None
    br = (C.c_int64 * max(len(block_rows), 1))(*block_rows) if block_rows is not None else None
    return lib.hyg_dmr_region_counts(control, kase, B, g, br, len(groups) if n_groups is None else n_groups, n_seeds,
                                     n_sites, regions, n_regions, num, den, out, None)


@pytest.mark.parametrize("kw,word", [
    (dict(groups=((10, 20), (0, 10)), block_rows=(0, 40, 10, 50)), "sorted"),
    (dict(groups=((0, 11), (10, 20))), "disjoint"),
    (dict(groups=((0, 10), (10, 21))), "outside"),
    (dict(groups=((-1, 10), (10, 20))), "outside"),
    (dict(groups=((0, -1), (10, 20))), "outside"),
    (dict(block_rows=(0, 40, -1, 50)), "block row"),
    (dict(num=6, den=5), "fraction"), (dict(num=-1), "fraction"), (dict(den=0, num=0), "fraction"),
    (dict(den=1001), "fraction"),
    (dict(control=None), "null"), (dict(kase=None), "null"), (dict(regions=None), "null"), (dict(out=None), "null"),
    (dict(groups=None, n_groups=2), "null"), (dict(block_rows=None), "null"),
    (dict(B=0), "B"), (dict(n_seeds=0), "n_seeds"), (dict(B=4096, n_seeds=5, block_rows=(0,) * 10), "trajectories"),
    (dict(n_regions=-1), "n_regions"), (dict(n_sites=-1), "n_sites"),
])
def test_region_counts_argument_errors(lib, kw, word):
    assert _counts(lib, **kw) == _lib.HYG_EINVAL
    assert _err(lib).startswith("hyg_dmr_region_counts:") and word in _err(lib)


@pytest.mark.parametrize("kw,word", [
    (dict(counts=None), "null"), (dict(stride=0), "stride"), (dict(stride=4097), "stride"),
    (dict(regions=None), "null"), (dict(sums=None), "null"), (dict(n_regions=-1), "n_regions"),
    (dict(n_sites=-1), "n_sites"),
])
def test_region_sums_argument_errors(lib, kw, word):
    a = dict(counts=DUMMY, stride=14, n_sites=10, regions=DUMMY, n_regions=2, sums=DUMMY)
    a.update(kw)
    rc = lib.hyg_dmr_region_sums(a["counts"], a["stride"], a["n_sites"], a["regions"], a["n_regions"], a["sums"], None)
    assert rc == _lib.HYG_EINVAL
    assert _err(lib).startswith("hyg_dmr_region_sums:") and word in _err(lib)


def test_valid_arguments_without_a_device(lib):
    if lib.hyg_device_count() > 0:
        return  # with a device the dummy pointers would be read: tests/test_gpu_dmr.py covers the entries
    assert _find(lib) == (_lib.HYG_EDEVICE, 0)
    assert _find(lib, regions=None, capacity=0) == (_lib.HYG_EDEVICE, 0)
    assert _counts(lib) == _lib.HYG_EDEVICE
    assert _counts(lib, n_regions=0, regions=None, out=None) == _lib.HYG_EDEVICE
    assert _counts(lib, groups=(), block_rows=(), n_groups=0) == _lib.HYG_EDEVICE
    assert lib.hyg_dmr_region_sums(DUMMY, 14, 10, DUMMY, 2, DUMMY, None) == _lib.HYG_EDEVICE
    assert "no HIP device" in _err(lib)
