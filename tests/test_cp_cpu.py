"""The change-point pass on a host without a GPU: the numpy restatement
(tests/cp_model.py) against a hand-worked example, the statistics of its
sticky generator, `hygeia get_change_points`' flag handling, and the argument
checks of hyg_cp_* (HYG_EINVAL with a message naming the entry, before any
device is touched; HYG_EDEVICE for valid arguments without a device)."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from hygeia_amd import _lib
from tests import cp_model as cm

STICKY_CASES = cm.STICKY_CASES


# ------------------------------------------------------------ the restatement
def _example():
    """Eight sites, four trajectories, two groups: sites [0, 5) and [5, 8)."""
    control = np.array([
        [(5, 0), (32766, 1), (-2, 2), (3, 0)],   # a group's first row: no event
        [(6, 0), (32767, 1), (-1, 2), (0, 1)],   # p3: reset and a new regime
        [(7, 0), (-32768, 1), (0, 2), (1, 1)],   # p1: 32767 -> -32768 and p2: -1 -> 0 continue
        [(0, 3), (0, 3), (1, 2), (2, 1)],        # p0, p1
        [(1, 3), (1, 3), (0, 2), (3, 1)],        # p2: d reset, the same regime
        [(0, 0), (7, 2), (4, 4), (1, 1)],        # the second group's first row: no event whatever the states
        [(1, 0), (8, 2), (5, 4), (2, 1)],
        [(2, 0), (0, 5), (6, 4), (3, 1)],        # p1
    ], dtype=np.int16)
    merged = np.array([[1, 1, 1, 1], [1, 1, 0, 1], [0, 1, 0, 1], [0, 1, 1, 1], [1, 1, 1, 1],
                       [0, 0, 1, 1], [0, 1, 1, 0], [0, 1, 1, 0]], dtype=np.int16)
    case = np.array([
        [(5, 0), (32766, 1), (-2, 2), (3, 0)],
        [(6, 0), (32767, 1), (-1, 5), (0, 1)],   # p2 splits: a regime of its own; p3 follows the control's event
        [(0, 4), (-32768, 1), (0, 5), (1, 1)],   # p0 splits; p1 and p2 (-1 -> 0) continue over the wraps
        [(1, 4), (0, 3), (1, 2), (2, 1)],        # p1 follows; p2 merges: d continues 0 -> 1, the regime jumps 5 -> 2
        [(1, 3), (1, 3), (0, 2), (3, 1)],        # p0 merges: the control's (d + 1, r), d 1 -> 1; p2 follows the reset
        [(0, 0), (3, 3), (4, 4), (1, 1)],
        [(1, 0), (8, 2), (5, 4), (0, 2)],        # p1 merges, p3 splits
        [(2, 0), (0, 5), (6, 4), (1, 2)],        # p1 follows
    ], dtype=np.int16)
    pos = np.array([100, 110, 120, 130, 140, 150, 160, 170], dtype=np.int64)
    return merged, control, case, pos, [(0, 5), (5, 3)]


EXAMPLE_EVENTS = [[0, 0, 0, 0, 0], [1, 2, 2, 1, 0], [0, 1, 1, 1, 0], [2, 2, 3, 0, 1], [1, 2, 2, 0, 1],
                  [0, 0, 0, 0, 0], [0, 2, 2, 1, 1], [1, 1, 1, 0, 0]]


def test_hand_worked_example():
    merged, control, case, pos, groups = _example()
    E = cm.event_matrix(merged, control, case, groups)
    ev = cm.site_events(E)
    assert ev.tolist() == EXAMPLE_EVENTS
    # the wraps are continuations of both groups; the merge of p2 at site 3 is a case event with d continuing
    assert not E[0, 2].any() and not E[1, 2, 1] and not E[1, 2, 2]
    assert E[1, 3, 2] and case[3, 2, 0] == case[2, 2, 0] + 1 and case[3, 2, 1] != case[2, 2, 1]
    assert E[1, 4, 0] and not E[0, 4, 0]  # the merge of p0: an event of the case group alone
    # the group's first row: site 5 differs from site 4 everywhere, and has no event
    assert not E[:, 5].any() and not E[:, 0].any()
    # one group instead of two: site 5 then has events of every trajectory
    assert cm.site_events(cm.event_matrix(merged, control, case, [(0, 8)]))[5].tolist() == [4, 4, 4, 2, 0]
    # windows
    assert cm.find_regions(ev[:, 1], pos, 1, 300, 1).tolist() == [[1, 5], [6, 8]]
    assert cm.find_regions(ev[:, 0], pos, 1, 300, 1).tolist() == [[1, 2], [3, 5], [7, 8]]
    assert cm.window_counts(E[1], [(1, 5), (6, 8)]).tolist() == [[4, 2], [2, 1]]
    assert cm.window_counts(E[0], [(0, 8), (5, 7)]).tolist() == [[4, 3], [0, 0]]
    assert cm.window_counts(E[3], [(1, 3), (6, 7)]).tolist() == [[2, 2], [1, 1]]
    assert cm.window_counts(E[4], [(3, 5)]).tolist() == [[2, 2]]
    # intervals of the control column [0, 1, 0, 2, 1, 0, 0, 1]
    c = ev[:, 0]
    assert cm.window_intervals(c, [(1, 5)], 1, 2).tolist() == [[4, 3, 3, 3]]
    assert cm.window_intervals(c, [(1, 5)], 9, 10).tolist() == [[4, 3, 1, 4]]  # the mode strictly inside
    assert cm.window_intervals(c, [(1, 5)], 1, 1).tolist() == [[4, 3, 1, 4]]
    assert cm.window_intervals(c, [(0, 8)], 1, 2).tolist() == [[5, 3, 3, 4]]
    assert cm.window_intervals(c, [(0, 8)], 1, 1).tolist() == [[5, 3, 1, 7]]
    assert cm.window_intervals(c, [(5, 7)], 9, 10).tolist() == [[0, 5, 5, 6]]  # E_tot = 0
    assert cm.window_intervals(ev[:, 1], [(1, 5)], 1, 2).tolist() == [[7, 1, 1, 4]]  # ties: the first maximum
    # merged == None: no split or merge events
    assert cm.site_events(cm.event_matrix(None, control, case, groups))[:, 3:].sum() == 0
    # segmentation: the stretches between the windows, per group
    assert cm.segments(groups, [(1, 2), (3, 5), (7, 8)]).tolist() == [[0, 1], [2, 3], [5, 7]]
    assert cm.segments(groups, []).tolist() == [[0, 5], [5, 8]]
    assert cm.modal_regime([0, 3, 3, 1], 6) == 4 and cm.modal_regime([2, 1, 1, 2], 6) == 2


@pytest.mark.parametrize("num,den", [(1, 2), (9, 10), (1, 1)])
def test_interval_properties(num, den):
    """lo <= hi, both inside the window; at level 1/1 they are the first and
    last site with an event; E_tot = 0 gives the window's edges."""
    rng = np.random.default_rng(num * 31 + den)
    c = np.where(rng.random(400) < 0.4, rng.integers(1, 60, 400), 0)
    c[100:120] = 0
    a = rng.integers(0, 390, 200)
    w = np.stack([a, np.minimum(a + rng.integers(1, 40, 200), 400)], 1)
    w = np.concatenate([w, [[100, 120], [0, 400], [105, 106]]])
    out = cm.window_intervals(c, w, num, den)
    for (a, b), (tot, mode, lo, hi) in zip(w, out):
        assert a <= lo <= hi < b and a <= mode < b and tot == c[a:b].sum()
        if tot == 0:
            assert (mode, lo, hi) == (a, a, b - 1)
            continue
        nz = np.nonzero(c[a:b])[0] + a
        assert nz[0] <= lo and hi <= nz[-1] and c[mode] == c[a:b].max() and (c[a:mode] < c[mode]).all()
        if (num, den) == (1, 1):
            assert (lo, hi) == (nz[0], nz[-1])
    assert out[-3].tolist() == [0, 100, 100, 119]


@pytest.mark.parametrize("T,P", list(STICKY_CASES))
def test_sticky_paths_statistics(T, P):
    """The generator gives windows that are neither empty nor full, with
    trajectories that have several events, intervals wider than a site, modes
    strictly inside them and wrapped continuations inside windows: a kernel
    that returned 0, P or the window's edges everywhere could not pass the GPU
    comparison. Observed over the four cases (one group, site_prob 0.05, level
    9/10), kinds control and case: 21 to 366 windows, 0.94 to 1.0 of them with
    0 < n_any < P, 0.14 to 1.0 with n_one != n_any, 0.46 to 1.0 with lo < hi, 15
    to 91 modes strictly inside, 1 to 134 wrapped continuations; kinds split
    and merge: 21 to 134 windows."""
    K = 6
    merged, control, case, pos = cm.sticky_paths(T, P, K, STICKY_CASES[(T, P)])
    assert merged.shape == (T, P) and control.shape == case.shape == (T, P, 2) and pos.shape == (T,)
    assert merged.dtype == control.dtype == case.dtype == np.int16
    for st in (control, case):
        assert st[..., 1].min() >= 0 and st[..., 1].max() < K
    assert (control[merged != 0] == case[merged != 0]).all()  # merged: the case state is the control's
    # both wraps occur, in continuing stretches
    for st in (control, case):
        d0, d1 = st[:-1, :, 0], st[1:, :, 0]
        assert ((d0 == 32767) & (d1 == -32768)).any() and ((d0 == -1) & (d1 == 0)).any()
    E = cm.event_matrix(merged, control, case, [(0, T)])
    ev = cm.site_events(E)
    assert (ev[:, 2] >= np.maximum(ev[:, 0], ev[:, 1])).all() and (ev[:, 2] <= ev[:, 0] + ev[:, 1]).all()
    mc = cm.min_count(0.05, P)
    wrapped = 0
    for kind in (0, 1):
        w = cm.find_regions(ev[:, kind], pos, mc, 300, 1)
        wc = cm.window_counts(E[kind], w)
        wi = cm.window_intervals(ev[:, kind], w, 9, 10)
        n = len(w)
        mid = float(((wc[:, 0] > 0) & (wc[:, 0] < P)).mean())
        differ = float((wc[:, 0] != wc[:, 1]).mean())
        wide = float((wi[:, 2] < wi[:, 3]).mean())
        inside = int(((wi[:, 1] != wi[:, 2]) & (wi[:, 1] != wi[:, 3])).sum())
        wr = cm.wrapped_continuations(control if kind == 0 else case, E[kind], w)
        print(T, P, kind, n, mid, differ, wide, inside, wr)
        assert 21 <= n <= 366
        assert 0.94 <= mid <= 1.0      # the issue asks for at least a half
        assert 0.14 <= differ <= 1.0   # at least a tenth
        assert 0.46 <= wide <= 1.0     # at least a tenth
        assert 15 <= inside <= 91      # at least one
        wrapped += wr
    assert wrapped >= 1
    for kind in (3, 4):
        n = len(cm.find_regions(ev[:, kind], pos, mc, 300, 1))
        print(T, P, kind, n)
        assert 21 <= n <= 134          # at least ten


# ------------------------------------------------------------------ flags
def test_level_parsing():
    from hygeia_amd import changepoints as cp
    from hygeia_amd import cli

    assert cp.parse_level("0.9") == Fraction(9, 10)
    assert cp.parse_level("9/10") == Fraction(9, 10)
    assert cp.parse_level("1") == Fraction(1, 1)
    assert cp.parse_level("0.999") == Fraction(999, 1000)
    assert cp.parse_level("0.5") == Fraction(1, 2)
    for bad in ("0", "0.9001", "1/1001", "1.5", "-0.1", "x", "1/0", "6/5"):
        with pytest.raises(cli.FlagError):
            cp.parse_level(bad)


@pytest.mark.parametrize("flag,value", [("--level", "0.12345"), ("--level", "0"), ("--site_prob", "0"),
                                        ("--site_prob", "1.5")])
def test_flag_errors_exit_1(tmp_path, capsys, flag, value):
    from hygeia_amd import cli

    rc = cli.main(["get_change_points", "--results_dir", str(tmp_path), "--output_dir", str(tmp_path / "o"),
                   flag, value])
    assert rc == 1
    assert flag[2:] in capsys.readouterr().err
    assert not (tmp_path / "o").exists()


def test_groups_and_segments_of_the_command():
    from hygeia_amd import changepoints as cp

    assert cp.groups_of(250, 100) == [(0, 100), (100, 100), (200, 50)]
    assert cp.groups_of(200, 100) == [(0, 100), (100, 100)]
    assert cp.groups_of(250, 0) == [(0, 250)] and cp.groups_of(50, 100) == [(0, 50)]
    groups = [(0, 5), (5, 3)]
    for wins in ([(1, 2), (3, 5), (7, 8)], [], [(1, 5), (6, 7)], [(6, 8)]):
        w = np.array(wins, dtype=np.int64).reshape(-1, 2)
        assert cp.segments_between(groups, w).tolist() == cm.segments(groups, wins).tolist()
    assert cp.segments_between(groups, np.array([[1, 5], [6, 7]])).tolist() == [[0, 1], [5, 6], [7, 8]]


def test_get_change_points_is_a_command():
    from hygeia_amd import changepoints as cp
    from hygeia_amd import cli

    assert "get_change_points" in cli.COMMANDS.split() and "get_change_points" in cli._SUBCOMMANDS
    assert cli._SUBCOMMANDS["get_change_points"][:2] == ("changepoints", "get_change_points_main")
    assert callable(cp.get_change_points_main)
    d = {n: v for n, _, v, _ in cp.GET_CHANGE_POINTS_FLAGS}
    assert d["fdr_thresholds"] == [.01, .05] and d["site_prob"] == 0.05 and d["max_gap_bp"] == 300
    assert d["n_regimes"] == 6 and d["segment_size"] == 100000 and cp.parse_level(d["level"]) == Fraction(9, 10)
    assert cp.KINDS == cm.KINDS
    for name in ("hyg_cp_site_events", "hyg_cp_window_counts", "hyg_cp_window_intervals"):
        assert name in _lib.EXPORTS


# ------------------------------------------------------- argument checks
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


DUMMY = 0x1000  # never dereferenced: the checks come before any device work


def _err(lib):
    return lib.hyg_last_error().decode()


def _groups(pairs):
    return (_lib.DmpGroup * max(len(pairs), 1))(*[_lib.DmpGroup(a, b) for a, b in pairs])


def _traj(kw):
    a = dict(merged=DUMMY, control=DUMMY, kase=DUMMY, B=5, groups=((0, 10), (10, 20)), block_rows=(0, 40, 10, 50),
             n_seeds=2, n_sites=30, n_groups=None)
    a.update(kw)
    g = _groups(a["groups"]) if a["groups"] is not None else None
    br = (C.c_int64 * max(len(a["block_rows"]), 1))(*a["block_rows"]) if a["block_rows"] is not None else None
    n_groups = len(a["groups"]) if a["n_groups"] is None else a["n_groups"]
    return a, (a["merged"], a["control"], a["kase"], a["B"], g, br, n_groups, a["n_seeds"], a["n_sites"])


def _events(lib, **kw):
    a, head = _traj(kw)
    return lib.hyg_cp_site_events(*head, a.get("events", DUMMY), None)


def _counts(lib, **kw):
    a, head = _traj(kw)
    return lib.hyg_cp_window_counts(*head, a.get("kind", 2), a.get("windows", DUMMY), a.get("n_windows", 3),
                                    a.get("counts", DUMMY), None)


def _intervals(lib, **kw):
    a = dict(events=DUMMY, stride=5, column=1, n_sites=30, windows=DUMMY, n_windows=3, num=9, den=10, out=DUMMY)
    a.update(kw)
    return lib.hyg_cp_window_intervals(a["events"], a["stride"], a["column"], a["n_sites"], a["windows"],
                                       a["n_windows"], a["num"], a["den"], a["out"], None)


TRAJECTORY_ERRORS = [
    (dict(groups=((10, 20), (0, 10))), "sorted"),
    (dict(groups=((0, 11), (10, 20))), "disjoint"),
    (dict(groups=((0, 10), (10, 21))), "outside"),
    (dict(groups=((-1, 10), (10, 20))), "outside"),
    (dict(groups=((0, -1), (10, 20))), "outside"),
    (dict(block_rows=(0, 40, -1, 50)), "block row"),
    (dict(control=None), "null"), (dict(kase=None), "null"),
    (dict(groups=None, n_groups=2), "null"), (dict(block_rows=None), "null"), (dict(n_groups=-1), "groups"),
    (dict(B=0), "B"), (dict(n_seeds=0), "n_seeds"), (dict(B=4096, n_seeds=5, block_rows=(0,) * 10), "trajectories"),
    (dict(n_sites=-1), "n_sites"),
]


@pytest.mark.parametrize("kw,word", TRAJECTORY_ERRORS + [(dict(events=None), "events")])
def test_site_events_argument_errors(lib, kw, word):
    assert _events(lib, **kw) == _lib.HYG_EINVAL
    assert _err(lib).startswith("hyg_cp_site_events:") and word in _err(lib)


@pytest.mark.parametrize("kw,word", TRAJECTORY_ERRORS + [
    (dict(kind=-1), "kind"), (dict(kind=5), "kind"),
    (dict(kind=3, merged=None), "merged"), (dict(kind=4, merged=None), "merged"),
    (dict(windows=None), "null"), (dict(counts=None), "null"), (dict(n_windows=-1), "n_windows"),
])
def test_window_counts_argument_errors(lib, kw, word):
    assert _counts(lib, **kw) == _lib.HYG_EINVAL
    assert _err(lib).startswith("hyg_cp_window_counts:") and word in _err(lib)


@pytest.mark.parametrize("kw,word", [
    (dict(events=None), "null"), (dict(windows=None), "null"), (dict(out=None), "null"),
    (dict(num=0, den=1), "level"), (dict(num=6, den=5), "level"), (dict(num=1, den=1001), "level"),
    (dict(num=-1), "level"), (dict(den=0, num=0), "level"),
    (dict(stride=0, column=0), "stride"), (dict(column=5), "column"), (dict(column=-1), "column"),
    (dict(n_windows=-1), "n_windows"), (dict(n_sites=-1), "n_sites"),
])
def test_window_intervals_argument_errors(lib, kw, word):
    assert _intervals(lib, **kw) == _lib.HYG_EINVAL
    assert _err(lib).startswith("hyg_cp_window_intervals:") and word in _err(lib)


def test_valid_arguments_without_a_device(lib):
    if lib.hyg_device_count() > 0:
        return  # with a device the dummy pointers would be read: tests/test_gpu_cp.py covers the entries
    assert _events(lib) == _lib.HYG_EDEVICE
    assert _events(lib, merged=None) == _lib.HYG_EDEVICE
    assert _events(lib, groups=(), block_rows=(), n_groups=0) == _lib.HYG_EDEVICE
    for kind in range(5):
        assert _counts(lib, kind=kind) == _lib.HYG_EDEVICE
    assert _counts(lib, kind=2, merged=None) == _lib.HYG_EDEVICE
    assert _counts(lib, kind=3, control=None, kase=None) == _lib.HYG_EDEVICE
    assert _counts(lib, n_windows=0, windows=None, counts=None) == _lib.HYG_EDEVICE
    assert _intervals(lib) == _lib.HYG_EDEVICE
    assert _intervals(lib, num=1, den=1) == _lib.HYG_EDEVICE
    assert _intervals(lib, n_windows=0, windows=None, out=None) == _lib.HYG_EDEVICE
    assert "no HIP device" in _err(lib)
