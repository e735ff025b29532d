"""GPU parity of the change-point pass (hyg_cp_* through the C ABI, the
functions of hygeia_amd/changepoints.py and `hygeia get_change_points`)
against the numpy restatement tests/cp_model.py.

Bar: exact. Everything here is integer arithmetic; the floats of the command's
TSV files are single float64 operations on those integers, compared as text."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import dmp_oracle as od  # noqa: E402
from tests import cp_model as cm  # noqa: E402

K = 6
STICKY_CASES = cm.STICKY_CASES
SHAPES = {(3000, 7): (7, 1), (3000, 50): (25, 2), (3000, 250): (25, 10), (1200, 2400): (300, 8)}  # (T, P): (B, seeds)
LEVELS = [(1, 2), (9, 10), (999, 1000), (1, 1)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    from hygeia_amd import _lib

    if _lib.load().hyg_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to("cuda:0")


def _quick_paths(T, P, seed, p_event=0.08):
    """(merged [T][P], control, case [T][P][2]) int16, vectorised: events with
    probability p_event per cell, durations counting up from them (a fifth of
    the trajectories start near each int16 wrap), regimes that change at most
    events and stay at some (a reset alone is an event too)."""
    rng = np.random.default_rng(seed)
    t = np.arange(T, dtype=np.int64)[:, None]

    def group():
        ev = rng.random((T, P)) < p_event
        ev[0] = False
        last = np.maximum.accumulate(np.where(ev, t, 0), axis=0)
        d0 = np.where(np.arange(P) % 5 == 1, 32768 - rng.integers(1, 40, P),
                      np.where(np.arange(P) % 5 == 3, 65536 - rng.integers(1, 40, P), rng.integers(0, 99, P)))
        d = t - last + np.where(last == 0, d0[None, :], 0)
        r = (rng.integers(0, K, P)[None, :] + np.cumsum(ev * rng.integers(0, K, (T, P)), axis=0)) % K
        return np.stack([d & 0xffff, r], -1).astype(np.uint16).view(np.int16)

    merged = (np.cumsum(rng.random((T, P)) < 0.05, axis=0) % 2).astype(np.int16) * 3  # 0 / 3: any non-zero is merged
    return merged, group(), group()


def _scatter(merged, control, case, B, S, seg, seed):
    """The trajectories of the segments `seg` = [(site_begin, rows)] as seed
    blocks placed in a shuffled order in one buffer with unused rows (random
    content), as hyg_tg_outputs holds them: (merged [rows][B], control, case
    [rows][B][2], block_rows)."""
    rng = np.random.default_rng(seed)
    rows = sum(r for _, r in seg) * S + 17
    fill = lambda: np.stack([rng.integers(1, 9, (rows, B)), rng.integers(0, K, (rows, B))], -1).astype(np.int16)  # noqa: E731
    m_b, c_b, k_b = rng.integers(0, 2, (rows, B)).astype(np.int16), fill(), fill()
    starts, o = {}, 5
    for q in rng.permutation(len(seg) * S):
        g, s = divmod(int(q), S)
        starts[(g, s)] = o
        s0, nr = seg[g]
        m_b[o:o + nr] = merged[s0:s0 + nr, s * B:(s + 1) * B]
        c_b[o:o + nr] = control[s0:s0 + nr, s * B:(s + 1) * B]
        k_b[o:o + nr] = case[s0:s0 + nr, s * B:(s + 1) * B]
        o += nr
    assert o <= rows
    return m_b, c_b, k_b, [[starts[(g, s)] for s in range(S)] for g in range(len(seg))]


@functools.lru_cache(maxsize=None)
def _case(T, P):
    """One sticky case, computed once: host arrays in four unequal groups, the
    restatement's events and windows (site_prob 0.05) and the device buffers."""
    B, S = SHAPES[(T, P)]
    merged, control, case, pos = cm.sticky_paths(T, P, K, STICKY_CASES[(T, P)])
    cuts = [0, T // 5 + 3, T // 2 + 1, T - T // 7, T]
    seg = [(cuts[i], cuts[i + 1] - cuts[i]) for i in range(4)]
    assert len({n for _, n in seg}) == 4  # unequal lengths
    E = cm.event_matrix(merged, control, case, seg)
    ev = cm.site_events(E)
    mc = cm.min_count(0.05, P)
    windows = [cm.find_regions(ev[:, kind], pos, mc, 300, 1) for kind in range(5)]
    m_b, c_b, k_b, block_rows = _scatter(merged, control, case, B, S, seg, 100 + P)
    return dict(B=B, S=S, T=T, P=P, E=E, ev=ev, pos=pos, seg=seg, cuts=cuts, windows=windows, mc=mc,
                block_rows=block_rows, merged=_dev(m_b, torch.int16), control=_dev(c_b, torch.int16),
                case=_dev(k_b, torch.int16), d_ev=_dev(ev, torch.int32), d_pos=_dev(pos, torch.int64))


# ------------------------------------------------------------- site_events
SIZES = [(n, P) for n in (1, 2, 255, 256, 257) for P in (1, 7, 50, 250, 256, 300)] + [(65_537, 7), (65_537, 50)]


@pytest.mark.parametrize("n_sites,P", SIZES)
def test_site_events_sizes(n_sites, P):
    """One group, one seed block (B = P): the edges of a 64-site tile and of
    the 256-thread step over a tile's words, B above and below 256."""
    from hygeia_amd import changepoints as cp

    merged, control, case = _quick_paths(n_sites, P, 1000 * P + n_sites)
    exp = cm.site_events(cm.event_matrix(merged, control, case, [(0, n_sites)]))
    if n_sites >= 255:
        assert exp.any(axis=0).all() and not exp[0].any()
    got = cp.site_events(_dev(merged, torch.int16), _dev(control, torch.int16), _dev(case, torch.int16), P,
                         [(0, n_sites)], [[0]], n_sites)
    assert got.dtype == torch.int32 and tuple(got.shape) == (n_sites, 5)
    np.testing.assert_array_equal(got.cpu().numpy(), exp)


@pytest.mark.parametrize("with_merged", [True, False])
def test_site_events_groups_seed_blocks_and_sentinel(with_merged):
    """Three groups with uncovered sites between them (one boundary inside a
    64-site tile), two seed blocks of B = 25 whose block rows are shuffled; rows
    outside the groups keep a sentinel, a group's first row is written as
    zeros; merged == NULL writes columns 3 and 4 as 0."""
    from hygeia_amd import changepoints as cp

    T, B, S = 3000, 25, 2
    merged, control, case, _ = cm.sticky_paths(T, B * S, K, STICKY_CASES[(T, B * S)])
    seg = [(3, 997), (1010, 1), (1030, 900), (1930, 1000)]  # holes: [0, 3), [1000, 1010), [1011, 1030), [2930, 3000)
    m_b, c_b, k_b, block_rows = _scatter(merged, control, case, B, S, seg, 77)
    exp = cm.site_events(cm.event_matrix(merged if with_merged else None, control, case, seg))
    covered = np.zeros(T, dtype=bool)
    for g0, n in seg:
        covered[g0:g0 + n] = True
        assert not exp[g0].any()
    assert exp[:, :3].any() and (exp[:, 3:].any() == with_merged)
    exp[~covered] = -7
    events = torch.full((T, 5), -7, dtype=torch.int32, device="cuda:0")
    got = cp.site_events(_dev(m_b, torch.int16) if with_merged else None, _dev(c_b, torch.int16),
                         _dev(k_b, torch.int16), B, seg, block_rows, T, events=events)
    assert got is events
    np.testing.assert_array_equal(got.cpu().numpy(), exp)
    # no group: nothing is written
    events.fill_(-7)
    cp.site_events(None, _dev(c_b, torch.int16), _dev(k_b, torch.int16), B, [], [], T, events=events)
    assert bool((events == -7).all())


@pytest.mark.parametrize("T,P", list(SHAPES))
def test_site_events_and_windows_of_the_sticky_cases(T, P):
    """The event matrix of the four (T, P) cases in four groups, and
    find_windows on it for every kind."""
    from hygeia_amd import changepoints as cp

    c = _case(T, P)
    ev = cp.site_events(c["merged"], c["control"], c["case"], c["B"], c["seg"], c["block_rows"], T)
    np.testing.assert_array_equal(ev.cpu().numpy(), c["ev"])
    for kind in range(5):
        w = cp.find_windows(ev, kind, c["mc"], c["d_pos"], 300)
        assert len(c["windows"][kind]) >= 10
        np.testing.assert_array_equal(w.cpu().numpy(), c["windows"][kind])
        for cut in c["cuts"][:-1]:  # no window holds a group's first row
            assert not ((c["windows"][kind][:, 0] <= cut) & (cut < c["windows"][kind][:, 1])).any()


# ----------------------------------------------------------- window_counts
@pytest.mark.parametrize("kind", range(5))
@pytest.mark.parametrize("T,P", list(SHAPES))
def test_window_counts_vs_restatement(T, P, kind):
    from hygeia_amd import changepoints as cp

    c = _case(T, P)
    w = c["windows"][kind]
    exp = cm.window_counts(c["E"][kind], w)
    assert ((exp[:, 0] > 0) & (exp[:, 0] < P)).sum() * 2 >= len(w)  # a 0 or P everywhere cannot pass
    if kind < 3:
        assert (exp[:, 0] != exp[:, 1]).any()
    # kinds 0 to 2 need no merged, kinds 3 and 4 nothing else
    got = cp.window_counts(c["merged"] if kind >= 3 else None, c["control"] if kind < 3 else None,
                           c["case"] if kind < 3 else None, c["B"], c["seg"], c["block_rows"], T, kind,
                           _dev(w, torch.int64))
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(w), 2)
    np.testing.assert_array_equal(got.cpu().numpy(), exp)


@pytest.mark.parametrize("T,P", [(3000, 50), (3000, 250), (1200, 2400)])
def test_window_counts_given_windows(T, P):
    """Windows given by hand: of 1, G and G + 1 sites (G = 256 / P lane rows),
    spanning a group boundary, starting on a group's first row, overlapping,
    and covering sites outside every group."""
    from hygeia_amd import changepoints as cp

    B, S = SHAPES[(T, P)]
    merged, control, case, _ = cm.sticky_paths(T, P, K, STICKY_CASES[(T, P)])
    seg = [(0, 500), (500, 300), (830, 0), (830, 200), (1040, 150)]  # holes: [800, 830), [1030, 1040), [1190, T)
    m_b, c_b, k_b, block_rows = _scatter(merged, control, case, B, S, seg, 8)
    E = cm.event_matrix(merged, control, case, seg)
    G = max(256 // P, 1)
    win = np.array([[10, 11], [13, 14], [100, 100 + G], [200, 201 + G], [480, 520], [500, 501], [500, 540],
                    [499, 501], [790, 840], [805, 820], [1020, 1045], [0, T], [0, 1], [1189, 1191], [100, 100 + G],
                    [1039, 1041], [829, 831]], dtype=np.int64)
    d = [_dev(a, torch.int16) for a in (m_b, c_b, k_b)]
    for kind in range(5):
        exp = cm.window_counts(E[kind], win)
        got = cp.window_counts(d[0], d[1], d[2], B, seg, block_rows, T, kind, _dev(win, torch.int64)).cpu().numpy()
        np.testing.assert_array_equal(got, exp)
        assert exp[5].tolist() == [0, 0] and exp[9].tolist() == [0, 0] and exp[11, 0] == P
    # the same paths as one group: the boundary rows then carry events
    one = cm.window_counts(cm.event_matrix(merged, control, case, [(0, T)])[2], win)
    assert (one != cm.window_counts(E[2], win)).any()
    # no group at all; no window at all
    got = cp.window_counts(d[0], d[1], d[2], B, [], [], T, 2, _dev(win[:4], torch.int64)).cpu().numpy()
    assert got.tolist() == [[0, 0]] * 4
    got = cp.window_counts(d[0], d[1], d[2], B, seg, block_rows, T, 2,
                           torch.zeros((0, 2), dtype=torch.int64, device="cuda:0"))
    assert tuple(got.shape) == (0, 2)


@functools.lru_cache(maxsize=None)
def _long():
    T, B, S = 70_050, 25, 2
    merged, control, case = _quick_paths(T, B * S, 5, p_event=2e-5)
    seg = [(0, 30_000), (30_000, 40_050)]
    return T, B, S, merged, control, case, seg


def test_window_counts_one_long_window():
    """70 000 sites in one window at P = 50, over two groups; events so rare
    that n_any and n_one are neither 0 nor P."""
    from hygeia_amd import changepoints as cp

    T, B, S, merged, control, case, seg = _long()
    m_b, c_b, k_b, block_rows = _scatter(merged, control, case, B, S, seg, 3)
    E = cm.event_matrix(merged, control, case, seg)
    win = np.array([[20, 70_020]], dtype=np.int64)
    d = [_dev(a, torch.int16) for a in (m_b, c_b, k_b)]
    for kind in (0, 1, 2, 4):
        s = E[kind][20:70_020].sum(axis=0)
        exp = [[int((s >= 1).sum()), int((s == 1).sum())]]
        if kind < 3:
            assert 0 < exp[0][1] < exp[0][0] < B * S
        got = cp.window_counts(d[0], d[1], d[2], B, seg, block_rows, T, kind, _dev(win, torch.int64)).cpu().numpy()
        assert got.tolist() == exp


# -------------------------------------------------------- window_intervals
@pytest.mark.parametrize("T,P", list(SHAPES))
def test_window_intervals_vs_restatement(T, P):
    from hygeia_amd import changepoints as cp

    c = _case(T, P)
    for kind in range(5):
        w = c["windows"][kind]
        for num, den in LEVELS:
            got = cp.window_intervals(c["d_ev"], kind, _dev(w, torch.int64), (num, den))
            assert got.dtype == torch.int64 and tuple(got.shape) == (len(w), 4)
            exp = cm.window_intervals(c["ev"][:, kind], w, num, den)
            np.testing.assert_array_equal(got.cpu().numpy(), exp)
    exp = cm.window_intervals(c["ev"][:, 0], c["windows"][0], 9, 10)
    assert (exp[:, 2] < exp[:, 3]).sum() * 10 >= len(exp)
    assert ((exp[:, 1] != exp[:, 2]) & (exp[:, 1] != exp[:, 3])).any()


def test_window_intervals_lengths_and_64_bit_sums():
    """Windows of 1, 255, 256, 257 and 70 000 sites (chunks of 256 with a
    carried sum), empty stretches, and a column with values near 2^31 / n, so
    the running sum and its products need 64 bits."""
    from hygeia_amd import changepoints as cp

    rng = np.random.default_rng(11)
    T = 70_400
    col = np.where(rng.random(T) < 0.3, rng.integers(1, 16_384, T), 0)
    col[5000:5600] = 0
    big = np.where(rng.random(T) < 0.5, rng.integers(2 ** 31 // 2 - 999, 2 ** 31 // 2, T), 0)
    mat = np.stack([col, big, np.full(T, 2 ** 31 - 1)], 1).astype(np.int32)
    win = np.array([[7, 8], [100, 355], [100, 356], [100, 357], [256, 512], [300, 70_300], [5000, 5600],
                    [5100, 5101], [4990, 5700], [0, T], [T - 1, T], [511, 769]], dtype=np.int64)
    d_mat, d_win = _dev(mat, torch.int32), _dev(win, torch.int64)
    for column in range(3):
        for num, den in LEVELS:
            got = cp.window_intervals(d_mat, column, d_win, (num, den)).cpu().numpy()
            exp = cm.window_intervals(mat[:, column], win, num, den)
            np.testing.assert_array_equal(got, exp)
    assert cm.window_intervals(mat[:, 2], win, 1, 2)[9, 0] > 2 ** 46
    assert cm.window_intervals(mat[:, 0], win, 1, 2)[6].tolist() == [0, 5000, 5000, 5599]
    got = cp.window_intervals(d_mat, 0, torch.zeros((0, 2), dtype=torch.int64, device="cuda:0"), (1, 2))
    assert tuple(got.shape) == (0, 4)


def test_two_calls_give_identical_bytes():
    from hygeia_amd import changepoints as cp

    c = _case(3000, 250)
    T = 3000
    for _ in range(2):
        a = cp.site_events(c["merged"], c["control"], c["case"], c["B"], c["seg"], c["block_rows"], T)
        b = cp.site_events(c["merged"], c["control"], c["case"], c["B"], c["seg"], c["block_rows"], T)
        assert torch.equal(a, b)
    w = cp.find_windows(a, 2, c["mc"], c["d_pos"], 300).contiguous()
    x = [cp.window_counts(c["merged"], c["control"], c["case"], c["B"], c["seg"], c["block_rows"], T, 2, w)
         for _ in range(2)]
    y = [cp.window_intervals(a, 2, w, (9, 10)) for _ in range(2)]
    assert torch.equal(x[0], x[1]) and torch.equal(y[0], y[1]) and len(w) > 50


# ------------------------------------------------- a real two-group launch
def test_site_events_on_a_real_launch():
    """K = 3, M = 20, B = 5, T = 400, two seeds: the (d, r) and merged rows
    that the backward kernel writes, through site_events, against the
    restatement on the same arrays copied to the host."""
    from hygeia_amd import changepoints as cp
    from hygeia_amd import synthetic as syn
    from hygeia_amd import two_group

    Kr, M, B, T, S = 3, 20, 5, 400, 2
    mu, sg = syn.regime_params(Kr)
    d = syn.simulate(T, 2, 2, K=Kr, seed=41, coverage=30.0, split_frac=0.2)
    maxr = int(max(d["tot_control"].max(), d["tot_case"].max()))
    model = two_group.CaseControlModel(mu, sg, two_group.uniform_theta(Kr), num_resampled_ancestors=M,
                                       num_samples_backward=B, max_total_reads=maxr, max_duration=T + 5)
    chains = [(0, T, seed, 700 + seed, seed * T) for seed in range(S)]
    out = two_group.run_chains_host({"control": d["meth_control"], "case": d["meth_case"]},
                                    {"control": d["tot_control"], "case": d["tot_case"]}, model, chains, S * T)
    assert (out["status"] == 0).all()
    merged, control, case = out["merged"], out["control"], out["case"]
    assert merged.shape == (S * T, B) and control.shape == (S * T, B, 2)
    by_site = lambda a: np.concatenate([a[s * T:(s + 1) * T] for s in range(S)], axis=1)  # noqa: E731
    E = cm.event_matrix(by_site(merged), by_site(control), by_site(case), [(0, T)])
    exp = cm.site_events(E)
    assert exp[:, 0].sum() > 0 and exp[:, 1].sum() > 0 and exp[:, 3].sum() + exp[:, 4].sum() > 0
    assert exp[:, 2].sum() < (T - 1) * B * S // 2  # most states continue
    got = cp.site_events(_dev(merged, torch.int16), _dev(control, torch.int16), _dev(case, torch.int16), B, [(0, T)],
                         [[0, T]], T)
    np.testing.assert_array_equal(got.cpu().numpy(), exp)


# ------------------------------------------------------- get_change_points
def _write_chrom(agg, chrom, merged, control, case, pos):
    import pandas as pd

    idx = pd.Series(pos.astype(np.int32), name="pos")
    for name, a, dt in (("control_regimes", control[..., 1], np.int8), ("case_regimes", case[..., 1], np.int8),
                        ("control_durations", control[..., 0], np.int16),
                        ("case_durations", case[..., 0], np.int16), ("merge_states", merged, np.int8)):
        pd.DataFrame(a.astype(dt)).set_index(idx).to_csv(agg / f"{name}_chrom_{chrom}.csv.gz", sep="\t",
                                                         compression="gzip")


def _hist(r, a, b):
    """Regime histogram of r [T][P] over the sites [a, b)."""
    return np.bincount(r[a:b].reshape(-1).astype(np.int64), minlength=K)


def _expected(chroms, data, P, segment, site_prob, max_gap, num, den):
    """The command's candidate rows per kind from the restatement, every field
    as text, and what the segmentation needs: per chromosome (groups, windows)."""
    rows = {name: [] for name in ("control", "case", "split", "merge")}
    wins = {name: [] for name in ("control", "case")}
    for chrom in chroms:
        merged, control, case, pos = data[chrom]
        T = len(pos)
        groups = [(g0, min(segment, T - g0)) for g0 in range(0, T, segment)]
        E = cm.event_matrix(merged, control, case, groups)
        ev = cm.site_events(E)
        for name, kind in (("control", 0), ("case", 1), ("split", 3), ("merge", 4)):
            w = cm.find_regions(ev[:, kind], pos, cm.min_count(site_prob, P), max_gap, 1)
            wc = cm.window_counts(E[kind], w)
            wi = cm.window_intervals(ev[:, kind], w, num, den)
            r = (control if name in ("control", "split") else case)[..., 1]
            for i, (a, b) in enumerate(w):
                n_any = int(wc[i, 0])
                rows[name].append([chrom, str(int(pos[a])), str(int(pos[b - 1])), str(int(b - a)), str(n_any),
                                   str(int(wc[i, 1])), str(int(wi[i, 0])), repr(n_any / P), repr(1. - n_any / P),
                                   str(int(pos[wi[i, 1]])), str(int(pos[wi[i, 2]])), str(int(pos[wi[i, 3]])),
                                   str(cm.modal_regime(r[a - 1], K)), str(cm.modal_regime(r[b - 1], K))])
            if name in wins:
                wins[name].append((chrom, groups, w, r, pos))
    return rows, wins


def _expected_segments(wins, keep, P):
    rows, o = [], 0
    for chrom, groups, w, r, pos in wins:
        sel = [tuple(x) for x, k in zip(w.tolist(), keep[o:o + len(w)]) if k]
        o += len(w)
        for u, v in cm.segments(groups, sel):
            h = _hist(r, u, v)
            m = int(np.argmax(h))
            rows.append([chrom, str(int(pos[u])), str(int(pos[v - 1])), str(int(v - u)), str(m + 1),
                         repr(int(h[m]) / (int(v - u) * P))])
    return rows


def _read_tsv(path):
    with open(path) as fh:
        lines = fh.read().split("\n")
    assert lines[-1] == ""
    return [ln.split("\t") for ln in lines[:-1]]


HEADER = ["chrom", "start", "end", "n_sites", "n_any", "n_one", "n_events", "prob_any", "null_stat", "mode_pos",
          "lo_pos", "hi_pos", "regime_before", "regime_after"]
SEG_HEADER = ["chrom", "start", "end", "n_sites", "regime", "regime_share"]


@pytest.fixture(scope="module")
def agg_dir(tmp_path_factory):
    agg = tmp_path_factory.mktemp("agg")
    data = {"5": cm.sticky_paths(1500, 50, K, 31), "X": cm.sticky_paths(1100, 50, K, 32),
            "s": cm.sticky_paths(300, 40, K, 33)}
    for chrom, (merged, control, case, pos) in data.items():
        _write_chrom(agg, chrom, merged, control, case, pos)
    return agg, data


def test_get_change_points_cli_end_to_end(agg_dir, tmp_path):
    """Two chromosomes, --segment_size 400 (four and three groups), a loose
    and a strict threshold; where the strict one selects nothing the files
    hold the header only, and the segmentation is then the groups themselves."""
    from hygeia_amd import cli

    agg, data = agg_dir
    out = tmp_path / "cp"
    thrs = [1e-09, 0.2]
    assert cli.main(["get_change_points", "--results_dir", str(agg), "--output_dir", str(out), "--chroms", "5,X",
                     "--segment_size", "400", "--fdr_thresholds", "1e-09", "--fdr_thresholds", "0.2"]) == 0
    P = 50
    rows, wins = _expected(["5", "X"], data, P, 400, 0.05, 300, 9, 10)  # the flag defaults
    names = []
    for name in ("control", "case", "split", "merge"):
        exp = rows[name]
        assert len({r[0] for r in exp}) == 2 and len(exp) >= 20
        got = _read_tsv(out / f"cp_{name}_candidates.tsv")
        assert got[0] == HEADER
        assert got[1:] == exp
        names.append(f"cp_{name}_candidates.tsv")
        t = np.array([1. - int(r[4]) / P for r in exp])
        n_sel = []
        for thr in thrs:
            _, _, threshold = od.fdr_procedure(t, thr)
            keep = t < threshold
            n_sel.append(int(keep.sum()))
            got = _read_tsv(out / f"cp_{name}_{thr}.tsv")
            assert got[0] == HEADER
            assert got[1:] == [r for r, k in zip(exp, keep) if k]
            names.append(f"cp_{name}_{thr}.tsv")
            if name in wins:
                got = _read_tsv(out / f"segments_{name}_{thr}.tsv")
                assert got[0] == SEG_HEADER
                assert got[1:] == _expected_segments(wins[name], keep, P)
                assert sum(int(r[3]) for r in got[1:]) == 1500 + 1100 - sum(int(r[3]) for r, k in zip(exp, keep) if k)
                names.append(f"segments_{name}_{thr}.tsv")
        assert n_sel[0] <= n_sel[1] and 0 < n_sel[1] < len(exp)
        if name != "case":  # (some case windows have n_any = P, a statistic of 0 that every threshold selects)
            assert n_sel[0] == 0 and _read_tsv(out / f"cp_{name}_{thrs[0]}.tsv") == [HEADER]
        if name == "control":
            assert len(_read_tsv(out / f"segments_{name}_{thrs[0]}.tsv")) == 1 + 4 + 3  # the groups themselves
    assert sorted(os.listdir(out)) == sorted(names)


def test_get_change_points_other_flags(agg_dir, tmp_path):
    """One group, a non-default site_prob, gap and a ratio for --level."""
    from hygeia_amd import cli

    agg, data = agg_dir
    out = tmp_path / "cp"
    assert cli.main(["get_change_points", "--results_dir", str(agg), "--output_dir", str(out), "--chroms", "X",
                     "--segment_size", "0", "--site_prob", "0.12", "--max_gap_bp", "40", "--level", "1/2",
                     "--fdr_thresholds", "0.3"]) == 0
    rows, wins = _expected(["X"], data, 50, 1100, 0.12, 40, 1, 2)
    for name in ("control", "case", "split", "merge"):
        assert len(rows[name]) >= 10
        assert _read_tsv(out / f"cp_{name}_candidates.tsv")[1:] == rows[name]
    t = np.array([1. - int(r[4]) / 50 for r in rows["case"]])
    _, _, threshold = od.fdr_procedure(t, 0.3)
    assert _read_tsv(out / "segments_case_0.3.tsv")[1:] == _expected_segments(wins["case"], t < threshold, 50)


def test_get_change_points_unequal_particles(agg_dir, tmp_path, capsys):
    from hygeia_amd import cli

    agg, _ = agg_dir
    assert cli.main(["get_change_points", "--results_dir", str(agg), "--output_dir", str(tmp_path / "cp"),
                     "--chroms", "5,s"]) == 1
    assert "chromosome s" in capsys.readouterr().err
