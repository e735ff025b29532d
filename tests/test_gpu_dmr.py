"""GPU parity of the region (DMR) pass (hyg_dmr_* through the C ABI, the
functions of hygeia_amd/dmr.py and `hygeia get_dmrs`) against the numpy
restatement tests/dmr_model.py.

Bar: exact. Everything here is integer arithmetic; the floats of the command's
TSV files are single float64 operations on those integers, compared as text."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import dmp_oracle as od  # noqa: E402
from tests import dmr_model as dm  # noqa: E402

K = 6
STICKY_CASES = dm.STICKY_CASES
SHAPES = {(3000, 7): (7, 1), (3000, 50): (25, 2), (3000, 250): (25, 10), (1200, 2400): (300, 8)}  # (T, P): (B, seeds)
FRACTIONS = [(1, 1), (4, 5), (1, 2), (0, 1)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    from hygeia_amd import _lib

    if _lib.load().hyg_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to("cuda:0")


def _scatter(r_ctrl, r_case, B, S, seg, seed):
    """The trajectories of the segments `seg` = [(site_begin, rows)] as seed
    blocks placed in a shuffled order in one buffer with unused rows (random
    content), as hyg_tg_outputs holds them: (control, case [rows][B][2], block_rows)."""
    rng = np.random.default_rng(seed)
    rows = sum(r for _, r in seg) * S + 17
    fill = lambda: np.stack([rng.integers(1, 9, (rows, B)), rng.integers(0, K, (rows, B))], -1).astype(np.int16)  # noqa: E731
    control, case = fill(), fill()
    starts, o = {}, 5
    for q in rng.permutation(len(seg) * S):
        g, s = divmod(int(q), S)
        starts[(g, s)] = o
        s0, nr = seg[g]
        control[o:o + nr, :, 1] = r_ctrl[s0:s0 + nr, s * B:(s + 1) * B]
        case[o:o + nr, :, 1] = r_case[s0:s0 + nr, s * B:(s + 1) * B]
        o += nr
    assert o <= rows
    return control, case, [[starts[(g, s)] for s in range(S)] for g in range(len(seg))]


@functools.lru_cache(maxsize=None)
def _case(T, P):
    """One sticky case, computed once: host arrays, the restatement's regions
    (min_sites 1) and the device buffers in four unequal groups."""
    B, S = SHAPES[(T, P)]
    r_ctrl, r_case, pos = dm.sticky_trajectories(T, P, K, STICKY_CASES[(T, P)])
    D = r_ctrl != r_case
    counts = dm.site_counts(r_ctrl, r_case, K)
    regions = dm.find_regions(counts[:, 1], pos, dm.min_count(0.5, P), 300, 1)
    # group boundaries inside regions of several sites, so that regions straddle them
    inner = [int(a) + (int(b) - int(a)) // 2 for a, b in regions if b - a >= 4]
    cuts = [0, inner[len(inner) // 5], inner[len(inner) // 2], inner[-2], T]
    seg = [(cuts[i], cuts[i + 1] - cuts[i]) for i in range(4)]
    assert len({n for _, n in seg}) == 4  # unequal lengths
    control, case, block_rows = _scatter(r_ctrl, r_case, B, S, seg, 100 + P)
    return dict(B=B, S=S, T=T, P=P, D=D, pos=pos, counts=counts, regions=regions, seg=seg, cuts=cuts,
                block_rows=block_rows, control=_dev(control, torch.int16), case=_dev(case, torch.int16),
                d_counts=_dev(counts, torch.int32), d_pos=_dev(pos, torch.int64), d_regions=_dev(regions, torch.int64))


# ------------------------------------------------------------ find_regions
def _random_sites(n, seed, p_seed=0.8):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 100, (n, 3)).astype(np.int32)
    counts[:, 1] = np.where(rng.random(n) < p_seed, rng.integers(5, 50, n), rng.integers(0, 5, n))
    pos = 10_000 + np.cumsum(rng.choice(dm.GAPS, size=n, p=dm.GAP_PROBS))
    return counts, pos.astype(np.int64)


@pytest.mark.parametrize("min_sites", [1, 3])
@pytest.mark.parametrize("n_sites", [1, 2, 255, 256, 257, 65_537, 300_001])
def test_find_regions_vs_restatement(n_sites, min_sites):
    """Column 1 of a stride-3 matrix; the sizes cover the edges of a scan tile
    (256), a second scan level (257 tiles of block sums at 65 537 sites) and
    runs that cross tile boundaries."""
    from hygeia_amd import dmr

    counts, pos = _random_sites(n_sites, n_sites + min_sites)
    exp = dm.find_regions(counts[:, 1], pos, 5, 300, min_sites)
    if n_sites > 300:
        assert len(exp) > n_sites // 40 and (exp[:, 1] - exp[:, 0]).max() > 10
    got = dmr.find_regions(_dev(counts, torch.int32), 1, 5, _dev(pos, torch.int64), 300, min_sites)
    assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == exp.shape
    np.testing.assert_array_equal(got.cpu().numpy(), exp)


def test_find_regions_special_cases():
    from hygeia_amd import dmr

    n = 1000
    counts = np.zeros((n, 3), np.int32)
    counts[:, 1] = 9
    pos = (100 + 2 * np.arange(n)).astype(np.int64)
    find = lambda c, p, mc=5, gap=300, ms=1: dmr.find_regions(  # noqa: E731
        _dev(c, torch.int32), 1, mc, _dev(p, torch.int64), gap, ms).cpu().numpy()
    # every site a seed site at 2-bp gaps: one region, ending at the last site
    assert find(counts, pos).tolist() == [[0, n]]
    # no seed site
    assert find(counts, pos, mc=10).shape == (0, 2)
    assert find(counts, pos, ms=n + 1).shape == (0, 2)
    # no link at all: every site its own region
    np.testing.assert_array_equal(find(counts, pos, gap=1), dm.find_regions(counts[:, 1], pos, 5, 1, 1))
    # a region ending at the last site after a non-seed site
    c2 = counts.copy()
    c2[n - 5, 1] = 0
    assert find(c2, pos).tolist() == [[0, n - 5], [n - 4, n]]
    # a restart of the positions in the middle: a non-positive difference never links
    p2 = pos.copy()
    p2[600:] = 50 + 2 * np.arange(n - 600)
    assert find(counts, p2).tolist() == [[0, 600], [600, n]]
    p3 = pos.copy()
    p3[600:] -= 2  # difference 0 between sites 599 and 600
    assert p3[600] == p3[599]
    assert find(counts, p3).tolist() == [[0, 600], [600, n]]
    # min_count 0: every site is a seed site
    assert find(np.zeros((n, 3), np.int32), pos, mc=0, ms=3).tolist() == [[0, n]]


def test_find_regions_count_only_capacity_and_determinism():
    from hygeia_amd import _lib, dmr

    counts, pos = _random_sites(70_000, 5)
    exp = dm.find_regions(counts[:, 1], pos, 5, 300, 3)
    n_exp = len(exp)
    assert n_exp > 1000
    d_counts, d_pos = _dev(counts, torch.int32), _dev(pos, torch.int64)
    L = _lib.load()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(buf, cap):
        n = C.c_int64(-1)
        rc = L.hyg_dmr_find_regions(d_counts.data_ptr(), 3, 1, len(pos), 5, d_pos.data_ptr(), 300, 3,
                                    buf.data_ptr() if buf is not None else None, cap, C.byref(n), s)
        return rc, n.value

    assert call(None, 0) == (_lib.HYG_OK, n_exp)  # count only
    buf = torch.full((n_exp + 1, 2), -9, dtype=torch.int64, device="cuda:0")
    assert call(buf, n_exp - 1) == (_lib.HYG_EINVAL, n_exp)  # capacity one short
    assert "capacity" in L.hyg_last_error().decode()
    torch.cuda.synchronize()
    assert bool((buf[n_exp - 1:] == -9).all())  # the rows behind the buffer are untouched
    assert call(buf, n_exp) == (_lib.HYG_OK, n_exp)  # exactly enough
    torch.cuda.synchronize()
    np.testing.assert_array_equal(buf[:n_exp].cpu().numpy(), exp)
    assert bool((buf[n_exp:] == -9).all())
    a = dmr.find_regions(d_counts, 1, 5, d_pos, 300, 3)
    b = dmr.find_regions(d_counts, 1, 5, d_pos, 300, 3)
    assert torch.equal(a, b) and torch.equal(a, buf[:n_exp])  # identical from run to run


def test_find_regions_counts_first_above_its_bound(monkeypatch):
    """The Python function counts first when its bound n_sites // min_sites
    would be a large allocation."""
    from hygeia_amd import dmr

    monkeypatch.setattr(dmr, "_BOUND_BYTES", 1024)
    counts, pos = _random_sites(5000, 9)
    got = dmr.find_regions(_dev(counts, torch.int32), 1, 5, _dev(pos, torch.int64), 300, 1)
    np.testing.assert_array_equal(got.cpu().numpy(), dm.find_regions(counts[:, 1], pos, 5, 300, 1))


@pytest.mark.parametrize("T,P", list(SHAPES))
def test_find_regions_on_device_site_counts(T, P):
    """dmp.site_counts' matrix straight into find_regions (column 1)."""
    from hygeia_amd import dmp, dmr

    c = _case(T, P)
    merged = torch.ones((c["control"].shape[0], c["B"]), dtype=torch.int16, device="cuda:0")
    counts, _ = dmp.site_counts(merged, c["control"], c["case"], c["B"], K, c["seg"], c["block_rows"], T)
    got = counts.cpu().numpy()
    got[:, 0] = 0  # (#merged == 0 is not part of the model's matrix)
    np.testing.assert_array_equal(got, c["counts"])
    for min_sites in (1, 3):
        reg = dmr.find_regions(counts, 1, dm.min_count(0.5, P), c["d_pos"], 300, min_sites)
        np.testing.assert_array_equal(reg.cpu().numpy(),
                                      dm.find_regions(c["counts"][:, 1], c["pos"], dm.min_count(0.5, P), 300, min_sites))


# ----------------------------------------------------------- region_counts
@pytest.mark.parametrize("T,P", list(SHAPES))
def test_region_counts_vs_restatement(T, P):
    """Four groups of unequal length, their seed blocks shuffled in one buffer
    with unused rows; regions straddle the group boundaries."""
    from hygeia_amd import dmr

    c = _case(T, P)
    reg = c["regions"]
    straddle = [(a, b) for a, b in reg for cut in c["cuts"][1:-1] if a < cut < b]
    assert len(straddle) >= 1
    exp11 = dm.region_counts(c["D"], reg, 1, 1)
    mid = (exp11[:, 0] > 0) & (exp11[:, 0] < P)
    assert mid.sum() * 2 >= len(reg)  # an all-zero or all-P result cannot pass
    for num, den in FRACTIONS:
        got = dmr.region_counts(c["control"], c["case"], c["B"], c["seg"], c["block_rows"], T, c["d_regions"],
                                (num, den))
        assert got.dtype == torch.int32 and tuple(got.shape) == (len(reg), 2)
        exp = dm.region_counts(c["D"], reg, num, den)
        if (num, den) == (0, 1):
            assert (exp[:, 1] == P).all()
        np.testing.assert_array_equal(got.cpu().numpy(), exp)


def test_region_counts_one_long_region():
    from hygeia_amd import dmr

    T, B, S = 6000, 25, 2
    P = B * S
    rng = np.random.default_rng(21)
    D = rng.random((T, P)) < 0.1
    D[500:5500] = rng.random((5000, P)) < 0.5
    D[500:5500, np.arange(P) % 3 != 0] = True
    r_ctrl = rng.integers(0, K, (T, P))
    r_case = np.where(D, (r_ctrl + rng.integers(1, K, (T, P))) % K, r_ctrl)
    pos = (1000 + 2 * np.arange(T)).astype(np.int64)
    counts = dm.site_counts(r_ctrl, r_case, K)
    reg = dm.find_regions(counts[:, 1], pos, dm.min_count(0.5, P), 300, 3)
    assert reg.tolist() == [[500, 5500]] and reg[0, 1] - reg[0, 0] == 5000
    seg = [(0, 700), (700, 2301), (3001, 2999)]
    control, case, block_rows = _scatter(r_ctrl, r_case, B, S, seg, 3)
    d_reg = dmr.find_regions(_dev(counts, torch.int32), 1, dm.min_count(0.5, P), _dev(pos, torch.int64), 300, 3)
    np.testing.assert_array_equal(d_reg.cpu().numpy(), reg)
    for num, den in FRACTIONS:
        got = dmr.region_counts(_dev(control, torch.int16), _dev(case, torch.int16), B, seg, block_rows, T, d_reg,
                                (num, den)).cpu().numpy()
        exp = dm.region_counts(D, reg, num, den)
        np.testing.assert_array_equal(got, exp)
    assert dm.region_counts(D, reg, 1, 1).tolist() == [[33, 33]]
    assert dm.region_counts(D, reg, 1, 2)[0, 1] > 33


def test_region_counts_given_regions_and_uncovered_sites():
    """Regions of exactly 1, 63, 64 and 65 sites given by hand, overlapping
    regions, and regions with sites outside every group: those sites count as
    not differential for every trajectory."""
    from hygeia_amd import dmr

    T, P = 3000, 50
    B, S = SHAPES[(T, P)]
    c = _case(T, P)
    r_ctrl, r_case, _ = dm.sticky_trajectories(T, P, K, STICKY_CASES[(T, P)])
    seg = [(0, 1500), (1600, 400), (2000, 0), (2000, 995)]  # holes: [1500, 1600) and [2995, 3000); an empty group
    control, case, block_rows = _scatter(r_ctrl, r_case, B, S, seg, 8)
    D = c["D"].copy()
    D[1500:1600] = False
    D[2995:] = False
    reg = np.array([[10, 11], [100, 163], [200, 264], [300, 365], [1480, 1620], [1510, 1520], [2990, 3000], [0, 3000],
                    [100, 163], [1599, 1601], [1499, 1500], [2999, 3000]], dtype=np.int64)
    for num, den in FRACTIONS:
        got = dmr.region_counts(_dev(control, torch.int16), _dev(case, torch.int16), B, seg, block_rows, T,
                                _dev(reg, torch.int64), (num, den)).cpu().numpy()
        np.testing.assert_array_equal(got, dm.region_counts(D, reg, num, den))
    full = dm.region_counts(c["D"], reg, 4, 5)
    holed = dm.region_counts(D, reg, 4, 5)
    assert (full != holed).any() and holed[5].tolist() == [0, 0]
    # no group at all: nothing is differential anywhere
    got = dmr.region_counts(_dev(control, torch.int16), _dev(case, torch.int16), B, [], [], T,
                            _dev(reg[:4], torch.int64), (1, 2)).cpu().numpy()
    assert got.tolist() == [[0, 0]] * 4
    # no region: an empty result, nothing launched
    got = dmr.region_counts(_dev(control, torch.int16), _dev(case, torch.int16), B, seg, block_rows, T,
                            torch.zeros((0, 2), dtype=torch.int64, device="cuda:0"), (1, 2))
    assert tuple(got.shape) == (0, 2)


# ------------------------------------------------------------- region_sums
@pytest.mark.parametrize("T,P", list(SHAPES))
def test_region_sums_vs_numpy(T, P):
    from hygeia_amd import dmr

    c = _case(T, P)
    assert c["counts"].shape[1] == 2 + 2 * K
    got = dmr.region_sums(c["d_counts"], c["d_regions"])
    assert got.dtype == torch.int64
    exp = dm.region_sums(c["counts"], c["regions"])
    np.testing.assert_array_equal(got.cpu().numpy(), exp)
    np.testing.assert_array_equal(exp[:, 2:2 + K].sum(1), (c["regions"][:, 1] - c["regions"][:, 0]) * P)


@pytest.mark.parametrize("stride", [1, 3, 256, 257, 700])
def test_region_sums_strides_and_large_values(stride):
    """Both column mappings of the kernel (stride <= 256 and above), and sums
    beyond int32."""
    from hygeia_amd import dmr

    rng = np.random.default_rng(stride)
    T = 700
    counts = rng.integers(2 ** 30, 2 ** 31 - 1, (T, stride)).astype(np.int32)
    counts[::7] *= -1
    reg = np.array([[0, 1], [1, 64], [64, 129], [5, 700], [699, 700], [0, 700]], dtype=np.int64)
    got = dmr.region_sums(_dev(counts, torch.int32), _dev(reg, torch.int64)).cpu().numpy()
    exp = np.stack([counts[a:b].astype(np.int64).sum(0) for a, b in reg])
    assert np.abs(exp).max() > 2 ** 32
    np.testing.assert_array_equal(got, exp)
    np.testing.assert_array_equal(got, dm.region_sums(counts, reg))
    assert tuple(dmr.region_sums(_dev(counts, torch.int32),
                                 torch.zeros((0, 2), dtype=torch.int64, device="cuda:0")).shape) == (0, stride)


# ---------------------------------------------------------------- get_dmrs
MU = [0.95, 0.05, 0.80, 0.20, 0.50, 0.50]


def _write_chrom(agg, chrom, r_ctrl, r_case, pos):
    import pandas as pd

    for name, a in (("control_regimes", r_ctrl), ("case_regimes", r_case)):
        pd.DataFrame(a.astype(np.int8)).set_index(pd.Series(pos.astype(np.int32), name="pos")).to_csv(
            agg / f"{name}_chrom_{chrom}.csv.gz", sep="\t", compression="gzip")


def _expected_rows(chroms, data, P, site_prob, max_gap, min_sites, num, den):
    """get_dmrs' candidate table from the restatement, every field as text."""
    rows = []
    for chrom in chroms:
        r_ctrl, r_case, pos = data[chrom]
        counts = dm.site_counts(r_ctrl, r_case, K)
        reg = dm.find_regions(counts[:, 1], pos, dm.min_count(site_prob, P), max_gap, min_sites)
        rc = dm.region_counts(r_ctrl != r_case, reg, num, den)
        sums = dm.region_sums(counts, reg)
        for i, (a, b) in enumerate(reg):
            n, n_all, n_frac = int(b - a), int(rc[i, 0]), int(rc[i, 1])
            h_ctrl, h_case = sums[i, 2:2 + K], sums[i, 2 + K:2 + 2 * K]
            delta = 0.0
            for r in range(K):
                delta += MU[r] * int(h_case[r] - h_ctrl[r])
            rows.append([chrom, str(int(pos[a])), str(int(pos[b - 1])), str(n), str(n_all), str(n_frac),
                         repr(n_all / P), repr(n_frac / P), repr(1. - n_frac / P),
                         repr(int(sums[i, 1]) / (n * P)), repr(delta / (n * P)),
                         str(int(np.argmax(h_ctrl)) + 1), str(int(np.argmax(h_case)) + 1)])
    return rows


def _read_tsv(path):
    with open(path) as fh:
        lines = fh.read().split("\n")
    assert lines[-1] == ""
    return [ln.split("\t") for ln in lines[:-1]]


HEADER = ["chrom", "start", "end", "n_sites", "n_all", "n_frac", "prob_all", "prob_frac", "null_stat",
          "mean_site_prob", "delta_mu", "control_regime", "case_regime"]


@pytest.fixture(scope="module")
def agg_dir(tmp_path_factory):
    agg = tmp_path_factory.mktemp("agg")
    data = {"5": dm.sticky_trajectories(3000, 50, K, 31), "X": dm.sticky_trajectories(3000, 50, K, 32),
            "s": dm.sticky_trajectories(300, 40, K, 33)}
    for chrom, (r_ctrl, r_case, pos) in data.items():
        _write_chrom(agg, chrom, r_ctrl, r_case, pos)
    return agg, data


def test_get_dmrs_cli_end_to_end(agg_dir, tmp_path):
    from hygeia_amd import cli

    agg, data = agg_dir
    out = tmp_path / "dmr"
    thrs = [0.05, 0.3]
    assert cli.main(["get_dmrs", "--results_dir", str(agg), "--output_dir", str(out), "--chroms", "5,X",
                     "--fdr_thresholds", "0.05", "--fdr_thresholds", "0.3"]) == 0
    P = 50
    exp = _expected_rows(["5", "X"], data, P, 0.5, 300, 3, 4, 5)  # the flag defaults
    assert len({r[0] for r in exp}) == 2 and len(exp) > 100
    got = _read_tsv(out / "dmr_candidates.tsv")
    assert got[0] == HEADER
    assert got[1:] == exp
    t = np.array([1. - int(r[5]) / P for r in exp])
    n_sel = []
    for thr in thrs:
        _, _, threshold = od.fdr_procedure(t, thr)
        sel = [r for r, ti in zip(exp, t) if ti < threshold]
        n_sel.append(len(sel))
        got = _read_tsv(out / f"dmr_{thr}.tsv")
        assert got[0] == HEADER
        assert got[1:] == sel
    assert 0 < n_sel[-1] < len(exp) and n_sel[0] <= n_sel[-1]
    assert sorted(os.listdir(out)) == ["dmr_0.05.tsv", "dmr_0.3.tsv", "dmr_candidates.tsv"]


def test_get_dmrs_other_flags(agg_dir, tmp_path):
    """Non-default site_prob, gap, min_sites and a ratio for --min_fraction."""
    from hygeia_amd import cli

    agg, data = agg_dir
    out = tmp_path / "dmr"
    assert cli.main(["get_dmrs", "--results_dir", str(agg), "--output_dir", str(out), "--chroms", "X",
                     "--site_prob", "0.3", "--max_gap_bp", "40", "--min_sites", "2", "--min_fraction", "2/3",
                     "--fdr_thresholds", "0.2"]) == 0
    exp = _expected_rows(["X"], data, 50, 0.3, 40, 2, 2, 3)
    assert len(exp) > 50
    assert _read_tsv(out / "dmr_candidates.tsv")[1:] == exp
    t = np.array([1. - int(r[5]) / 50 for r in exp])
    _, _, threshold = od.fdr_procedure(t, 0.2)
    assert _read_tsv(out / "dmr_0.2.tsv")[1:] == [r for r, ti in zip(exp, t) if ti < threshold]


def test_get_dmrs_no_region_writes_headers(agg_dir, tmp_path):
    from hygeia_amd import cli

    agg, _ = agg_dir
    out = tmp_path / "dmr"
    assert cli.main(["get_dmrs", "--results_dir", str(agg), "--output_dir", str(out), "--chroms", "5",
                     "--max_gap_bp", "0", "--min_sites", "2"]) == 0
    for name in ("dmr_candidates.tsv", "dmr_0.01.tsv", "dmr_0.05.tsv"):
        assert _read_tsv(out / name) == [HEADER]


def test_get_dmrs_unequal_particles(agg_dir, tmp_path, capsys):
    from hygeia_amd import cli

    agg, _ = agg_dir
    assert cli.main(["get_dmrs", "--results_dir", str(agg), "--output_dir", str(tmp_path / "dmr"),
                     "--chroms", "5,s"]) == 1
    assert "chromosome s" in capsys.readouterr().err
