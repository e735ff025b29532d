"""SURVEY.md 8f-3 on CPU: a restatement of src/two_group/preprocess_bed.py's
join semantics (polars 1.8.2 full joins, strand collapse, rounding) written
here with pandas, checked on hand-computed cases; the flag validation of
`hygeia preprocess`. The device path is compared with this restatement in
tests/test_gpu_preprocess.py. polars is absent, so against the reference
itself the outputs are parity unpinned (the restatement follows its source).
Also: the rounding pinned against exact decimal arithmetic, the array-level
restatement the large GPU cases use (tests/pre_model.py) against the pandas
one, and the arguments hyg_pre_collapse refuses before it looks for a device."""
import decimal

import numpy as np
import pandas as pd
import pytest

from hygeia_amd import _lib, cli
from tests import pre_model

COLS = ["chr", "start", "end", "name", "score", "strand", "thickStart", "thickEnd", "itemRgb", "coverage",
        "percent_methylated", "ref_genotype", "sample_genotype", "quality_score"]


def polars_round(x):
    """Rust f64::round (half away from zero): numpy's rint is exact but sends
    ties to the even neighbour, so only the ties (a fraction of exactly one half;
    x - trunc(x) is exact in f64) are moved. floor(|x| + 0.5) is not it: the sum
    rounds 0.49999999999999994 + 0.5 up to 1.0."""
    x = np.asarray(x, dtype=np.float64)
    t = np.trunc(x)
    return np.where(np.abs(x - t) == 0.5, t + np.sign(x), np.rint(x))


def ref_collapse(bed: pd.DataFrame, chrom: str) -> pd.DataFrame:
    """read_bed_file filter (:160-168) + collapse_strands (:183-259)"""
    b = bed[(bed["chr"].astype(str) == chrom) & (bed["ref_genotype"] == "CG")]
    pos, neg = b[b["strand"] == "+"], b[b["strand"] == "-"]
    m = pos.merge(neg, left_on=["chr", "end"], right_on=["chr", "start"], how="outer", suffixes=("", "_neg"))
    cp = m["coverage"].fillna(0).astype(float)
    cn = m["coverage_neg"].fillna(0).astype(float)
    pp = m["percent_methylated"].fillna(0).astype(float)
    pn = m["percent_methylated_neg"].fillna(0).astype(float)
    total = cp + cn
    start = m["start"].where(m["start"].notna(), m["start_neg"] - 1)
    keep = total > 0
    avg = ((cp * pp) + (cn * pn)) / total
    return pd.DataFrame({"start": start[keep].astype(np.int64), "total": total[keep], "avg": avg[keep]})


def ref_counts(cpg_pos0, beds, chrom):
    """process_sample_data + the Pos0 joins + extract_count_arrays: per sample
    (meth, unmeth) on the CpG grid, NaN where the sample has no collapsed row."""
    out = np.full((len(cpg_pos0), 2 * len(beds)), np.nan)
    idx = {int(p): i for i, p in enumerate(cpg_pos0)}
    for s, bed in enumerate(beds):
        if bed is None:
            continue
        c = ref_collapse(bed, chrom)
        meth = polars_round((c["total"] * c["avg"]) / 100.0)
        unmeth = polars_round((c["total"] * (100.0 - c["avg"])) / 100.0)
        for k, a, b in zip(c["start"], meth, unmeth):
            if int(k) in idx:
                out[idx[int(k)], 2 * s] = a
                out[idx[int(k)], 2 * s + 1] = b
    return out


def bed_rows(rows):
    """rows of (chr, start, end, strand, coverage, percent, ref)"""
    return pd.DataFrame([[c, s, e, ".", 0, st, s, e, "0,0,0", cov, pct, ref, "CG", 30]
                         for c, s, e, st, cov, pct, ref in rows], columns=COLS)


def test_restatement_hand_cases():
    bed = bed_rows([
        ("22", 100, 101, "+", 3, 50.0, "CG"),    # paired with the "-" at 101: total 5, avg 40 -> 2, 3
        ("22", 101, 102, "-", 2, 25.0, "CG"),
        ("22", 200, 201, "+", 5, 50.0, "CG"),    # "+" only: 2.5 -> 3 (half away from zero), 2.5 -> 3
        ("22", 301, 302, "-", 4, 100.0, "CG"),   # "-" only: key 300
        ("22", 400, 401, "+", 0, 0.0, "CG"),     # coverage 0: dropped (null -> 0, NaN here)
        ("22", 500, 501, "+", 9, 10.0, "CH"),    # not CG
        ("21", 600, 601, "+", 9, 10.0, "CG"),    # other chromosome
        ("22", 700, 701, "+", 7, 30.0, "CG"),    # not a CpG site of the grid: dropped
    ])
    got = ref_counts(np.array([100, 200, 300, 400, 500, 600, 900]), [bed], "22")
    exp = [[2, 3], [3, 3], [4, 0], [np.nan, np.nan], [np.nan, np.nan], [np.nan, np.nan], [np.nan, np.nan]]
    np.testing.assert_array_equal(got, np.array(exp, float))
    assert polars_round(np.array([0.5, 1.5, 2.5, -0.5]))[2] == 3.0


def test_flag_validation(tmp_path, capsys):
    assert cli.main(["preprocess", "--chromosome", "22"]) == 1  # no --cpg_file_path
    assert cli.main(["preprocess", "--cpg_file_path", str(tmp_path / "x.tsv")]) == 1  # no samples
    assert cli.main(["preprocess", "--cpg_file_path", str(tmp_path / "x.tsv"), "--case_data_path", "a.bed",
                     "--case_id_names", "a", "--case_id_names", "b"]) == 1  # names != paths
    assert cli.main(["preprocess", "--cpg_file_path", str(tmp_path / "missing.tsv"),
                     "--control_data_path", "a.bed"]) == 1  # CpG file not found
    assert cli.main(["preprocess", "--bogus", "1"]) == 1


# ---- the array-level restatement (tests/pre_model.py) against the pandas one

def bed_of(plus, minus, chrom="22"):
    """the records of tests/pre_model.py's arrays as a BED frame ("-" records one base long)"""
    (ps, pe, pc, pp), (ms, mc, mp) = plus, minus
    return bed_rows([(chrom, int(s), int(e), "+", c, p, "CG") for s, e, c, p in zip(ps, pe, pc, pp)] +
                    [(chrom, int(s), int(s) + 1, "-", c, p, "CG") for s, c, p in zip(ms, mc, mp)])


def same_words(got, want):
    """every f64 word equal, NaN at the same places"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan)
    np.testing.assert_array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64))


HALVES = [0.49999999999999994, 0.5, 1.5, 2.5, -0.5, 2.0 ** 52 + 1.0]


def exact_round(x: float) -> float:
    """half away from zero in exact decimal arithmetic (every double is a finite decimal)"""
    d = decimal.Decimal(x)
    r = abs(d).to_integral_value(rounding=decimal.ROUND_HALF_UP)
    return float(-r if d < 0 else r)


@pytest.mark.parametrize("rnd", [polars_round, pre_model.round_half_away], ids=["polars_round", "round_half_away"])
def test_rounding_is_half_away_from_zero_exactly(rnd):
    np.testing.assert_array_equal(rnd(np.array(HALVES)), [0.0, 1.0, 2.0, 3.0, -1.0, 2.0 ** 52 + 1.0])
    rng = np.random.default_rng(3)
    whole = rng.integers(0, 1000, 2000).astype(np.float64)
    x = np.concatenate([HALVES, whole + 0.5, np.nextafter(whole + 0.5, 0.0), np.nextafter(whole + 0.5, 2000.0),
                        -(whole + 0.5), rng.random(2000) * 100.0, whole, [2.0 ** 52 - 0.5, 2.0 ** 53, 0.0, 1e300]])
    np.testing.assert_array_equal(rnd(x), [exact_round(float(v)) for v in x])
    # the case that reaches the difference: "+" coverage 1 at just under 50 percent, no "-" record
    pct = np.nextafter(50.0, 0.0)
    avg = ((1.0 * pct) + (0.0 * 0.0)) / 1.0
    assert (1.0 * avg) / 100.0 == 0.49999999999999994
    assert rnd(np.array([(1.0 * avg) / 100.0]))[0] == 0.0 and np.floor(np.abs((1.0 * avg) / 100.0) + 0.5) == 1.0


@pytest.mark.parametrize("seed, lengths", [(1, (1,)), (2, (1, 2, 3, 7))], ids=["single_base", "multi_base"])
def test_array_restatement_equals_the_pandas_one(seed, lengths):
    multi = len(lengths) > 1
    pos0, plus, minus = pre_model.random_records(seed, 4000, lengths, n_dup=25, n_long=6 * multi, n_cross=6 * multi,
                                                 n_share=6 * multi)
    assert pos0.size == 4000 and np.all(np.diff(pos0) >= 0)
    for a in (plus[0], minus[0]):
        assert np.all(np.diff(a) > 0)
    sit = pre_model.situations(pos0, plus, minus)
    need = ["paired", "plus_without_partner", "minus_without_partner", "zero_plus_only", "zero_minus_only",
            "zero_both", "off_grid_plus", "off_grid_minus", "duplicated_sites"]
    if multi:
        need += ["multi_base", "long_paired", "matched_minus_on_a_bare_site", "shared_partner"]
    else:
        assert sit["multi_base"] == 0 and np.all(plus[1] == plus[0] + 1)
    assert all(sit[k] > 0 for k in need), sit
    got, conflicts, claimed = pre_model.collapse_counts(pos0, *plus, *minus, return_claimed=True)
    assert conflicts == 0 and claimed == 0
    want = ref_counts(pos0, [bed_of(plus, minus)], "22")
    # ref_counts writes a duplicated grid position once (its dict keeps the last row): both rows carry the value
    first = np.searchsorted(pos0, pos0)
    last = np.searchsorted(pos0, pos0, side="right") - 1
    assert np.isnan(want[first[first != last]]).all()
    same_words(got, want[last])
    assert np.isfinite(got).any() and np.isnan(got).any()


def test_array_restatement_on_the_hand_cases():
    pos0 = np.array([100, 200, 300, 400, 500, 600, 900])
    got, conflicts = pre_model.collapse_counts(pos0, [100, 200, 400, 700], [101, 201, 401, 701], [3, 5, 0, 7],
                                               [50.0, 50.0, 0.0, 30.0], [101, 301], [2, 4], [25.0, 100.0])
    exp = [[2, 3], [3, 3], [4, 0], [np.nan, np.nan], [np.nan, np.nan], [np.nan, np.nan], [np.nan, np.nan]]
    same_words(got, np.array(exp, float))
    assert conflicts == 0
    bed = bed_rows([("22", 100, 101, "+", 3, 50.0, "CG"), ("22", 101, 102, "-", 2, 25.0, "CG"),
                    ("22", 200, 201, "+", 5, 50.0, "CG"), ("22", 301, 302, "-", 4, 100.0, "CG"),
                    ("22", 400, 401, "+", 0, 0.0, "CG"), ("22", 700, 701, "+", 7, 30.0, "CG")])
    same_words(got, ref_counts(pos0, [bed], "22"))
    # empty strands and an empty grid
    nan2 = np.full((2, 2), np.nan)
    same_words(pre_model.collapse_counts([5, 9], [], [], [], [], [], [], [])[0], nan2)
    same_words(pre_model.collapse_counts([5, 9], [], [], [], [], [6], [4], [25.0])[0], [[1, 3], [np.nan, np.nan]])
    same_words(pre_model.collapse_counts([5, 9], [9], [12], [4], [25.0], [], [], [])[0], [[np.nan, np.nan], [1, 3]])
    assert pre_model.collapse_counts([], [9], [12], [4], [25.0], [12], [1], [0.0])[0].shape == (0, 2)


def test_array_restatement_counts_conflicts():
    """A "+" record at k that does not end at k + 1 and a "-" record at k + 1
    no "+" record ends at: two rows with key k, once per grid row at k; a row
    of coverage 0 is dropped first (`claimed` counts it all the same)."""
    pos0 = [10, 20, 20, 30, 40]
    plus = ([10, 20, 30, 38], [12, 23, 32, 41], [1, 1, 0, 1], [0.0] * 4)
    minus = ([11, 21, 31, 41], [1, 1, 1, 1], [100.0] * 4)
    out, conflicts, claimed = pre_model.collapse_counts(pos0, *plus, *minus, return_claimed=True)
    assert (conflicts, claimed) == (3, 4)  # 10, 20 twice; 30 has a "+" row of coverage 0; 41 is the partner of 38
    np.testing.assert_array_equal(pre_model.conflicted_sites(pos0, plus[0], plus[1], minus[0]),
                                  [True, True, True, True, False])
    same_words(out[3:], [[1, 0], [np.nan, np.nan]])


# ---- what hyg_pre_collapse refuses before it looks for a device

def test_pre_collapse_refusals():
    L = _lib.load()
    buf = np.zeros(8, np.int64)  # never read: every call below returns before anything is enqueued
    p = buf.ctypes.data
    names = ["pos0", "T", "plus_start", "plus_end", "plus_cov", "plus_pct", "n_plus", "minus_start", "minus_cov",
             "minus_pct", "n_minus", "single", "scratch", "counts", "stride", "column", "conflicts", "stream"]
    good = dict(pos0=p, T=1, plus_start=p, plus_end=p, plus_cov=p, plus_pct=p, n_plus=1, minus_start=p, minus_cov=p,
                minus_pct=p, n_minus=1, single=0, scratch=p, counts=p, stride=2, column=0, conflicts=p, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return L.hyg_pre_collapse(*[a[n] for n in names])

    refused = [dict(stride=1), dict(stride=0), dict(stride=-2), dict(column=-1), dict(column=1), dict(stride=6, column=5),
               dict(stride=3, column=2), dict(T=-1), dict(n_plus=-1), dict(n_minus=-1),
               dict(pos0=None), dict(counts=None), dict(conflicts=None),
               dict(plus_start=None), dict(plus_end=None), dict(plus_cov=None), dict(plus_pct=None),
               dict(minus_start=None), dict(minus_cov=None), dict(minus_pct=None), dict(scratch=None)]
    for kw in refused:
        assert call(**kw) == _lib.HYG_EINVAL, kw
        assert L.hyg_last_error()
    # a size of 0 asks for none of its buffers; with no site nothing is launched (HYG_OK on a device, else HYG_EDEVICE)
    accepted = (_lib.HYG_OK, _lib.HYG_EDEVICE)
    none_plus = dict(plus_start=None, plus_end=None, plus_cov=None, plus_pct=None)
    none_minus = dict(minus_start=None, minus_cov=None, minus_pct=None, scratch=None)
    assert call(T=0, pos0=None, counts=None, conflicts=None, n_plus=0, n_minus=0, **none_plus, **none_minus) in accepted
    assert call(T=0, n_plus=0, single=1, **none_plus) in accepted
    assert call(T=0, n_minus=0, single=1, **none_minus) in accepted
    # plus_single_base = 1 needs no scratch; = 0 does
    assert call(T=0, single=1, scratch=None) in accepted
    assert call(T=0, single=0, scratch=None) == _lib.HYG_EINVAL
    assert call(T=0, single=1, stride=6, column=4, scratch=None) in accepted
