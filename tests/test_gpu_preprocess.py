"""SURVEY.md 8f-3 on the GPU: `hygeia preprocess` end to end (host parse,
hyg_pre_collapse on the device, np.savetxt outputs) against the restatement of
preprocess_bed.py in tests/test_preprocess.py, file by file, on synthetic
per-strand BED files: paired and single-strand CpGs, zero coverage, non-CG and
other-chromosome rows, sites outside the CpG grid, half-integer roundings,
extra columns, a missing sample file, and the all-covered case (int output).

hyg_pre_collapse itself, through the C ABI on device arrays, against the
array-level restatement in tests/pre_model.py, every output word equal and NaN
at the same places: "+" records longer than one base (the marking pass, partners
outside a chunk's window), chunks with more than 1,024 records in their span
(the searches in HBM), grids and strands past 256 * 32 chunks (a second
iteration of both kernels' loops), positions above 2^32, *conflicts, the
roundings at and next to a half, interleaved output columns and empty inputs.
Every call writes into a poisoned matrix with canary rows behind it, and
nothing but the site's two words may change."""
import functools
import gzip
import logging

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import pre_model  # noqa: E402
from tests.test_preprocess import COLS, ref_counts, same_words  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from hygeia_amd import _lib

    L = _lib.load()
    if L.hyg_device_count() <= 0:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X (gpurun)")
    return L


def synth(n_cpg, seed, chrom="22", full=False):
    rng = np.random.default_rng(seed)
    cpg1 = np.cumsum(rng.integers(2, 40, n_cpg)) + 1000  # 1-based C positions
    beds = []
    for s in range(3):
        rows = []
        for p in cpg1 - 1:  # 0-based C
            r = rng.random()
            cov_p, cov_n = int(rng.integers(0, 30)), int(rng.integers(0, 30))
            pct_p, pct_n = float(rng.choice([0.0, 50.0, 100.0, round(rng.random() * 100, 2)])), \
                float(round(rng.random() * 100, 2))
            if full:
                cov_p = max(cov_p, 1)
                r = 0.0
            if r < 0.6:
                rows += [(chrom, p, p + 1, "+", cov_p, pct_p, "CG"), (chrom, p + 1, p + 2, "-", cov_n, pct_n, "CG")]
            elif r < 0.75:
                rows.append((chrom, p, p + 1, "+", cov_p, pct_p, "CG"))
            elif r < 0.9:
                rows.append((chrom, p + 1, p + 2, "-", cov_n, pct_n, "CG"))
            elif r < 0.95:
                rows.append((chrom, p, p + 1, "+", cov_p, pct_p, "CHG"))
        if not full:
            rows += [("21", 5, 6, "+", 4, 50.0, "CG"), (chrom, int(cpg1[-1]) + 100, int(cpg1[-1]) + 101, "+", 3, 50.0,
                                                          "CG")]
        beds.append(pd.DataFrame([[c, a, b, ".", 0, st, a, b, "0,0,0", cv, pc, rf, "CG", 30, "extra"]
                                  for c, a, b, st, cv, pc, rf in rows], columns=COLS + ["x"]))
    return cpg1, beds


def write_inputs(tmp, cpg1, beds, chrom):
    cpg = pd.DataFrame({"seqID": [chrom] * len(cpg1) + ["21"], "start": list(cpg1) + [6], "end": 0})
    cpg.to_csv(tmp / "cpg.tsv", sep="\t", index=False)
    paths = []
    for s, b in enumerate(beds):
        p = tmp / f"s{s}.bed"
        with open(p, "w") as fh:
            fh.write("track header\n")
            b.to_csv(fh, sep="\t", index=False, header=False)
        paths.append(str(p))
    return paths


def read_out(path):
    with gzip.open(path, "rt") as fh:
        return fh.read()


@pytest.mark.parametrize("full", [False, True])
def test_preprocess_end_to_end(lib, tmp_path, full):
    from hygeia_amd import cli

    chrom = "22"
    cpg1, beds = synth(3000, 7 + full, chrom, full=full)
    paths = write_inputs(tmp_path, cpg1, beds, chrom)
    ctrl = [paths[0], str(tmp_path / "missing.bed")] if not full else [paths[0]]
    case = [paths[1], paths[2]]
    argv = ["preprocess", "--cpg_file_path", str(tmp_path / "cpg.tsv"), "--output_path", str(tmp_path / "out"),
            "--chromosome", chrom]
    for p in ctrl:
        argv += ["--control_data_path", p]
    for i, p in enumerate(case):
        argv += ["--case_data_path", p, "--case_id_names", f"k{i}"]
    assert cli.main(argv) == 0
    pos0 = np.sort(cpg1 - 1)
    ref = ref_counts(pos0, [beds[0]] + ([None] if not full else []) + [beds[1], beds[2]], chrom)
    has_null = np.isnan(ref).any()
    assert has_null != full
    ref = np.nan_to_num(ref)
    if not has_null:
        ref = ref.astype(np.int64)
    nc = len(ctrl)
    exp = {"positions": pos0, "cpg_sites_merged": np.array([len(pos0)]),
           "n_methylated_reads_control": ref[:, 0:2 * nc:2],
           "n_total_reads_control": ref[:, 1:2 * nc:2] + ref[:, 0:2 * nc:2],
           "n_methylated_reads_case": ref[:, 2 * nc::2], "n_total_reads_case": ref[:, 2 * nc + 1::2] + ref[:, 2 * nc::2]}
    for name, arr in exp.items():
        np.savetxt(tmp_path / f"exp_{name}.txt.gz", arr, delimiter=",", fmt="%s")
        assert read_out(tmp_path / "out" / f"{name}_{chrom}.txt.gz") == read_out(tmp_path / f"exp_{name}.txt.gz"), name
    txt = read_out(tmp_path / "out" / f"n_total_reads_case_{chrom}.txt.gz")
    assert (".0" in txt) == (not full)


def test_marking_pass_equals_single_base_path(lib):
    """hyg_pre_collapse with plus_single_base = 0 (the pre_mark_kernel pass)
    and = 1 (pairing through the grid's own lookup) agree on single-base data."""
    from hygeia_amd import _lib
    from hygeia_amd.preprocess import read_bed
    import ctypes as C

    cpg1, beds = synth(5000, 11)
    dev = torch.device("cuda", 0)
    pos0 = torch.from_numpy(np.sort(cpg1 - 1)).to(dev)
    import tempfile, os
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "s.bed")
        with open(p, "w") as fh:
            fh.write("h\n")
            beds[0].to_csv(fh, sep="\t", index=False, header=False)
        (ps, pe, pc, pp), (ms, _, mc, mp) = read_bed(p, "22")[0]
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (ps, pe, pc, pp, ms, mc, mp)]
    outs = []
    for single in (0, 1):
        out = torch.full((pos0.numel(), 2), -7.0, dtype=torch.float64, device=dev)
        scratch = torch.empty(max(len(ms), 1), dtype=torch.uint8, device=dev)
        conf = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.hyg_pre_collapse(pos0.data_ptr(), pos0.numel(), t[0].data_ptr(), t[1].data_ptr(),
                                        t[2].data_ptr(), t[3].data_ptr(), len(ps), t[4].data_ptr(), t[5].data_ptr(),
                                        t[6].data_ptr(), len(ms), single, scratch.data_ptr(), out.data_ptr(), 2, 0,
                                        conf.data_ptr(), None))
        torch.cuda.synchronize()
        assert int(conf.item()) == 0
        outs.append(out.cpu().numpy())
    np.testing.assert_array_equal(np.nan_to_num(outs[0], nan=-1), np.nan_to_num(outs[1], nan=-1))
    assert np.isfinite(outs[0]).any() and np.isnan(outs[0]).any()


# ---- hyg_pre_collapse on device arrays against tests/pre_model.py

CANARY_ROWS, POISON = 3, -7.0
CHUNK, KWIN, MAX_BLOCKS = 256, 1024, 256 * 32  # pre_kernels.hip: sites per block, LDS window, the launcher's grid cap


def poisoned(n_sites, stride=2):
    return torch.full((n_sites + CANARY_ROWS, stride), POISON, dtype=torch.float64, device=torch.device("cuda", 0))


def collapse(lib, pos0, plus, minus, single, stride=2, column=0, counts=None):
    """One hyg_pre_collapse call on device copies of the arrays, into `counts`
    ([n_sites + CANARY_ROWS][stride], poisoned when not given). Asserts that no
    word but the sites' own two changed; returns ([n_sites][2], *conflicts)."""
    from hygeia_amd import _lib

    dev = torch.device("cuda", 0)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(dev)  # noqa: E731
    ptr = lambda t: t.data_ptr() if t.numel() else None  # noqa: E731
    (ps, pe, pc, pp), (ms, mc, mp) = plus, minus
    d_pos = up(pos0, np.int64)
    d = [up(ps, np.int64), up(pe, np.int64), up(pc, np.float64), up(pp, np.float64), up(ms, np.int64),
         up(mc, np.float64), up(mp, np.float64)]
    T, n_plus, n_minus = d_pos.numel(), d[0].numel(), d[4].numel()
    assert all(t.numel() == n_plus for t in d[:4]) and all(t.numel() == n_minus for t in d[4:])
    if counts is None:
        counts = poisoned(T, stride)
    assert counts.shape == (T + CANARY_ROWS, stride) and counts.is_contiguous()
    before = counts.cpu().numpy().copy()
    scratch = torch.full((max(n_minus, 1),), 0xA5, dtype=torch.uint8, device=dev)  # the marking pass clears it itself
    conf = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(lib.hyg_pre_collapse(ptr(d_pos), T, ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), n_plus, ptr(d[4]),
                                    ptr(d[5]), ptr(d[6]), n_minus, single, None if single else scratch.data_ptr(),
                                    counts.data_ptr(), stride, column, conf.data_ptr(), None))
    torch.cuda.synchronize()
    after = counts.cpu().numpy()
    others = np.ones(after.shape, bool)
    others[:T, column:column + 2] = False
    np.testing.assert_array_equal(after.view(np.int64)[others], before.view(np.int64)[others])
    return after[:T, column:column + 2].copy(), int(conf.item())


def chunk_last(pos0, t):
    """position of the last site of the 256-site chunk that holds row t"""
    return pos0[np.minimum((t // CHUNK + 1) * CHUNK, pos0.size) - 1]


@pytest.mark.parametrize("offset", [0, 2 ** 33], ids=["low", "above_2_32"])
def test_multi_base_pairing(lib, offset):
    """1,025 sites (four chunks and one site), plus_single_base = 0: the smallest
    grid on which a "+" record's partner can lie in another chunk's window and
    the last chunk is a single site. With every position moved up by 2^33 a
    32-bit truncation anywhere would show."""
    pos0, plus, minus = pre_model.random_records(5, 1025, (1, 2, 3, 7), n_dup=6, n_long=12, n_cross=8, n_share=8,
                                                 offset=offset)
    ps, pe = plus[0], plus[1]
    assert pos0.size == 1025 and pos0[0] > offset and (offset == 0 or pos0[0] > 2 ** 32)
    sit = pre_model.situations(pos0, plus, minus)
    for k in ("paired", "multi_base", "long_paired", "plus_without_partner", "minus_without_partner",
              "matched_minus_on_a_bare_site", "shared_partner", "zero_plus_only", "zero_minus_only", "zero_both",
              "off_grid_plus", "off_grid_minus", "duplicated_sites"):
        assert sit[k] > 0, (k, sit)
    assert {1, 2, 3, 7} <= set(np.unique(pe - ps).tolist())
    # long records whose partner starts past their own chunk's last site + 1: found only by the whole-array search;
    # some of these partners start one past a grid site, which must then stay NaN
    long_ = (pe - ps > 4000) & np.isin(ps, pos0) & np.isin(pe, minus[0])
    leaves = long_ & (pe > chunk_last(pos0, np.searchsorted(pos0, ps) % pos0.size) + 1)
    assert leaves.sum() >= 6 and np.isin(pe[leaves] - 1, pos0).sum() >= 3
    assert not np.all(np.diff(pe) >= 0)  # ends out of order: the marking pass's window test has to fail sometimes
    want, conflicts = pre_model.collapse_counts(pos0, *plus, *minus)
    assert conflicts == 0
    bare = np.isin(pos0, pe[leaves] - 1) & ~np.isin(pos0, ps)
    assert bare.any() and np.isnan(want[bare]).all()
    got, n_conf = collapse(lib, pos0, plus, minus, 0)
    assert n_conf == 0
    same_words(got, want)
    dup = np.flatnonzero(np.diff(pos0) == 0)
    assert dup.size and np.isfinite(got[dup]).any()
    same_words(got[dup], got[dup + 1])
    assert np.isfinite(got).sum() > 1000 and np.isnan(got).sum() > 200


def window_records(targets, seed):
    """A grid of 256 sites per entry of `targets`, about 40 bases apart, all
    "+" records single-base. Each chunk has records on its sites (the first
    site a pair; the last a pair in even chunks and a "-" record alone in odd
    ones, starting at the chunk's last position + 1). A chunk with targets
    (P, M) gets records between its sites until exactly P "+" starts lie in
    [first, last] and M "-" starts in [first + 1, last + 1]; None leaves the
    chunk with its own records only."""
    rng = np.random.default_rng(seed)
    pos0 = 1000 + np.cumsum(rng.integers(30, 51, CHUNK * len(targets)))
    ps, ms = [], []
    for c, tgt in enumerate(targets):
        s = pos0[c * CHUNK:(c + 1) * CHUNK]
        r = rng.random(CHUNK)
        plus_on, minus_on = r < 0.6, (r < 0.4) | (r >= 0.8)
        plus_on[0] = minus_on[0] = minus_on[-1] = True
        plus_on[-1] = c % 2 == 0
        ps.append(s[plus_on])
        ms.append(s[minus_on] + 1)
        if tgt is None:
            continue
        need_p, need_m = tgt[0] - int(plus_on.sum()), tgt[1] - int(minus_on.sum())
        both = min(need_p, need_m) // 2
        pool = np.arange(s[0] + 3, s[-1] - 3, 3)  # q and q + 1 of two picks never meet
        q = rng.choice(pool[~np.isin(pool, s)], need_p + need_m - both, replace=False)
        ps.append(q[:need_p])  # the first `both` of them with a partner at q + 1
        ms += [q[:both] + 1, q[need_p:] + 1]
    ps, ms = np.sort(np.concatenate(ps)), np.sort(np.concatenate(ms))
    assert np.all(np.diff(ps) > 0) and np.all(np.diff(ms) > 0)
    cov = lambda m: rng.integers(0, 30, m).astype(np.float64)  # noqa: E731
    pct = lambda m: np.round(rng.random(m) * 100.0, 2)  # noqa: E731
    mc = cov(ms.size)
    at_end = np.isin(ms, pos0[CHUNK - 1::CHUNK] + 1)  # reads on every chunk's last "-" record: its site is not NaN
    mc[at_end] = np.maximum(mc[at_end], 1.0)
    return pos0, (ps, ps + 1, cov(ps.size), pct(ps.size)), (ms, mc, pct(ms.size))


WINDOW_LAYOUTS = {  # per chunk: ("+" starts, "-" starts) in its span
    "at_and_past_kwin": [(KWIN, KWIN + 1), (KWIN + 1, KWIN), None],
    "both_past_kwin": [(1500, 1300), None, (KWIN, KWIN)],
}


@pytest.mark.parametrize("single", [1, 0])
@pytest.mark.parametrize("layout", sorted(WINDOW_LAYOUTS))
def test_windows_around_kwin(lib, layout, single):
    """768 sites: three chunks whose spans hold exactly kWin = 1,024 records
    (the last size staged in LDS), 1,025 (the first searched in HBM, with
    global indices), both strands past kWin, or only the chunk's own."""
    targets = WINDOW_LAYOUTS[layout]
    pos0, plus, minus = window_records(targets, 21)
    assert pos0.size == 768 and 35 < np.diff(pos0).mean() < 45
    for c, tgt in enumerate(targets):
        first, last = pos0[c * CHUNK], pos0[(c + 1) * CHUNK - 1]
        n_p = np.searchsorted(plus[0], last + 1) - np.searchsorted(plus[0], first)
        n_m = np.searchsorted(minus[0], last + 2) - np.searchsorted(minus[0], first + 1)
        assert tgt is None and n_p <= CHUNK and n_m <= CHUNK or (n_p, n_m) == tgt, (c, n_p, n_m)
        # the "-" record at the chunk's last position + 1: a partner in even chunks, alone in odd ones
        assert np.isin(last + 1, minus[0]) and np.isin(first, plus[0]) and np.isin(last, plus[0]) == (c % 2 == 0)
    want, conflicts = pre_model.collapse_counts(pos0, *plus, *minus)
    assert conflicts == 0
    ends = np.arange(CHUNK - 1, pos0.size, CHUNK)
    assert np.isfinite(want[ends]).all()
    got, n_conf = collapse(lib, pos0, plus, minus, single)
    assert n_conf == 0
    same_words(got, want)
    assert np.isfinite(got).sum() > 800 and np.isnan(got).sum() > 100


N_LOOP = MAX_BLOCKS * CHUNK + 257  # 8,194 chunks on 8,192 blocks: blocks 0 and 1 run a second iteration


@functools.lru_cache(maxsize=1)
def loop_case(single):
    if single:
        pos0, plus, minus = pre_model.random_records(31, N_LOOP, (1,), off_grid=0.45, max_gap=12)
    else:
        pos0, plus, minus = pre_model.random_records(32, N_LOOP, (1, 1, 2, 3), n_long=16, n_cross=16, n_share=16,
                                                     off_grid=0.45, max_gap=12)
    return pos0, plus, minus, pre_model.collapse_counts(pos0, *plus, *minus)


@pytest.mark.parametrize("single", [1, 0])
def test_grid_stride_loops(lib, single):
    """2,097,409 sites and more "+" records than that: the smallest sizes (plus
    a chunk and a site) at which pre_grid_kernel's and pre_mark_kernel's loops
    run a second iteration, with their barriers and the `continue` of the
    threads past the end."""
    pos0, plus, minus, (want, conflicts) = loop_case(single)
    assert pos0.size == N_LOOP == 2_097_409 and plus[0].size > MAX_BLOCKS * CHUNK and conflicts == 0
    assert bool(np.all(plus[1] == plus[0] + 1)) == bool(single)
    tail = want[MAX_BLOCKS * CHUNK:]  # the second iteration's sites
    assert tail.shape[0] == 257 and np.isfinite(tail).sum() > 100 and np.isnan(tail).sum() > 20
    minus_only = ~np.isin(minus[0], plus[1]) & (minus[1] > 0) & np.isin(minus[0] - 1, pos0[MAX_BLOCKS * CHUNK:])
    assert minus_only.sum() > 5
    # "+" records of the marking pass's second iteration with a partner
    assert single or np.isin(plus[1][MAX_BLOCKS * CHUNK:], minus[0]).sum() > 100
    got, n_conf = collapse(lib, pos0, plus, minus, single)
    assert n_conf == 0
    same_words(got, want)


def conflict_case(conflicts_at, near_miss_at, zero_plus_at=()):
    """601 grid rows 10 bases apart (three chunks; position 300 twice), a
    single-base pair on every site, except
      conflicts_at: "+" (k, k + 3) with nothing at k + 3, and "-" at k + 1 that
        no "+" record ends at: two collapsed rows with key k
      near_miss_at: the same, plus a longer "+" record (k - 4, k + 1) that the
        "-" record at k + 1 pairs with: one row with key k
      zero_plus_at: a conflict whose "+" record has coverage 0
    All other coverages are positive."""
    rng = np.random.default_rng(77)
    site = 1000 + 10 * np.arange(600)
    pos0 = np.sort(np.concatenate([site, site[300:301]]))
    odd = np.zeros(600, bool)
    odd[list(conflicts_at) + list(near_miss_at) + list(zero_plus_at)] = True
    ps = np.concatenate([site, site[list(near_miss_at)] - 4])
    pe = np.concatenate([np.where(odd, site + 3, site + 1), site[list(near_miss_at)] + 1])
    order = np.argsort(ps)
    ps, pe = ps[order], pe[order]
    pc = rng.integers(1, 30, ps.size).astype(np.float64)
    pc[np.isin(ps, site[list(zero_plus_at)])] = 0.0
    ms = site + 1
    pp, mc, mp = np.round(rng.random(ps.size) * 100, 2), rng.integers(1, 30, 600).astype(np.float64), \
        np.round(rng.random(600) * 100, 2)
    return pos0, (ps, pe, pc, pp), (ms, mc, mp)


def test_conflicts_are_counted(lib):
    """*conflicts: grid rows whose position two collapsed rows claim, in the
    first and the last chunk and on a duplicated position (two rows); every
    other site keeps the restatement's values."""
    at = [3, 100, 300, 590, 599]
    pos0, plus, minus = conflict_case(at, [50, 450])
    assert (plus[2] > 0).all() and (minus[1] > 0).all() and (np.diff(pos0) == 0).sum() == 1
    want, conflicts, claimed = pre_model.collapse_counts(pos0, *plus, *minus, return_claimed=True)
    bad = pre_model.conflicted_sites(pos0, plus[0], plus[1], minus[0])
    assert conflicts == claimed == bad.sum() == len(at) + 1
    np.testing.assert_array_equal(pos0[bad], 1000 + 10 * np.array([3, 100, 300, 300, 590, 599]))
    assert bad[:CHUNK].any() and bad[2 * CHUNK:].any()
    got, n_conf = collapse(lib, pos0, plus, minus, 0)
    assert n_conf == conflicts
    same_words(got[~bad], want[~bad])
    assert np.isfinite(got[~bad]).all()


def test_near_misses_are_no_conflicts(lib):
    """A "+" record at k that ends past k + 1 and a "-" record at k + 1 that a
    longer "+" record ends at: one collapsed row with key k, no conflict."""
    pos0, plus, minus = conflict_case([], [2, 50, 255, 256, 450, 599])
    want, conflicts, claimed = pre_model.collapse_counts(pos0, *plus, *minus, return_claimed=True)
    assert conflicts == claimed == 0
    got, n_conf = collapse(lib, pos0, plus, minus, 0)
    assert n_conf == 0
    same_words(got, want)
    assert np.isfinite(got).all()


def test_conflict_with_a_row_of_coverage_zero_is_counted(lib):
    """include/hygeia_amd.h: *conflicts counts a site two collapsed rows claim
    even when one of them has coverage 0, a row the reference's filter drops
    before its joins (so the reference has no conflict there: conservative)."""
    pos0, plus, minus = conflict_case([], [50], zero_plus_at=[200, 400])
    want, conflicts, claimed = pre_model.collapse_counts(pos0, *plus, *minus, return_claimed=True)
    assert (conflicts, claimed) == (0, 2)
    bad = pre_model.conflicted_sites(pos0, plus[0], plus[1], minus[0])
    np.testing.assert_array_equal(pos0[bad], [3000, 5000])
    assert np.isfinite(want[bad]).all()  # the reference keeps the "-" record's row there
    got, n_conf = collapse(lib, pos0, plus, minus, 0)
    assert n_conf == claimed
    same_words(got[~bad], want[~bad])


@pytest.mark.parametrize("single", [1, 0])
def test_rounding_at_and_next_to_a_half(lib, single):
    """Single-record sites whose count is an exact half (odd coverage at 50
    percent: up, away from zero), the f64 next to one (coverage 1 at the double
    below 50 percent: total * avg / 100 = 0.49999999999999994, which
    floor(x + 0.5) would send to 1), percent 0 and 100, and a pair whose
    average is a repeating fraction."""
    below, above = np.nextafter(50.0, 0.0), np.nextafter(50.0, 100.0)
    odd = np.arange(1, 40, 2, dtype=np.float64)
    rows = [(1.0, below, None)]                                  # -> 0, 1
    rows += [(c, 50.0, None) for c in odd]                       # halves -> (c + 1) / 2 twice
    rows += [(c, below, None) for c in odd] + [(c, above, None) for c in odd]
    rows += [(c, p, None) for c in (1.0, 2.0, 7.0, 30.0) for p in (0.0, 100.0)]
    rows += [(None, None, (c, 50.0)) for c in odd]               # "-" records alone
    rows += [(None, None, (1.0, below))]
    rows += [(1.0, 100.0, (2.0, 0.0)), (2.0, 100.0, (1.0, 0.0)), (1.0, 50.0, (2.0, 100.0)), (3.0, 50.0, (4.0, 50.0))]
    pos0 = 500 + 4 * np.arange(len(rows))
    has_p = np.array([r[0] is not None for r in rows])
    has_m = np.array([r[2] is not None for r in rows])
    plus = (pos0[has_p], pos0[has_p] + 1, np.array([r[0] for r in rows if r[0] is not None]),
            np.array([r[1] for r in rows if r[0] is not None]))
    minus = (pos0[has_m] + 1, np.array([r[2][0] for r in rows if r[2]]), np.array([r[2][1] for r in rows if r[2]]))
    want, conflicts = pre_model.collapse_counts(pos0, *plus, *minus)
    assert conflicts == 0 and np.isfinite(want).all()
    # by hand
    np.testing.assert_array_equal(want[0], [0.0, 1.0])
    np.testing.assert_array_equal(want[1:21], np.stack([(odd + 1) / 2, (odd + 1) / 2], 1))
    np.testing.assert_array_equal(want[61:69], [[0, 1], [1, 0], [0, 2], [2, 0], [0, 7], [7, 0], [0, 30], [30, 0]])
    np.testing.assert_array_equal(want[69:89], np.stack([(odd + 1) / 2, (odd + 1) / 2], 1))
    np.testing.assert_array_equal(want[[89, 90, 91, 93]], [[0, 1], [1, 2], [2, 1], [4, 4]])
    avg = ((1.0 * below) + (0.0 * 0.0)) / 1.0
    assert (1.0 * avg) / 100.0 == 0.49999999999999994 and np.floor((1.0 * avg) / 100.0 + 0.5) == 1.0
    got, n_conf = collapse(lib, pos0, plus, minus, single)
    assert n_conf == 0
    same_words(got, want)


def test_interleaved_columns(lib):
    """Three samples into one [n_sites][6] matrix (stride 6, columns 0, 2, 4):
    each call leaves the other four columns as they were (collapse() checks
    every word it may not touch), and the matrix equals three stride-2 runs."""
    n = 700  # two chunks and an odd rest
    cases = [pre_model.random_records(40 + s, n, (1, 2, 3, 7), n_dup=3, n_long=4, n_cross=4, n_share=4, grid_seed=40)
             for s in range(3)]
    pos0 = cases[0][0]
    assert all(np.array_equal(c[0], pos0) for c in cases) and not np.array_equal(cases[0][1][0], cases[1][1][0])
    counts = poisoned(n, 6)
    for s in (1, 2, 0):
        _, plus, minus = cases[s]
        got, n_conf = collapse(lib, pos0, plus, minus, 0, stride=6, column=2 * s, counts=counts)
        want, conflicts = pre_model.collapse_counts(pos0, *plus, *minus)
        assert n_conf == conflicts == 0
        same_words(got, want)
        alone, _ = collapse(lib, pos0, plus, minus, 0)
        same_words(got, alone)
    full = counts.cpu().numpy()
    assert (full[n:] == POISON).all() and not (full[:n] == POISON).any()
    for s in range(3):
        same_words(full[:n, 2 * s:2 * s + 2], pre_model.collapse_counts(pos0, *cases[s][1], *cases[s][2])[0])


@pytest.mark.parametrize("single", [1, 0])
def test_empty_strands_and_tiny_grids(lib, single):
    lengths = (1,) if single else (1, 2, 3, 7)
    pos0, plus, minus = pre_model.random_records(50, 300, lengths, n_dup=2)
    none_p, none_m = tuple(a[:0] for a in plus), tuple(a[:0] for a in minus)
    for p, m in ((none_p, minus), (plus, none_m), (none_p, none_m)):
        want, conflicts = pre_model.collapse_counts(pos0, *p, *m)
        got, n_conf = collapse(lib, pos0, p, m, single)
        assert n_conf == conflicts == 0
        same_words(got, want)
        assert np.isnan(got).all() == (p is none_p and m is none_m) and np.isnan(got).any()
    # one site: a pair, a "-" record alone, nothing; then no site at all
    k = int(plus[0][np.isin(plus[0], pos0) & np.isin(plus[1], minus[0]) & (plus[2] > 0)][0])
    alone = minus[0][~np.isin(minus[0], plus[1]) & np.isin(minus[0] - 1, pos0) & (minus[1] > 0)]
    for site, finite in ((k, True), (int(alone[0]) - 1, True), (int(pos0[0]) - 1, False)):
        want, _ = pre_model.collapse_counts([site], *plus, *minus)
        got, n_conf = collapse(lib, [site], plus, minus, single)
        assert n_conf == 0 and got.shape == (1, 2) and np.isfinite(want).all() == finite
        same_words(got, want)
    got, n_conf = collapse(lib, [], plus, minus, single)  # HYG_OK (collapse() checks), the canary rows untouched
    assert got.shape == (0, 2) and n_conf == 0


# ---- the command on records longer than one base

def synth_two_base(n_cpg, seed, chrom="22", n_conflicts=0):
    """synth() with "+" records two bases long and their "-" partner at start + 2;
    n_conflicts "+" records get an unpaired "-" record at start + 1 instead."""
    rng = np.random.default_rng(seed)
    cpg1 = np.cumsum(rng.integers(2, 40, n_cpg)) + 1000
    rows = []
    clash = set(rng.choice(n_cpg, n_conflicts, replace=False).tolist())
    for i, p in enumerate(cpg1 - 1):
        r = rng.random()
        cov_p, cov_n = int(rng.integers(0, 30)), int(rng.integers(0, 30))
        pct_p, pct_n = float(rng.choice([0.0, 50.0, 100.0, round(rng.random() * 100, 2)])), \
            float(round(rng.random() * 100, 2))
        if i in clash:
            rows += [(chrom, p, p + 2, "+", cov_p + 1, pct_p, "CG"), (chrom, p + 1, p + 2, "-", cov_n + 1, pct_n, "CG")]
        elif r < 0.6:
            rows += [(chrom, p, p + 2, "+", cov_p, pct_p, "CG"), (chrom, p + 2, p + 3, "-", cov_n, pct_n, "CG")]
        elif r < 0.75:
            rows.append((chrom, p, p + 2, "+", cov_p, pct_p, "CG"))
        elif r < 0.9:
            rows.append((chrom, p + 1, p + 2, "-", cov_n, pct_n, "CG"))
    bed = pd.DataFrame([[c, a, b, ".", 0, st, a, b, "0,0,0", cv, pc, rf, "CG", 30, "extra"]
                        for c, a, b, st, cv, pc, rf in rows], columns=COLS + ["x"])
    return cpg1, bed


def test_preprocess_two_base_records_end_to_end(lib, tmp_path):
    from hygeia_amd import cli

    chrom = "22"
    cpg1, b0 = synth_two_base(3000, 61, chrom)
    beds = [b0, synth_two_base(3000, 61, chrom)[1].sample(frac=0.9, random_state=1).sort_values("start"),
            synth(3000, 61, chrom)[1][0]]
    assert np.array_equal(cpg1, synth(3000, 61, chrom)[0])
    paths = write_inputs(tmp_path, cpg1, beds, chrom)
    argv = ["preprocess", "--cpg_file_path", str(tmp_path / "cpg.tsv"), "--output_path", str(tmp_path / "out"),
            "--chromosome", chrom, "--control_data_path", paths[0], "--case_data_path", paths[1],
            "--case_data_path", paths[2]]
    assert cli.main(argv) == 0
    pos0 = np.sort(cpg1 - 1)
    ref = ref_counts(pos0, beds, chrom)
    two = b0[(b0["strand"] == "+")]
    assert ((two["end"] - two["start"]) == 2).all() and np.isin(two["end"], b0[b0["strand"] == "-"]["start"]).sum() > 1000
    assert np.isnan(ref).any() and np.isfinite(ref[:, 0]).sum() > 2000
    ref = np.nan_to_num(ref)
    exp = {"positions": pos0, "cpg_sites_merged": np.array([len(pos0)]),
           "n_methylated_reads_control": ref[:, 0:2:2], "n_total_reads_control": ref[:, 1:2:2] + ref[:, 0:2:2],
           "n_methylated_reads_case": ref[:, 2::2], "n_total_reads_case": ref[:, 3::2] + ref[:, 2::2]}
    assert len(exp) == 6
    for name, arr in exp.items():
        np.savetxt(tmp_path / f"exp_{name}.txt.gz", arr, delimiter=",", fmt="%s")
        assert read_out(tmp_path / "out" / f"{name}_{chrom}.txt.gz") == read_out(tmp_path / f"exp_{name}.txt.gz"), name


def test_preprocess_refuses_conflicting_records(lib, tmp_path, caplog):
    from hygeia_amd import cli

    chrom = "22"
    cpg1, bed = synth_two_base(3000, 62, chrom, n_conflicts=7)
    paths = write_inputs(tmp_path, cpg1, [bed], chrom)
    with caplog.at_level(logging.ERROR):
        rc = cli.main(["preprocess", "--cpg_file_path", str(tmp_path / "cpg.tsv"), "--output_path",
                       str(tmp_path / "out"), "--chromosome", chrom, "--control_data_path", paths[0]])
    assert rc == 1
    errors = [r.getMessage() for r in caplog.records if r.levelno >= logging.ERROR]
    assert len(errors) == 1 and "7 CpG sites claimed by two collapsed rows" in errors[0], errors
    out = tmp_path / "out"
    assert not out.exists() or list(out.iterdir()) == []
