"""numpy restatement of hyg_pre_collapse (TEST INFRASTRUCTURE ONLY).

Written from the join semantics of src/two_group/preprocess_bed.py that
tests/test_preprocess.py restates with pandas (ref_collapse / ref_counts), over
whole arrays: no chunks, no windows, no per-site loop, so it serves the
2-million-site grids that ref_counts' per-row dict walk cannot. For one sample
on one chromosome, each strand's records sorted by start with unique starts:

  every "+" record (s, e, cov, pct) is a collapsed row with key s; its partner
    is the "-" record starting at e (two "+" records may share one partner)
  every "-" record (s, cov, pct) that no "+" record ends at is a collapsed row
    with key s - 1
  a missing strand has coverage 0 and percent 0; total = cov+ + cov-; rows
    with total > 0 are kept; avg = (cov+ pct+ + cov- pct-) / total
  meth = round(total avg / 100), unmeth = round(total (100 - avg) / 100), half
    away from zero (Rust f64::round, what polars rounds with)
  a grid site with position k takes the kept row with key k, else NaN, NaN

All arithmetic is f64 + * / in the order written above, so a device built
without FMA contraction equals it bit for bit.

conflicts = the number of grid rows whose position is the key of two kept
rows (the reference's joins would multiply such rows; the values returned
there are those of one of the two rows and mean nothing). Two rows can share a
key k only as a "+" record starting at k plus an unpaired "-" record starting
at k + 1. `claimed` counts the same before the total > 0 filter: what the
device reports in *conflicts, which also counts a site one of whose two rows
the filter would have dropped.
"""
from __future__ import annotations

import numpy as np


def round_half_away(x) -> np.ndarray:
    """Rust f64::round: to the nearest integer, halves away from zero. a -
    floor(a) is exact in f64 (the fraction of a double is a double), so the
    comparison with 0.5 sees the true fraction; floor(a + 0.5) does not
    (0.49999999999999994 + 0.5 rounds up to 1.0)."""
    x = np.asarray(x, dtype=np.float64)
    a = np.abs(x)
    f = np.floor(a)
    return np.copysign(np.where(a - f >= 0.5, f + 1.0, f), x)


def collapse_counts(pos0, plus_start, plus_end, plus_cov, plus_pct, minus_start, minus_cov, minus_pct,
                    return_claimed=False):
    """([n_sites][2] f64 (meth, unmeth) with NaN, conflicts[, claimed]) for the
    arrays hyg_pre_collapse takes; pos0 sorted, duplicates allowed."""
    pos0 = np.asarray(pos0, np.int64)
    ps, pe, ms = (np.asarray(a, np.int64) for a in (plus_start, plus_end, minus_start))
    pc, pp, mc, mp = (np.asarray(a, np.float64) for a in (plus_cov, plus_pct, minus_cov, minus_pct))
    # "+" rows with their partners
    j = np.searchsorted(ms, pe)
    jc = np.minimum(j, max(ms.size - 1, 0))
    paired = (j < ms.size) & (ms[jc] == pe) if ms.size else np.zeros(pe.size, bool)
    cn = np.where(paired, mc[jc], 0.0) if ms.size else np.zeros(pe.size)
    pn = np.where(paired, mp[jc], 0.0) if ms.size else np.zeros(pe.size)
    # "-" rows no "+" record ends at
    alone = ~np.isin(ms, pe)
    key = np.concatenate([ps, ms[alone] - 1])
    cov_p = np.concatenate([pc, np.zeros(alone.sum())])
    pct_p = np.concatenate([pp, np.zeros(alone.sum())])
    cov_n = np.concatenate([cn, mc[alone]])
    pct_n = np.concatenate([pn, mp[alone]])
    total = cov_p + cov_n
    claimed = int(conflicted_sites(pos0, ps, pe, ms).sum())
    keep = total > 0
    key, total = key[keep], total[keep]
    avg = ((cov_p[keep] * pct_p[keep]) + (cov_n[keep] * pct_n[keep])) / total
    meth = round_half_away((total * avg) / 100.0)
    unmeth = round_half_away((total * (100.0 - avg)) / 100.0)
    # left join onto the grid
    out = np.full((pos0.size, 2), np.nan)
    uniq, first, count = np.unique(key, return_index=True, return_counts=True)
    if uniq.size:
        i = np.minimum(np.searchsorted(uniq, pos0), uniq.size - 1)
        hit = uniq[i] == pos0
        out[hit, 0] = meth[first[i[hit]]]
        out[hit, 1] = unmeth[first[i[hit]]]
        conflicts = int((hit & (count[i] > 1)).sum())
    else:
        conflicts = 0
    return (out, conflicts, claimed) if return_claimed else (out, conflicts)


def random_records(seed, n_sites, lengths=(1,), n_dup=0, n_long=0, n_cross=0, n_share=0, offset=0, off_grid=0.4,
                   max_gap=20, grid_seed=None):
    """(pos0, (plus_start, plus_end, plus_cov, plus_pct), (minus_start, minus_cov,
    minus_pct)) with whole-array numpy calls: a sorted grid of n_sites rows of
    which n_dup repeat a position, 2 .. max_gap - 1 bases apart from `offset` on
    (drawn from grid_seed when given: several samples on one grid).
    Per site, by chance: a "+" record (length from `lengths`) with its "-"
    partner at its end, a "+" record alone, a "-" record alone at site + 1, or
    nothing. On top of these
      n_long  "+" records about 5,000 bases long whose partner starts one past
              a far grid site that has no record of its own,
      n_cross "+" records ending one past the next-but-one site, on the "-"
              record that site would else own alone,
      n_share pairs of neighbouring "+" records with one end, and so one partner,
      off_grid * n_sites "+" and as many "-" records at random positions, half
              of the "+" ones with a partner.
    About a tenth of the coverages of either strand are 0. Starts are unique
    per strand and sorted; "-" records that would make two collapsed rows share
    a key are left out, so the data has no conflicts."""
    grid = np.random.default_rng(seed if grid_seed is None else grid_seed)  # samples of one grid share grid_seed
    rng = np.random.default_rng([seed, 1])
    n = n_sites - n_dup
    site = offset + 1000 + np.cumsum(grid.integers(2, max_gap, n))
    pos0 = np.sort(np.concatenate([site, grid.choice(site, n_dup, replace=False)]))
    r = rng.random(n)
    has_plus, partner, minus_alone = r < 0.7, r < 0.5, (r >= 0.7) & (r < 0.85)
    end = site + rng.choice(np.asarray(lengths), n)
    # the special records sit on sites 8 apart, so none touches another's neighbours
    special = 8 * rng.choice(max(n // 8 - 1, 1), n_long + n_cross + n_share, replace=False) + 1
    long_, cross, share = np.split(special, [n_long, n_long + n_cross])
    far = np.minimum(np.searchsorted(site, site[long_] + 5000), n - 1)
    reach = site[far] > site[long_] + 4000  # near the grid's end there is no far site: those ends lie past the grid
    end[long_] = np.where(reach, site[far] + 1, site[long_] + 5000 + rng.integers(0, 50, n_long))
    far = far[reach]
    has_plus[far], minus_alone[far] = False, False
    end[cross] = site[cross + 2] + 1
    has_plus[cross + 2], minus_alone[cross + 2] = False, True
    end[share] = end[share + 1]
    has_plus[special], partner[special] = True, True
    has_plus[share + 1], partner[share + 1] = True, True
    n_off = int(off_grid * n)
    lo, hi = int(site[0]), int(site[-1]) + 50
    off_p = rng.integers(lo, hi, n_off)
    off_e = off_p + rng.choice(np.asarray(lengths), n_off)
    ps = np.concatenate([site[has_plus], off_p])
    pe = np.concatenate([end[has_plus], off_e])
    ps, first = np.unique(ps, return_index=True)  # the first record with a start stays: the grid's own
    pe = pe[first]
    ms = np.unique(np.concatenate([end[has_plus & partner], site[minus_alone] + 1, off_e[: n_off // 2],
                                   rng.integers(lo, hi, n_off)]))
    ms = ms[np.isin(ms, pe) | ~np.isin(ms - 1, ps)]  # no unpaired "-" record one past a "+" start

    def reads(m):
        cov = rng.integers(1, 30, m).astype(np.float64)
        cov[rng.random(m) < 0.1] = 0.0
        pct = np.where(rng.random(m) < 0.5, rng.choice([0.0, 50.0, 100.0], m), np.round(rng.random(m) * 100.0, 2))
        return cov, pct

    pc, pp = reads(ps.size)
    mc, mp = reads(ms.size)
    return pos0, (ps, pe, pc, pp), (ms, mc, mp)


def situations(pos0, plus, minus) -> dict:
    """How often each situation a test wants occurs in its inputs (counts of
    records; a test asserts the ones it is about to be > 0)."""
    pos0 = np.asarray(pos0, np.int64)
    (ps, pe, pc, _), (ms, mc, _) = plus, minus
    on = np.isin(ps, pos0)
    j = np.minimum(np.searchsorted(ms, pe), max(ms.size - 1, 0))
    paired = ms[j] == pe if ms.size else np.zeros(ps.size, bool)
    cn = np.where(paired, mc[j], -1.0) if ms.size else np.full(ps.size, -1.0)
    matched = np.isin(ms, pe)
    owns_site = np.isin(ms - 1, pos0)
    ends, times = np.unique(pe[on & paired], return_counts=True)
    uniq, rows = np.unique(pos0, return_counts=True)
    return {
        "paired": int((on & paired).sum()),
        "plus_without_partner": int((on & ~paired).sum()),
        "minus_without_partner": int((~matched & owns_site).sum()),
        "matched_minus_on_a_bare_site": int((matched & owns_site & ~np.isin(ms - 1, ps)).sum()),
        "shared_partner": int((times > 1).sum()),
        "multi_base": int((on & (pe - ps > 1)).sum()),
        "long_paired": int((on & paired & (pe - ps > 4000)).sum()),
        "zero_plus_only": int((on & paired & (pc == 0) & (cn > 0)).sum()),
        "zero_minus_only": int((on & paired & (pc > 0) & (cn == 0)).sum()),
        "zero_both": int((on & paired & (pc == 0) & (cn == 0)).sum()),
        "off_grid_plus": int((~on).sum()),
        "off_grid_minus": int((~owns_site & ~matched).sum()),
        "duplicated_sites": int((rows > 1).sum()),
    }


def conflicted_sites(pos0, plus_start, plus_end, minus_start) -> np.ndarray:
    """bool [n_sites]: the grid rows two collapsed rows claim, before the
    total > 0 filter (their values are unspecified)."""
    ps, pe, ms = (np.asarray(a, np.int64) for a in (plus_start, plus_end, minus_start))
    key = np.concatenate([ps, ms[~np.isin(ms, pe)] - 1])
    uniq, count = np.unique(key, return_counts=True)
    return np.isin(np.asarray(pos0, np.int64), uniq[count > 1])
