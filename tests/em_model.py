"""Numpy restatement of the transition statistics (hyg_tg_transition_stats) and
a sampler of legal paths (TEST INFRASTRUCTURE ONLY).

Written from the rule in include/hygeia_amd.h ("transition statistics") and
ExactModel.case_branch / log_trans (tests/tg_exact_model.py); shares no code
with hygeia_amd/em.py. Trajectories are by site, as tests/cp_model.py holds
them: merged [T][P], control / case [T][P][2] (d, r) int16; groups = [(site
begin, rows)]; a group's first row has no predecessor.
"""
from __future__ import annotations

import numpy as np


def classify(x, y, u: int):
    """One transition x -> y of states (m, d_c, r_c, d_k, r_k), m in {0, 1},
    durations already the unsigned 16-bit values: (cell of the 2 x 2 table or
    None, case duration of a hazard trial or None, whether the hazard fired)."""
    m, dc, _, dk, rk = x
    m2, dc2, rc2, dk2, _ = y
    cell = 2 * m + m2 if min(dc, dk) >= u else None
    if m2 == 1:                      # branch 1: the case state is the control's
        return cell, None, False
    if m == 1 and dc2 != 1:          # branch 2: a merged ancestor splits, the control continues: a forced change
        return cell, None, False
    if m == 0 and rc2 == rk:         # branch 3: the control moves onto the case regime: a forced change
        return cell, None, False
    return cell, dk, dk2 == 1        # branch 4: the hazard decides


def state(merged, control, case, t: int, p: int):
    u16 = lambda v: int(v) & 0xffff  # noqa: E731
    return (1 if merged[t, p] != 0 else 0, u16(control[t, p, 0]), int(control[t, p, 1]), u16(case[t, p, 0]),
            int(case[t, p, 1]))


def _row_states(merged, control, case, t: int):
    """state() for every trajectory of row t (plain Python ints)."""
    return list(zip((merged[t] != 0).astype(int).tolist(), (control[t, :, 0].astype(np.int64) & 0xffff).tolist(),
                    control[t, :, 1].tolist(), (case[t, :, 0].astype(np.int64) & 0xffff).tolist(),
                    case[t, :, 1].tolist()))


def transition_stats(merged, control, case, groups, minimum_duration: int, dcap: int):
    """(table [2][2], trials [dcap + 1], events [dcap + 1]) int64: a plain
    double loop over the rows that have a predecessor and the trajectories."""
    table = np.zeros((2, 2), dtype=np.int64)
    trials = np.zeros(dcap + 1, dtype=np.int64)
    events = np.zeros(dcap + 1, dtype=np.int64)
    for g0, n in groups:
        for t in range(g0 + 1, g0 + n):
            before, now = _row_states(merged, control, case, t - 1), _row_states(merged, control, case, t)
            for x, y in zip(before, now):
                cell, d, fired = classify(x, y, minimum_duration)
                if cell is not None:
                    table[cell // 2, cell % 2] += 1
                if d is not None:
                    j = min(d, dcap)
                    trials[j] += 1
                    if fired:
                        events[j] += 1
    return table, trials, events


def expected_stats(pair, u: int, dcap: int):
    """The same statistics in expectation under pairwise marginals: pair[t] =
    {(x, y): p(x_t, x_{t+1} | y)} (ExactModel.forward_backward), float64."""
    table, trials, events = np.zeros((2, 2)), np.zeros(dcap + 1), np.zeros(dcap + 1)
    for d in pair:
        for (x, y), pr in d.items():
            cell, dk, fired = classify(x, y, u)
            if cell is not None:
                table[cell // 2, cell % 2] += pr
            if dk is not None:
                trials[min(dk, dcap)] += pr
                if fired:
                    events[min(dk, dcap)] += pr
    return table, trials, events


def sample_paths(ex, T: int, P: int, seed: int):
    """P independent paths of T sites from ExactModel ex's prior: the initial
    law of a uniform phantom regime, then the transition law of
    ExactModel.log_trans, every trajectory advanced at once. Returns (merged
    [T][P], control, case [T][P][2]) int16 (durations below 2^15)."""
    rng = np.random.default_rng(seed)
    K, u = ex.K, ex.u
    D = min(T + 2, 512)  # the hazard is tabulated this far; a longer sojourn (never seen: rho >= 0.1 there) is refused

    def hazard(g, r, d):
        try:
            return ex.rho(g, r, d)
        except ValueError:  # log1p(-1): the float32 cdf is 1, where the model's rule gives 0.1
            return 0.1

    rho = np.array([[[hazard(g, r, d) for d in range(D)] for r in range(K)] for g in range(2)])
    Pm, Pc = np.exp(ex.lPm), np.exp(ex.lPc)  # [m][m'], [r][r'] (zero diagonal)

    def draw(probs):  # one index per row of a [P][n] probability matrix
        c = np.cumsum(probs, axis=1)
        return (rng.random(P)[:, None] * c[:, -1:] >= c).sum(axis=1).clip(0, probs.shape[1] - 1)

    def uniform_not(a, b):  # a regime outside {a, b}, uniformly
        ok = np.ones((P, K))
        ok[np.arange(P), a] = 0
        ok[np.arange(P), b] = 0
        return draw(ok)

    merged = np.zeros((T, P), dtype=np.int16)
    control, case = np.zeros((T, P, 2), dtype=np.int16), np.zeros((T, P, 2), dtype=np.int16)
    rc = draw(Pc[rng.integers(0, K, P)])
    m, dc, dk, rk = np.ones(P, dtype=np.int64), np.ones(P, dtype=np.int64), np.ones(P, dtype=np.int64), rc.copy()
    for t in range(T):
        if t > 0:
            assert max(dc.max(), dk.max()) < D
            free = np.minimum(dc, dk) >= u
            m2 = np.where(free, (rng.random(P) < Pm[m, 1]).astype(np.int64), m)
            c_change = rng.random(P) < rho[0, rc, dc]
            rc2 = np.where(c_change, draw(Pc[rc]), rc)
            dc2 = np.where(c_change, 1, dc + 1)
            b2 = (m2 == 0) & (m == 1) & (dc2 != 1)
            b3 = (m2 == 0) & (m == 0) & (rc2 == rk)
            b4 = (m2 == 0) & ~b2 & ~b3
            k_change = b2 | b3 | (b4 & (rng.random(P) < rho[1, rk, dk]))
            rk2 = np.where(m2 == 1, rc2, np.where(k_change, uniform_not(rc2, np.where(b2, rc2, rk)), rk))
            dk2 = np.where(m2 == 1, dc2, np.where(k_change, 1, dk + 1))
            m, dc, rc, dk, rk = m2, dc2, rc2, dk2, rk2
        merged[t] = m
        control[t, :, 0], control[t, :, 1] = dc, rc
        case[t, :, 0], case[t, :, 1] = dk, rk
    return merged, control, case
