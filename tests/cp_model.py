"""numpy restatement of the change-point pass (TEST INFRASTRUCTURE ONLY).

Written from the definitions, with loops over groups, windows and sites, not
from the kernels. For
one chromosome with sites t = 0 .. T-1 and P trajectories, in site order
(merged [T][P], control / case [T][P][2] = (d, r) int16) and groups = sorted,
disjoint (site_begin, n_rows):

  a group's first row and a site inside no group have no event of any kind;
  otherwise, against row t - 1 of the same trajectory, a state *continues* when
  r_t == r_{t-1} and uint16(d_t) == uint16(d_{t-1} + 1)
  kind 0 control : the control state does not continue
  kind 1 case    : the case state does not continue
  kind 2 any     : kind 0 or kind 1
  kind 3 split   : merged[t-1] != 0 and merged[t] == 0
  kind 4 merge   : merged[t-1] == 0 and merged[t] != 0

  c_t = sum_p E[t][p];  window [a, b): s_p = sum_t E[t][p], E_tot = sum_t c_t
  n_any = #{p : s_p >= 1}, n_one = #{p : s_p == 1}
  mode = the smallest t with c_t = max c;  C(t) = sum_{a <= u <= t} c_u
  tail = den - num;  lo = min{t : 2 den C(t) > tail E_tot}
  hi = max{t : 2 den (E_tot - C(t - 1)) > tail E_tot}
  E_tot = 0: mode = lo = a, hi = b - 1

and a generator of consistent sticky paths whose windows are neither empty nor
full (tests/test_cp_cpu.py pins its statistics).
"""
from __future__ import annotations

import numpy as np

from tests.dmr_model import GAP_PROBS, GAPS, find_regions, min_count  # noqa: F401  (windows are regions of a column)

KINDS = ("control", "case", "any", "split", "merge")


def continues(prev, cur) -> np.ndarray:
    """bool [...]: the (d, r) states cur [...][2] continue the states prev [...][2] of the row before."""
    d0 = prev[..., 0].astype(np.int64) & 0xffff
    d1 = cur[..., 0].astype(np.int64) & 0xffff
    return (cur[..., 1] == prev[..., 1]) & (d1 == ((d0 + 1) & 0xffff))


def event_matrix(merged, control, case, groups) -> np.ndarray:
    """E [5][T][P] bool. merged may be None: kinds 3 and 4 are then all False."""
    T, P = control.shape[:2]
    E = np.zeros((5, T, P), dtype=bool)
    for g0, n in groups:
        g0, g1 = int(g0), int(g0) + int(n)
        if g1 - g0 < 2:
            continue
        t = slice(g0 + 1, g1)  # the group's first row has no predecessor
        b = slice(g0, g1 - 1)  # the row before each of them
        E[0, t] = ~continues(control[b], control[t])
        E[1, t] = ~continues(case[b], case[t])
        E[2, t] = E[0, t] | E[1, t]
        if merged is not None:
            E[3, t] = (merged[b] != 0) & (merged[t] == 0)
            E[4, t] = (merged[b] == 0) & (merged[t] != 0)
    return E


def site_events(E) -> np.ndarray:
    """[T][5] int32, c_t of the five kinds."""
    return np.ascontiguousarray(E.sum(axis=2).T.astype(np.int32))


def window_counts(Ek, windows) -> np.ndarray:
    """[n][2] int32 (n_any, n_one) of one kind's E [T][P]."""
    out = np.zeros((len(windows), 2), dtype=np.int32)
    for i, (a, b) in enumerate(windows):
        s = np.zeros(Ek.shape[1], dtype=np.int64)
        for t in range(max(int(a), 0), min(int(b), Ek.shape[0])):
            s += Ek[t]
        out[i] = (int((s >= 1).sum()), int((s == 1).sum()))
    return out


def window_intervals(c, windows, num: int, den: int) -> np.ndarray:
    """[n][4] int64 (n_events, mode, lo, hi) of the column c [T]; Python integers throughout."""
    out = np.zeros((len(windows), 4), dtype=np.int64)
    tail = den - num
    for i, (a, b) in enumerate(windows):
        a, b = int(a), int(b)
        col = [int(c[t]) for t in range(a, b)]
        tot = sum(col)
        if tot == 0:
            out[i] = (0, a, a, b - 1)
            continue
        mode = a + col.index(max(col))
        lo = hi = None
        run = 0
        for j, v in enumerate(col):
            before = run  # C(t - 1)
            run += v      # C(t)
            if lo is None and 2 * den * run > tail * tot:
                lo = a + j
            if 2 * den * (tot - before) > tail * tot:
                hi = a + j
        out[i] = (tot, mode, lo, hi)
    return out


def segments(groups, windows):
    """The stretches of each group between consecutive windows, empty ones dropped: [n][2] int64."""
    out = []
    for g0, n in groups:
        g0, g1 = int(g0), int(g0) + int(n)
        u = g0
        for a, b in windows:
            a, b = int(a), int(b)
            if a < g0 or b > g1:
                continue
            if a > u:
                out.append((u, a))
            u = b
        if g1 > u:
            out.append((u, g1))
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def modal_regime(r_col, K: int) -> int:
    """1-based mode of the regimes r_col [P], ties to the lowest."""
    return int(np.argmax(np.bincount(np.asarray(r_col, dtype=np.int64), minlength=K))) + 1


def wrapped_continuations(st, Ek, windows) -> int:
    """Cells (t, p) inside the windows where the state st [T][P][2] continues
    (no event of Ek) across an int16 wrap: 32767 -> -32768 or -1 -> 0."""
    n = 0
    for a, b in windows:
        for t in range(max(int(a), 1), int(b)):
            d0, d1 = st[t - 1, :, 0], st[t, :, 0]
            wrap = ((d0 == 32767) & (d1 == -32768)) | ((d0 == -1) & (d1 == 0))
            n += int((wrap & ~Ek[t]).sum())
    return n


# the generator seeds of the (T, P) cases of tests/test_cp_cpu.py and tests/test_gpu_cp.py
STICKY_CASES = {(3000, 7): 4, (3000, 50): 0, (3000, 250): 0, (1200, 2400): 0}


def _truth_sites(T: int, rng, lo: int, mean: float):
    """Ascending sites from `lo`, at least 8 apart, geometric spacing."""
    out, t = [], lo
    while t < T - 8:
        out.append(t)
        t += 8 + int(rng.geometric(1.0 / mean))
    return out


def _placed(T: int, P: int, truth, rng, p_take=0.9, p_double=0.15, p_own=0.002):
    """[T][P] bool: each trajectory places a truth change with probability
    p_take at the truth site + U{-3..3}, with probability p_double a second one
    1 or 2 sites later, and changes of its own with probability p_own per site."""
    chg = rng.random((T, P)) < p_own
    for tau in truth:
        take = rng.random(P) < p_take
        at = np.clip(tau + rng.integers(-3, 4, P), 1, T - 1)
        chg[at[take], np.nonzero(take)[0]] = True
        dbl = take & (rng.random(P) < p_double)
        at2 = np.clip(at + rng.integers(1, 3, P), 1, T - 1)
        chg[at2[dbl], np.nonzero(dbl)[0]] = True
    chg[0] = False
    return chg


def sticky_paths(T: int, P: int, K: int, seed: int):
    """(merged [T][P], control [T][P][2], case [T][P][2], pos [T]) int16 / int64:
    consistent paths around shared truth sets of change sites (control changes
    from site 12 on about 40 sites apart, case changes about 50 apart, split /
    merge pairs 10 to 30 sites long about 45 apart). Durations count up from an
    event, regimes change at events; while merged the case state is the control
    state, a split gives the case group a regime of its own with d = 0, a merge
    gives it the control's (d + 1, r). Trajectories p % 5 == 1 start with d near
    32 760 and p % 5 == 3 near 65 530 (as int16), so both wraps occur in
    continuing stretches. positions = 10 000 + cumsum of CpG-like gaps."""
    rng = np.random.default_rng(seed)
    chg_c = _placed(T, P, _truth_sites(T, rng, 12, 40.0), rng)
    chg_k = _placed(T, P, _truth_sites(T, rng, 20, 50.0), rng)
    # merged: 1 until a split, 0 until the merge of the pair
    m = np.ones((T, P), dtype=np.int16)
    t = 30
    while t < T - 45:
        n = int(rng.integers(10, 31))
        take = rng.random(P) < 0.9
        s_at = np.clip(t + rng.integers(-3, 4, P), 1, T - 1)
        m_at = np.clip(t + n + rng.integers(-3, 4, P), 1, T - 1)
        for p in np.nonzero(take)[0]:
            m[s_at[p]:m_at[p], p] = 0
        t += n + 8 + int(rng.geometric(1.0 / 37.0))
    control = np.zeros((T, P, 2), dtype=np.int64)
    case = np.zeros((T, P, 2), dtype=np.int64)
    ar = np.arange(P)
    d = np.where(ar % 5 == 1, 32768 - rng.integers(4, 28, P), np.where(ar % 5 == 3, 65536 - rng.integers(4, 28, P),
                                                                      rng.integers(0, 500, P)))
    c = np.stack([d, rng.integers(0, K, P)], axis=1)
    k = c.copy()
    k[m[0] == 0, 1] = (k[m[0] == 0, 1] + 1) % K
    control[0], case[0] = c, k
    for t in range(1, T):
        c, k = c.copy(), k.copy()
        c[:, 0] += 1
        k[:, 0] += 1
        ev = chg_c[t]
        c[ev, 0] = 0
        c[ev, 1] = (c[ev, 1] + rng.integers(1, K, P)[ev]) % K
        mt, mb = m[t] != 0, m[t - 1] != 0
        ev = chg_k[t] & ~mt & ~mb  # the case group's own changes, while split
        k[ev, 0] = 0
        k[ev, 1] = (k[ev, 1] + rng.integers(1, K, P)[ev]) % K
        sp = mb & ~mt  # split: a regime of its own, d = 0
        k[sp, 0] = 0
        k[sp, 1] = (c[sp, 1] + rng.integers(1, K, P)[sp]) % K
        k[mt] = c[mt]  # merged (a merge included): the control's state
        control[t], case[t] = c, k
    pos = 10_000 + np.cumsum(rng.choice(GAPS, size=T, p=GAP_PROBS))
    to16 = lambda a: (a & 0xffff).astype(np.uint16).view(np.int16)  # noqa: E731
    return m, to16(control), to16(case), pos.astype(np.int64)
