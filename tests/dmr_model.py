"""numpy restatement of the region (DMR) pass (TEST INFRASTRUCTURE ONLY).

Written from the definitions, with loops, not from the kernels. For one
chromosome with sites t = 0 .. T-1, positions pos[t] and P trajectories:

  D[t][p]  = (r_ctrl[t][p] != r_case[t][p]);  c_t = sum_p D[t][p]
  seed     : c_t >= min_count
  link     : seed sites t, t + 1 with 0 < pos[t + 1] - pos[t] <= max_gap
  region   : a maximal run [a, b) of linked seed sites with b - a >= min_sites,
             in ascending order of a
  s_p      = sum_{t in [a, b)} D[t][p]
  n_all    = #{p : s_p == n},  n_frac = #{p : s_p * den >= num * n}   (n = b - a)
  sums     = the column sums of a per-site count matrix over [a, b)

and a generator of sticky synthetic trajectories whose regions are neither all
empty nor all full (tests/test_dmr_cpu.py pins its statistics).
"""
from __future__ import annotations

import numpy as np


def find_regions(c, pos, min_count: int, max_gap: int, min_sites: int) -> np.ndarray:
    """[n][2] int64 (begin, end) of the candidate regions."""
    T = len(c)
    out = []
    t = 0
    while t < T:
        if int(c[t]) < min_count:
            t += 1
            continue
        a = t
        while t + 1 < T and int(c[t + 1]) >= min_count and 0 < int(pos[t + 1]) - int(pos[t]) <= max_gap:
            t += 1
        t += 1
        if t - a >= min_sites:
            out.append((a, t))
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def region_counts(D, regions, num: int, den: int) -> np.ndarray:
    """[n][2] int32 (n_all, n_frac); D [T][P] of 0 / 1."""
    P = D.shape[1]
    out = np.zeros((len(regions), 2), dtype=np.int32)
    for i, (a, b) in enumerate(regions):
        n = int(b) - int(a)
        n_all = n_frac = 0
        col = np.asarray(D[a:b], dtype=np.int64).sum(axis=0).tolist()  # s_p of every trajectory
        for p in range(P):
            s = col[p]
            n_all += 1 if s == n else 0
            n_frac += 1 if s * den >= num * n else 0
        out[i] = (n_all, n_frac)
    return out


def region_sums(counts, regions) -> np.ndarray:
    """[n][stride] int64 column sums of counts [T][stride] over each region."""
    out = np.zeros((len(regions), counts.shape[1]), dtype=np.int64)
    for i, (a, b) in enumerate(regions):
        for t in range(int(a), int(b)):
            out[i] += counts[t].astype(np.int64)
    return out


def min_count(site_prob: float, P: int) -> int:
    """The smallest integer c in [0, P + 1] with c / P >= site_prob in float64."""
    for c in range(P + 2):
        if c / P >= site_prob:
            return c
    return P + 1


# the generator seeds of the (T, P) cases of tests/test_dmr_cpu.py and tests/test_gpu_dmr.py
STICKY_CASES = {(3000, 7): 16, (3000, 50): 0, (3000, 250): 4, (1200, 2400): 14}

GAPS = np.array([2, 10, 40, 200, 900], dtype=np.int64)
GAP_PROBS = np.array([.3, .3, .2, .15, .05])


def sticky_trajectories(T: int, P: int, K: int, seed: int):
    """(r_ctrl [T][P], r_case [T][P], pos [T]): a shared truth track of
    differential stretches of geometric lengths (p = 0.08), each on with
    probability 0.45; each trajectory keeps its indicator with probability 0.95
    per site and otherwise follows the truth with probability 0.6 or a coin;
    r_case = (r_ctrl + U{1..K-1}) mod K where the indicator holds; positions =
    10 000 + cumsum of gaps from {2, 10, 40, 200, 900}."""
    rng = np.random.default_rng(seed)
    truth = np.zeros(T, dtype=bool)
    t = 0
    while t < T:
        n = int(rng.geometric(0.08))
        truth[t:t + n] = rng.random() < 0.45
        t += n
    keep = rng.random((T, P)) < 0.95
    follow = rng.random((T, P)) < 0.6
    coin = rng.random((T, P)) < 0.5
    D = np.zeros((T, P), dtype=bool)
    D[0] = np.where(follow[0], truth[0], coin[0])
    for t in range(1, T):
        D[t] = np.where(keep[t], D[t - 1], np.where(follow[t], truth[t], coin[t]))
    r_ctrl = rng.integers(0, K, (T, P))
    r_case = np.where(D, (r_ctrl + rng.integers(1, K, (T, P))) % K, r_ctrl)
    pos = 10_000 + np.cumsum(rng.choice(GAPS, size=T, p=GAP_PROBS))
    return r_ctrl.astype(np.int16), r_case.astype(np.int16), pos.astype(np.int64)


def site_counts(r_ctrl, r_case, K: int) -> np.ndarray:
    """hyg_dmp_site_counts' [T][2 + 2K] matrix with merged == 1 everywhere."""
    T = r_ctrl.shape[0]
    out = np.zeros((T, 2 + 2 * K), dtype=np.int32)
    out[:, 1] = (r_ctrl != r_case).sum(axis=1)
    for r in range(K):
        out[:, 2 + r] = (r_ctrl == r).sum(axis=1)
        out[:, 2 + K + r] = (r_case == r).sum(axis=1)
    return out
