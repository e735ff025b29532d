"""Reference rows of a traced forward-only launch (hyg_tg_trace_chains*), from
the CPU oracle as it stands: row t is what the chain of the first t + 1 sites
reports (oracle.chain on the prefix, same seed and chain id) -- its log Z, and
the filtering marginals as the contract of include/hygeia_amd.h defines them on
its final weights and states: exact integer sums of the 2^-100 images
fix100(det_exp(w - max w)) per class, one f64 division, rounded to f32.
"""
import numpy as np

from oracle import binding as ob
from oracle import tg_oracle_np as onp


def marginals(K, w, states):
    """(split_prob, regime_probs[2K]) f32 of one particle set."""
    w = np.asarray(w, np.float64)
    idx = np.nonzero(w > -np.inf)[0]
    if idx.size == 0:
        return np.float32(np.nan), np.full(2 * K, np.nan, np.float32)
    mx = float(w[idx].max())
    S, Sc = 0, [0] * (1 + 2 * K)
    for n in idx:
        m_n = onp.fix100(onp.det_exp(float(w[n]) - mx))
        if m_n == 0:
            continue
        m, _, rc, _, rk = ob.unpack(int(states[n]))
        S += m_n
        if m == 0:
            Sc[0] += m_n
        Sc[1 + rc] += m_n
        Sc[1 + K + rk] += m_n
    tot = onp.int_to_f64(S, 100)
    p = np.array([onp.int_to_f64(s, 100) / tot for s in Sc], np.float64).astype(np.float32)
    return p[0], p[1:]


def row(p, E, t, seed, chain_id):
    """Row t of the trace of the chain (seed, chain_id) over the emission rows E:
    (log_z_t, split_prob, regime_probs[2K])."""
    K = p.n_regimes
    r = ob.chain(p, np.ascontiguousarray(E[: t + 1]), seed, chain_id)
    if r["status"] != 0:
        return -np.inf, np.float32(np.nan), np.full(2 * K, np.nan, np.float32)
    sp, rp = marginals(K, r["final_log_weights"], r["final_states"])
    return r["log_z"], sp, rp


def rows(p, E, ts, seed, chain_id):
    """The rows `ts` (any iterable of site indices): dict of log_z_t [n] f64,
    split_probs [n] f32, regime_probs [n, 2K] f32, and `rows`, the sorted indices."""
    ts = sorted(set(int(t) for t in ts))
    K = p.n_regimes
    out = {"rows": np.array(ts, np.int64), "log_z_t": np.empty(len(ts)), "split_probs": np.empty(len(ts), np.float32),
           "regime_probs": np.empty((len(ts), 2 * K), np.float32)}
    for i, t in enumerate(ts):
        out["log_z_t"][i], out["split_probs"][i], out["regime_probs"][i] = row(p, E, t, seed, chain_id)
    return out


def row_set(modes, stride=5, every=False):
    """The rows a GPU test compares: 0, 1, 2 and T - 1, every step whose mode
    differs from its predecessor's and the step after it, every unbiased step
    (mode 2) and its successor, every stride-th row otherwise; all rows with
    `every`."""
    T = len(modes)
    if every:
        return list(range(T))
    R = {0, 1, 2, T - 1} | set(range(0, T, stride))
    for t in range(1, T):
        if modes[t] != modes[t - 1] or modes[t] == 2:
            R |= {t, t + 1}
    return sorted(t for t in R if 0 <= t < T)
