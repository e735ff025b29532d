"""A sequential restatement of the forward recursion of the single-group SMC
(oracle/sg_oracle.c: sg_chain_core without the smoothing), which also keeps
what the C oracle throws away: log Z_t, the filtering marginals and the final
particle set. TEST INFRASTRUCTURE ONLY: the reference of hyg_sg_filter_chains /
hyg_sg_trace_chains (tests/test_gpu_sg_filter.py), tied to the C oracle bit for
bit in tests/test_sg_filter_cpu.py.

Built on the bit-exact helpers of oracle/tg_oracle_np.py (det_exp / det_log are
hyg_exp / hyg_log, det_fma an IEEE fma, fix100 / int_to_f64 the exact 2^-100
images, rand64 the Philox stream); hazard rows, exit flags, constants and the
emission table come from the C oracle (oracle.sg_binding). About a millisecond
per particle and step.

`exact_log_z` is an independent check of the recursion: the plain forward
recursion over every state (d, r) in floating point, the exact likelihood that
log Z equals while the particle set still enumerates every reachable state
(N_prev + K <= N_max at every step).
"""
from __future__ import annotations

import math

import numpy as np

from oracle import sg_binding as sg
from oracle.tg_oracle_np import det_exp, det_fma, det_log, fix100, int_to_f64, rand64

NINF = float("-inf")
RNG_SG_SYSTEMATIC = 5  # HYG_RNG_SG_SYSTEMATIC
HYG_OK, HYG_ENUMERIC = 0, -2


class Tables:
    """Hazard rows [K][n][2] (log rho, log(1 - rho)), exit flags and log P of a model."""

    def __init__(self, p, n_sites: int):
        c = sg.consts(p)
        self.K, self.u, self.Nmax, self.log_K = c.K, c.u, c.Nmax, c.log_K
        K = self.K
        self.logP = [[c.logP[r * K + q] for q in range(K)] for r in range(K)]
        n = n_sites + 2
        rows = [sg.hazard(p, r, n) for r in range(K)]
        self.hz = [[(float(h[d, 0]), float(h[d, 1])) for d in range(n)] for h, _, _ in rows]
        self.ex = [[int(e[d]) for d in range(n)] for _, e, _ in rows]

    def cont(self, d: int, r: int) -> float:  # sg_trans((d + 1, r) | (d, r))
        return self.hz[r][d - 1][1]

    def base(self, d: int, r: int) -> float:  # sg_bpart
        if d < self.u:
            return NINF
        return 0.0 if self.ex[r][d - 1] else self.hz[r][d - 1][0]


def lse(x):
    """exact log-sum-exp: max + log(sum fix100(exp(x - max)))"""
    mx = NINF
    for v in x:
        if v > mx:
            mx = v
    if not mx > NINF:
        return NINF
    s = 0
    for v in x:
        s += fix100(det_exp(v - mx))
    return mx + det_log(int_to_f64(s, 100))


def _sort_desc(v):
    """descending by value, ties by ascending index"""
    return sorted(range(len(v)), key=lambda i: (-v[i], i))


def _ceil_mul(T: float, R: int) -> int:
    if not T > 0.0:
        return 0
    num, den = T.as_integer_ratio()
    return -((-num * R) // den)


def forward(p, E, seed: int = 0, chain_id: int = 0, marginals: bool = True, tables: Tables = None):
    """The forward recursion over the T sites of E [T][K]. Returns a dict:
    status, t_stop (the first site whose weights are all -inf, else T),
    log_z_t [T], regime_probs [T][K], cp_probs [T] (NaN / -inf from t_stop on),
    nparts [T] (0 from t_stop on), and the final particle set: log_weights [N],
    states [N][2] as (d, r), log_z. After HYG_ENUMERIC the set is empty and
    log_z is -inf."""
    E = np.ascontiguousarray(E, np.float64)
    T = E.shape[0]
    tb = tables if tables is not None else Tables(p, T)
    K, Nmax = tb.K, tb.Nmax
    log_z_t = np.full(T, NINF)
    regime = np.full((T, K), np.nan)
    cp = np.full(T, np.nan)
    nparts = np.zeros(T, np.int32)

    def fail(t):
        return {"status": HYG_ENUMERIC, "t_stop": t, "log_z_t": log_z_t, "regime_probs": regime, "cp_probs": cp,
                "nparts": nparts, "log_weights": np.zeros(0), "states": np.zeros((0, 2), np.int32), "log_z": NINF}

    def record(t, d, r, lw, logZ):
        w = [det_exp(x - logZ) for x in lw]
        log_z_t[t] = logZ
        nparts[t] = len(lw)
        if marginals:
            im = [fix100(x) for x in w]
            for q in range(K):
                regime[t, q] = int_to_f64(sum(m for m, rr in zip(im, r) if rr == q), 100)
            cp[t] = int_to_f64(sum(m for m, dd in zip(im, d) if dd == 1), 100)
        return w

    # t = 0: N = K particles (1, r), log w = -log K + log g_0(r)
    d = [1] * K
    r = list(range(K))
    lw = [-tb.log_K + float(E[0, n]) for n in range(K)]
    logZ = lse(lw)
    if not logZ > NINF:
        return fail(0)
    w = record(0, d, r, lw, logZ)
    for t in range(1, T):
        Np, dP, rP, lwP, wP, logZp = len(lw), d, r, lw, w, logZ
        N = Nmax if Np + K > Nmax else Np + K
        M = N - K
        Et = [float(x) for x in E[t]]
        # resampleCp
        if N < Np + K:
            fin = sum(1 for x in lwP if math.isfinite(x))
            keep_top = True
            if fin > M:
                idx = _sort_desc(wP)
                logq = [det_log(wP[i]) for i in idx]
                cum = [0] * (Np + 1)
                for q in range(Np - 1, -1, -1):
                    cum[q] = cum[q + 1] + fix100(wP[idx[q]])
                kOld, kNew, logC = 1, 0, 0.0
                while kNew != kOld:
                    kOld = kNew
                    logC = det_log(float(M - kOld)) - det_log(int_to_f64(cum[kOld], 100))
                    kNew = kOld + sum(1 for q in range(kOld, Np) if logq[q] > -logC)
                if math.isfinite(logC):
                    keep_top = False
                    Kk, L = kNew, M - kNew
                    anc = [idx[q] for q in range(Kk)]
                    lwres = [lwP[idx[q]] for q in range(Kk)]
                    if L > 0:
                        rmax = max(logq[Kk:Np])
                        run, cumr = 0, {}
                        for q in range(Kk, Np):
                            run += fix100(det_exp(logq[q] - rmax))
                            cumr[q] = run
                        uu = float(rand64(seed, chain_id, RNG_SG_SYSTEMATIC, t, 0) >> 11) * 1.1102230246251565404e-16
                        i = Kk
                        for j in range(L):
                            thr = _ceil_mul((float(j) + uu) / float(L), run)
                            while i < Np - 1 and cumr[i] < thr:
                                i += 1
                            anc.append(idx[i])
                            lwres.append(logZp - logC)
            if keep_top:
                idx = _sort_desc(lwP)
                anc = idx[:M]
                lwres = [lwP[i] for i in anc]
        else:
            anc = list(range(M))
            lwres = list(lwP[:M])
        # continuing particles (d + 1, r)
        d = [dP[a] + 1 for a in anc]
        r = [rP[a] for a in anc]
        lw = [lwres[n] + (tb.cont(dP[a], rP[a]) + Et[rP[a]]) for n, a in enumerate(anc)]
        # fresh particles (1, q), factorised over the regimes as the oracle
        A = [NINF] * K
        a_n = [lwP[n] + tb.base(dP[n], rP[n]) for n in range(Np)]
        for n in range(Np):
            if a_n[n] > A[rP[n]]:
                A[rP[n]] = a_n[n]
        Er = [0] * K
        for n in range(Np):
            if a_n[n] > NINF:
                Er[rP[n]] += fix100(det_exp(a_n[n] - A[rP[n]]))
        Ef = [int_to_f64(x, 100) for x in Er]
        for q in range(K):
            mq = NINF
            for rr in range(K):
                v = A[rr] + tb.logP[rr][q]
                if v > mq:
                    mq = v
            d.append(1)
            r.append(q)
            if mq > NINF:
                S = 0.0
                for rr in range(K):
                    S = det_fma(det_exp((A[rr] + tb.logP[rr][q]) - mq), Ef[rr], S)
                lw.append((mq + det_log(S)) + Et[q])
            else:
                lw.append(NINF)
        logZ = lse(lw)
        if not logZ > NINF:
            return fail(t)
        w = record(t, d, r, lw, logZ)
    return {"status": HYG_OK, "t_stop": T, "log_z_t": log_z_t, "regime_probs": regime, "cp_probs": cp,
            "nparts": nparts, "log_weights": np.array(lw, np.float64),
            "states": np.array(list(zip(d, r)), np.int32).reshape(-1, 2), "log_z": logZ}


def _logsumexp(a) -> float:
    a = np.asarray(a, np.float64)
    m = float(a.max())
    if not math.isfinite(m):
        return m
    return m + math.log(float(np.exp(a - m).sum()))


def exact_log_z(p, E) -> float:
    """log p(y_0..T-1) by the plain forward recursion over every state (d, r),
    d <= T, with the model's hazard tables (numpy, libm)."""
    E = np.asarray(E, np.float64)
    T = E.shape[0]
    tb = Tables(p, T)
    K = tb.K
    logP = np.array(tb.logP)
    cont = np.array([[tb.cont(dd, r) for r in range(K)] for dd in range(1, T + 1)])
    base = np.array([[tb.base(dd, r) for r in range(K)] for dd in range(1, T + 1)])
    la = np.full((T + 1, K), NINF)  # la[d - 1][r]
    la[0] = -tb.log_K + E[0]
    for t in range(1, T):
        new = np.full((T + 1, K), NINF)
        new[1:t + 1] = la[:t] + cont[:t] + E[t]
        out = la[:t] + base[:t]  # [d][r]: mass leaving (d, r)
        for q in range(K):
            with np.errstate(invalid="ignore"):
                new[0, q] = _logsumexp((out + logP[:, q]).ravel()) + E[t, q]
        la = new
    return _logsumexp(la.ravel())
