"""The reference of the single-group backward simulation
(hyg_sg_history_chains_multi, hyg_sg_sample_paths_multi). TEST INFRASTRUCTURE
ONLY, numpy and Python integers.

`history` restates the forward recursion of tests/sg_filter_ref.py in one pass
and keeps the particle set of every site (tests/test_sg_sample_cpu.py ties it
to `forward`'s final set and log Z_t on every prefix); `sample` is the path
rule of DESIGN.md section 3; `exact_marginals` is a plain forward-backward over
(d, r) in numpy, the exact smoothing marginals that the draws follow while the
sets enumerate every reachable state.
"""
from __future__ import annotations

import bisect
import math

import numpy as np

from oracle.tg_oracle_np import det_exp, det_fma, det_log, fix100, int_to_f64, rand64
from tests.sg_filter_ref import (HYG_ENUMERIC, HYG_OK, NINF, RNG_SG_SYSTEMATIC, Tables, _ceil_mul, _sort_desc, lse)

RNG_SG_SAMPLE = 6  # the Philox stream of the backward draws
U53 = 1.1102230246251565404e-16


def case_moments(K: int):
    """mu and sigma of the test models: the three regimes of the exactness cases, the binding's defaults beyond."""
    if K <= 3:
        return [0.7, 0.3, 0.5][:K], [0.15, 0.15, 0.25][:K]
    mu = [(i + 0.5) / K for i in range(K)]
    return mu, [0.05 + 0.2 * min(m, 1 - m) for m in mu]


def synthetic_case(K: int, u: int, Nmax: int, T: int, seed: int = 11):
    """The data of the tests: one sample, 0 .. 4 reads per site, the level
    constant over blocks of eight sites. Returns (params, meth, tot, E)."""
    from oracle import sg_binding as sg

    rng = np.random.default_rng(seed)
    mu, sigma = case_moments(K)
    tot = rng.integers(0, 5, (T, 1))
    lev = np.repeat(rng.choice(mu, (T + 7) // 8), 8)[:T]
    meth = rng.binomial(tot, lev[:, None])
    p = sg.make_params(K=K, mu=mu, sigma=sigma, u=u, Nmax=Nmax)
    meth, tot = np.ascontiguousarray(meth, np.uint16), np.ascontiguousarray(tot, np.uint16)
    return p, meth, tot, sg.emission(p, meth, tot)


def history(p, E, seed: int = 0, chain_id: int = 0, tables: Tables = None):
    """The forward recursion over E [T][K], every step's set kept. Returns a
    dict: status, t_stop, log_z, log_z_t [T], and `sets`, a list of T entries
    (lw [N] floats, states [N] of (d, r)); from t_stop on the entries are empty."""
    E = np.ascontiguousarray(E, np.float64)
    T = E.shape[0]
    tb = tables if tables is not None else Tables(p, T)
    K, Nmax = tb.K, tb.Nmax
    sets = [([], []) for _ in range(T)]
    log_z_t = np.full(T, NINF)

    def out(status, t_stop, logZ):
        return {"status": status, "t_stop": t_stop, "log_z": logZ, "log_z_t": log_z_t, "sets": sets}

    d = [1] * K
    r = list(range(K))
    lw = [-tb.log_K + float(E[0, n]) for n in range(K)]
    logZ = lse(lw)
    if not logZ > NINF:
        return out(HYG_ENUMERIC, 0, NINF)
    sets[0] = (list(lw), list(zip(d, r)))
    log_z_t[0] = logZ
    w = [det_exp(x - logZ) for x in lw]
    for t in range(1, T):
        Np, dP, rP, lwP, wP, logZp = len(lw), d, r, lw, w, logZ
        N = Nmax if Np + K > Nmax else Np + K
        M = N - K
        Et = [float(x) for x in E[t]]
        if N < Np + K:  # resampleCp
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
                        uu = float(rand64(seed, chain_id, RNG_SG_SYSTEMATIC, t, 0) >> 11) * U53
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
        d = [dP[a] + 1 for a in anc]
        r = [rP[a] for a in anc]
        lw = [lwres[n] + (tb.cont(dP[a], rP[a]) + Et[rP[a]]) for n, a in enumerate(anc)]
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
            return out(HYG_ENUMERIC, t, NINF)
        sets[t] = (list(lw), list(zip(d, r)))
        log_z_t[t] = logZ
        w = [det_exp(x - logZ) for x in lw]
    return out(HYG_OK, T, logZ)


def history_arrays(h, Nmax: int):
    """The three history arrays of a chain as the launch lays them out: entries
    n >= N keep the fill values (NaN, 0xffffffff), which the launch never writes."""
    T = len(h["sets"])
    lw = np.full((T, Nmax), np.nan)
    st = np.full((T, Nmax), 0xFFFFFFFF, np.uint32)
    npart = np.zeros(T, np.int32)
    for t, (l, s) in enumerate(h["sets"]):
        N = len(l)
        npart[t] = N
        lw[t, :N] = l
        st[t, :N] = [d | (r << 24) for d, r in s]
    return lw, st, npart


def _i16(x: int) -> int:
    v = x & 0xFFFF
    return v - 0x10000 if v & 0x8000 else v


def cumulative(logits):
    """C_n of a draw with these logits (exact integers), or None without a finite logit."""
    m = NINF
    for v in logits:
        if v > m:
            m = v
    if not (m > NINF and m < math.inf):
        return None
    c, out = 0, []
    for v in logits:
        c += fix100(det_exp(v - m)) if v > NINF else 0
        out.append(c)
    return out


def draw(cum, seed: int, chain_id: int, s: int, b: int) -> int:
    """n* of the draw of trajectory b from the set of site s with cumulative sums cum."""
    uu = float(rand64(seed, chain_id, RNG_SG_SAMPLE, s, b) >> 11) * U53
    thr = max(1, _ceil_mul(uu, cum[-1]))
    return bisect.bisect_left(cum, thr)  # the smallest n with C_n >= thr


def sample(sets, tables: Tables, T: int, B: int, seed: int, chain_id: int):
    """B trajectories from the sets of a history (`history(...)["sets"]` or
    hand-made ones: a list of (lw, [(d, r)])). Returns paths int16 [T][B][2] =
    (d mod 2^16 as int16, r) and the sample status; a trajectory that meets no
    finite logit, a d > t + 1 or an r >= K is -1 from there down. The sums of a
    draw depend on (site, regime entered) only and are formed once."""
    paths = np.full((T, B, 2), -1, np.int16)
    status = HYG_OK
    K = tables.K
    cums = {}

    def cum_of(t, r_to):
        if (t, r_to) not in cums:
            lw, st = sets[t]
            if r_to < 0:
                logits = list(lw)
            else:
                logits = [(lw[n] + tables.base(dn, rn)) + tables.logP[rn][r_to] if dn >= 1 and rn < K else NINF
                          for n, (dn, rn) in enumerate(st)]
            cums[t, r_to] = cumulative([NINF if v != v else v for v in logits])
        return cums[t, r_to]

    for b in range(B):
        t, r_to = T - 1, -1
        while t >= 0:
            cum = cum_of(t, r_to)
            ok = cum is not None
            if ok:
                d, r = sets[t][1][draw(cum, seed, chain_id, t, b)]
                ok = 1 <= d <= t + 1 and r < K
            if not ok:
                status = HYG_ENUMERIC
                break  # rows 0 .. t stay -1
            paths[t - d + 1:t + 1, b, 0] = [_i16(d - k) for k in range(d - 1, -1, -1)]
            paths[t - d + 1:t + 1, b, 1] = r
            r_to = r
            t -= d
    return paths, status


def exact_marginals(tb: Tables, E):
    """Exact smoothing marginals of the change-point model by forward-backward
    over every state (d <= T, r) in numpy (libm), with the model's hazard
    tables: regime [T][K] = P(r_t = r | y), start [T] = P(d_t = 1 | y)."""
    E = np.asarray(E, np.float64)
    T, K = E.shape[0], tb.K
    logP = np.array(tb.logP)
    cont = np.array([[tb.cont(dd, r) for r in range(K)] for dd in range(1, T + 1)])  # [d - 1][r]
    base = np.array([[tb.base(dd, r) for r in range(K)] for dd in range(1, T + 1)])

    def lse_all(a):
        a = np.asarray(a, np.float64).ravel()
        m = float(a.max())
        return m if not math.isfinite(m) else m + math.log(float(np.exp(a - m).sum()))

    with np.errstate(invalid="ignore", divide="ignore"):
        al = np.full((T, T, K), NINF)  # alpha[t][d - 1][r]
        al[0, 0] = -tb.log_K + E[0]
        for t in range(1, T):
            al[t, 1:t + 1] = al[t - 1, :t] + cont[:t] + E[t]
            outm = al[t - 1, :t] + base[:t]  # [d][r]
            for q in range(K):
                al[t, 0, q] = lse_all((outm + logP[:, q]).ravel()) + E[t, q]
        be = np.full((T, T, K), NINF)  # beta[t][d - 1][r] = log p(y_{t+1..} | state)
        be[T - 1, :T] = 0.0
        for t in range(T - 2, -1, -1):
            fresh = np.array([lse_all(logP[r] + E[t + 1] + be[t + 1, 0]) for r in range(K)])  # [r]
            stay = cont[:t + 1] + E[t + 1] + be[t + 1, 1:t + 2]
            go = base[:t + 1] + fresh[None, :]
            be[t, :t + 1] = np.logaddexp(stay, go)
        logZ = lse_all(al[T - 1].ravel())
        post = np.exp(al + be - logZ)
    post = np.nan_to_num(post)
    return post.sum(axis=1), post[:, 0, :].sum(axis=1)
