"""Two-group chains that end in HYG_ENUMERIC, built from emission tables with
-inf entries (tests/test_gpu_tg_enumeric.py): the shapes, the poisoned patterns,
the chain list of the one mixed launch per shape and what the CPU oracle says
of every chain in it. Everything here is computed once per shape and shared,
read-only, by the tests that need it.

A launch's table is the clean table E [T][2K] followed by one copy of it per
chain that is not a clean one, with that chain's entries set to -inf; the
chain's site_begin points at its copy, the clean twins keep rows [0, T).
"""
import numpy as np

from tests import tg_trace_ref
from tests import test_gpu_tg_filter as flt
from tests import test_gpu_tg_global_w as gw

KEEP, OPTIMAL, UNBIASED = 0, 1, 2
NINF = float("-inf")

# name: the row the data comes from (flt.OWN, or gw.CASES), sites used, forced forward widths (0: automatic),
# the shape arguments of the kernel name per width, GW
SHAPES = {
    "generic": ("generic", 80, (64, 128, 256, 512, 768), "%d,0,0,0", False),
    "pipeline": ("c3", 80, (256, 512, 768), "%d,6,50,25", False),
    "pipeline_cov1000": ("c3_unbiased", 80, (256, 512, 768), "%d,6,50,25", False),
    "k12": ("c5", 60, (512, 768), "%d,12,50,25", False),
    "gw": (("gw", 0), 60, (0,), "256,0,0,0", True),
}
GAP = 3    # unowned output rows between two chains
LEAD = 2   # and before the first
TAIL = 5   # and behind the last

_PLANS = {}


def build_of(shape, width):
    fmt = SHAPES[shape][3]
    return fmt % width if "%d" in fmt else fmt


def poisoned(E, kind, arg):
    """E with the entries of one pattern set to -inf; (copy, first site with such an entry)."""
    K = E.shape[1] // 2
    P = E.copy()
    if kind == "all":          # every weight of site `arg`
        P[arg, :] = NINF
        return P, arg
    if kind == "ctrl":         # the control columns alone: every weight still
        P[arg, :K] = NINF
        return P, arg
    if kind == "conflict":     # regime 0 alone at `arg`, regime 1 alone at `arg` + 1, in both groups:
        #                        a particle must change regime below the minimum duration
        for t, r in ((arg, 0), (arg + 1, 1)):
            keep = P[t, [r, K + r]].copy()
            P[t, :] = NINF
            P[t, [r, K + r]] = keep
        return P, arg
    if kind == "stretch":      # regime 0 impossible in both groups over [a, b)
        a, b = arg
        P[a:b, 0] = NINF
        P[a:b, K] = NINF
        return P, a
    raise ValueError(kind)


def first_failure(oracle, p, E, seed, cid):
    """The first site whose weights are all -inf: n - 1 for the smallest n at
    which the chain over E[:n] has status -2 (binary search: the status is
    monotone in n); None for a chain that survives."""
    def status(n):
        st = oracle.chain(p, E[:n], seed, cid)["status"]
        assert st in (0, -2), st
        return st

    T = len(E)
    if status(T) == 0:
        return None
    lo, hi = 0, T  # (no sites: nothing failed yet)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if status(mid) == -2:
            hi = mid
        else:
            lo = mid
    return hi - 1


class Plan:
    """One shape's mixed launch. specs[i] = (kind, argument, identity) of chain
    i; chains[i] its (site_begin, n_sites, seed, chain id, out_begin) over
    E_all; a chain under model m is expected(i, m)."""

    def __init__(self, oracle, shape):
        case, T, widths, _, is_gw = SHAPES[shape]
        row = flt.OWN[case] if isinstance(case, str) else gw.CASES[case[1]]
        K, M, B, T_data, S, cov, dseed, seed, _ = row
        mu, sg, theta0, d, _ = gw._setup(oracle, K, M, B, T_data, S, cov, dseed)
        self.oracle, self.shape, self.K, self.M, self.B, self.T, self.is_gw = oracle, shape, K, M, B, T, is_gw
        self.mu, self.sg, self.max_reads = mu, sg, flt._maxr(d)
        rng = np.random.default_rng(900 + K)
        self.thetas = [theta0, theta0 + rng.normal(0.0, 0.7, theta0.shape)]
        self.params = [oracle.make_params(K=K, M=M, B=B, mu=mu, sigma=sg, theta=th) for th in self.thetas]
        E = oracle.emission(self.params[0], d["meth_control"][:T], d["tot_control"][:T], d["meth_case"][:T],
                            d["tot_case"][:T])  # (the models share mu and sigma: one table)
        assert np.isfinite(E).all()
        self.E = E
        self.idents = [(42, 1042), (43, 2042)]  # (seed, chain id) of the chains: A and B
        # the clean chain of every (identity, model)
        self.clean = {}
        for a, (sd, cid) in enumerate(self.idents):
            for m in range(2):
                self.clean[(a, m)] = self._frozen(oracle.chain(self.params[m], E, sd, cid, want_modes=True))
        modes = self.clean[(0, 0)]["modes"] // 65536
        self.modes = modes
        self.fixed = [0, 1, 2, 7, 8, 9, T - 2, T - 1]  # 7, 8, 9: around the first staged block of kEBlock = 8 rows
        self.keep_site = max(t for t in range(10, T - 2) if modes[t] == KEEP)
        self.optimal_site = min(t for t in range(30, T - 2) if modes[t] == OPTIMAL)
        unb = [int(t) for t in np.nonzero(modes == UNBIASED)[0]]
        self.unbiased_sites = [unb[0], unb[0] + 1] if unb else []
        half = T // 2
        self.stretch = (half - 10, half + 10)
        # clean twins first: under chain_model[i] = i % 2 they are (A, 0), (A, 1), (B, 0), (B, 1);
        # the patterns whose fate the oracle decides sit at even indices (model 0 in both kinds of launch)
        specs = [("clean", None, 0), ("clean", None, 0), ("clean", None, 1), ("clean", None, 1),
                 ("stretch", self.stretch, 0), ("ctrl", half, 0)]
        if K == 6:
            specs += [("conflict", half, 0), ("ctrl", half + 3, 1)]
        specs += [("all", s, j % 2) for j, s in enumerate(self.fixed)]
        specs += [("all", s, 0) for s in [self.keep_site, self.optimal_site] + self.unbiased_sites]
        self.specs = specs
        tables, self.tables, self.p0, chains = [E], {}, {}, []
        for i, (kind, arg, a) in enumerate(specs):
            s0 = 0
            if kind != "clean":
                P, self.p0[i] = poisoned(E, kind, arg)
                P.setflags(write=False)
                s0 = T * len(tables)
                tables.append(P)
                self.tables[i] = P
            sd, cid = self.idents[a]
            chains.append((s0, T, sd, cid, LEAD + i * (T + GAP)))
        self.chains = chains
        self.n_out = LEAD + len(chains) * (T + GAP) - GAP + TAIL
        self.E_all = np.ascontiguousarray(np.concatenate(tables))
        self.E_all.setflags(write=False)
        owned = np.zeros(self.n_out, bool)
        for c in chains:
            owned[c[4]:c[4] + T] = True
        self.unowned = np.nonzero(~owned)[0]
        self._expected = {}

    @staticmethod
    def _frozen(r):
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        return r

    def table(self, i):
        return self.tables.get(i, self.E)

    def twin(self, i, m):
        """The clean chain of chain i's identity under model m (one of the first four)."""
        return 2 * self.specs[i][2] + m

    def trace_rows(self, modes, extra=()):
        """The rows of a surviving chain compared with the oracle's prefix
        chains (one oracle chain per row): all at K = 3; else 0, 1, 2, T - 1,
        every tenth, `extra`, and an unbiased step with its successor."""
        T = self.T
        if self.K == 3:
            return list(range(T))
        R = {0, 1, 2, T - 1} | set(range(0, T, 10)) | set(extra)
        for t in np.nonzero(np.asarray(modes) == UNBIASED)[0]:
            R |= {int(t) - 1, int(t), int(t) + 1}
        return sorted(t for t in R if 0 <= t < T)

    def expected(self, i, m):
        """What the oracle says of chain i under model m. tstar: its failing
        site (None: it survives). A survivor: ref, its oracle chain, and (model
        0) rows, some rows of its trace. A failed chain: p0, its first poisoned
        site; log_z_before, the oracle's log Z over the sites before tstar;
        rows, the trace rows [p0, tstar) (None where there are none)."""
        if (i, m) in self._expected:
            return self._expected[(i, m)]
        o, p = self.oracle, self.params[m]
        kind, arg, a = self.specs[i]
        sd, cid = self.idents[a]
        P = self.table(i)
        if kind == "clean":
            e = dict(tstar=None, ref=self.clean[(a, m)], rows=None)
            if (a, m) == (0, 0):
                e["rows"] = tg_trace_ref.rows(p, P, self.trace_rows(self.modes), sd, cid)
        else:
            # every weight of site `arg` holds one of its -inf entries; the other patterns: the oracle decides
            tstar = arg if kind in ("all", "ctrl") else first_failure(o, p, P, sd, cid)
            if tstar is None:
                ref = self._frozen(o.chain(p, P, sd, cid, want_modes=True))
                assert ref["status"] == 0
                a0, b0 = arg if kind == "stretch" else (arg, arg + 2)
                rows = tg_trace_ref.rows(p, P, self.trace_rows(ref["modes"] // 65536,
                                                               (a0 - 1, a0, a0 + 1, b0 - 1, b0, b0 + 1)), sd, cid)
                e = dict(tstar=None, ref=ref, rows=rows)
            else:
                p0 = self.p0[i]
                assert p0 <= tstar
                before = o.chain(p, P[:tstar], sd, cid) if tstar > 0 else None
                assert before is None or before["status"] == 0
                e = dict(tstar=tstar, p0=p0, log_z_before=None if before is None else before["log_z"],
                         rows=tg_trace_ref.rows(p, P, range(p0, tstar), sd, cid) if tstar > p0 else None)
        for v in (e["rows"] or {}).values():
            v.setflags(write=False)
        self._expected[(i, m)] = e
        return e


def plan(oracle, shape):
    if shape not in _PLANS:
        _PLANS[shape] = Plan(oracle, shape)
    return _PLANS[shape]
