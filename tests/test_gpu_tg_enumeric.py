"""Two-group chains whose particle weights all become -inf (HYG_ENUMERIC), on
the GPU: the contract of include/hygeia_amd.h for a failed chain in full,
forward-only and traced launches, and for the chains that share its launch.

Counts cannot produce such a chain (the Beta-Binomial log-pmf is finite), but
the device entries take the emission table as a pointer: a chain fails where a
row of its table holds -inf (tests/tg_enumeric.py). The CPU oracle runs on the
same table, so everything is compared bit for bit. Per shape and forced width
one launch holds every poisoned chain, clean twins (same seed and chain id over
the clean rows) and a chain that survives a poisoned stretch, with gaps of
unowned output rows between them; the outputs are filled with a byte pattern
before every launch. For a chain that fails at site t*:

1. status HYG_ENUMERIC, log Z -inf, all N_max final weights -inf, the same
   bytes in the full, the forward-only and the traced launch;
2. traced: rows before t* are the clean twin's (before the first poisoned
   site) or the oracle's prefix chains' (from there on); row t* - 1 of log_z_t
   is the oracle's log Z over the sites before t*;
3. traced: rows from t* on hold -inf and NaN, with the probabilities and
   without (trace="log_z");
4. full: none of its rows is written;
5. every other chain equals the oracle and the launch without the failing chains.

The CPU part (no GPU) checks on the oracle that every pattern reaches what it
is here for.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import tg_enumeric as en  # noqa: E402

HYG_ENUMERIC = -2
PATTERN = 0xA5  # the byte every output holds before a launch
ROWS = ("merged", "control", "case", "split_probs", "regime_probs")
CHAIN = ("log_z", "final_w", "status")
TRACE = ("log_z_t", "split_probs", "regime_probs")
KINDS = ("full", "filter", "trace_all", "trace_log_z")


# --------------------------------------------------------------- the CPU part
@pytest.mark.parametrize("shape", list(en.SHAPES))
def test_patterns_on_the_oracle(oracle, shape):
    """Every pattern's status and failing site on the CPU oracle (by the binary
    search over prefixes, also where the site is known by construction), the
    status on either side of it, and the kinds of step the sites were chosen for."""
    pl = en.plan(oracle, shape)
    K, T, p = pl.K, pl.T, pl.params[0]
    for r in pl.clean.values():
        assert r["status"] == 0
    m = pl.modes
    assert m[pl.keep_site] == en.KEEP and m[pl.optimal_site] == en.OPTIMAL and pl.keep_site != pl.optimal_site
    u = pl.unbiased_sites  # the first unbiased step's site and the site after it, wherever the clean chain has one
    assert shape != "pipeline_cov1000" or len(u) == 2
    assert not u or (m[u[0]] == en.UNBIASED and m[u[1]] != en.UNBIASED and u[1] == u[0] + 1)
    sites = {arg for kind, arg, _ in pl.specs if kind == "all"}
    assert sites >= {0, 1, 2, 7, 8, 9, T - 2, T - 1, pl.keep_site, pl.optimal_site} | set(pl.unbiased_sites)
    kinds = [s[0] for s in pl.specs]
    assert kinds.count("clean") == 4 and kinds.count("stretch") == 1 and kinds.count("ctrl") >= 1
    assert ("conflict" in kinds) == (K == 6)
    for i, (kind, arg, a) in enumerate(pl.specs):
        if kind == "clean":
            continue
        sd, cid = pl.idents[a]
        P = pl.table(i)
        e = pl.expected(i, 0)
        tstar = e["tstar"]
        if kind in ("all", "ctrl"):  # by construction; the whole chain and the prefixes around t* below
            assert tstar == arg and oracle.chain(p, P, sd, cid)["status"] == HYG_ENUMERIC
        else:
            assert tstar == en.first_failure(oracle, p, P, sd, cid)
        if kind == "stretch":
            assert tstar is None
            lo, hi = arg  # the chain survives, and no draw has regime 0 there
            assert (e["ref"]["control"][lo:hi, :, 1] != 0).all() and (e["ref"]["case"][lo:hi, :, 1] != 0).all()
        if kind == "conflict":
            # K = 6, coverage 100: the particles die out one site after the sparse one; at coverage 1 000 they survive
            assert tstar == {"pipeline": arg + 1, "pipeline_cov1000": None}[shape]
        print(f"{shape}: chain {i} {kind} {arg}: t* = {tstar}")
        if tstar is not None:  # monotone around t*
            assert oracle.chain(p, P[:tstar + 1], sd, cid)["status"] == HYG_ENUMERIC
            assert tstar == 0 or oracle.chain(p, P[:tstar], sd, cid)["status"] == 0
    # under chain_model[i] = i % 2 the second model runs only clean chains and chains that fail by construction
    for i, (kind, arg, a) in enumerate(pl.specs):
        assert i % 2 == 0 or kind in ("clean", "all", "ctrl")


# --------------------------------------------------------------- the launches
def _need_gpu():
    from hygeia_amd import _lib

    L = _lib.load()
    if L.hyg_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")
    return L


def _names(L, models, n, multi):
    """The forward kernels of the full, the forward-only and the traced launch of n chains."""
    out = []
    for fn, args in (("hyg_tg_kernel_name", (0,)), ("hyg_tg_filter_kernel_name", ()), ("hyg_tg_trace_kernel_name", ())):
        buf = C.create_string_buffer(128)
        if multi:
            h = (C.c_void_p * len(models))(*[m.handle for m in models])
            assert getattr(L, fn + "_multi")(h, len(models), n, *args, buf, 128) > 1
        else:
            assert getattr(L, fn)(models[0].handle, n, *args, buf, 128) > 1
        out.append(buf.value.decode())
    return out


def _assert_names(L, pl, models, n, width, multi):
    b, g = en.build_of(pl.shape, width), "true" if pl.is_gw else "false"
    mm = "true" if multi else "false"
    want = ["tg_forward_kernel<%s,false,%s%s>" % (b, g, ",true" if multi else ""),
            "tg_forward_kernel<%s,false,%s,%s,false>" % (b, g, mm),
            "tg_forward_kernel<%s,false,%s,%s,false,true>" % (b, g, mm)]
    assert _names(L, models, n, multi) == want


def _models(pl, n):
    from hygeia_amd import two_group

    return [two_group.CaseControlModel(pl.mu, pl.sg, th, num_resampled_ancestors=pl.M, num_samples_backward=pl.B,
                                       max_total_reads=pl.max_reads, max_duration=pl.T + 5) for th in pl.thetas[:n]]


def _fill(*tensors):
    for a in tensors:
        a.view(torch.uint8).fill_(PATTERN)


class Launches:
    """The four launches of one chain list over one table: a DeviceChains, a
    DeviceFilter, a DeviceFilter(trace="all") and one with trace="log_z", kept
    so that a test can run them again on the same workspaces."""

    def __init__(self, model, chains, n_out, chain_model=None):
        from hygeia_amd import two_group

        dev = torch.device("cuda", 0)
        kw = dict(device=dev, final_weights=True, chain_model=chain_model)
        self.obj = {"full": two_group.DeviceChains(model, chains, n_out, **kw),
                    "filter": two_group.DeviceFilter(model, chains, **kw),
                    "trace_all": two_group.DeviceFilter(model, chains, trace="all", n_out_rows=n_out, **kw),
                    "trace_log_z": two_group.DeviceFilter(model, chains, trace="log_z", n_out_rows=n_out, **kw)}
        self.dev = dev

    def run(self, kind, E):
        """One launch over the device table E, every output holding the pattern before it; host arrays."""
        o = self.obj[kind]
        keys = CHAIN + (ROWS if kind == "full" else TRACE if kind == "trace_all" else
                        ("log_z_t",) if kind == "trace_log_z" else ())
        _fill(*[getattr(o, k) for k in keys])
        o.run(E)
        torch.cuda.synchronize()
        return {k: getattr(o, k).cpu().numpy() for k in keys}

    def run_all(self, E):
        return {kind: self.run(kind, E) for kind in KINDS}


def _device_table(E):
    return torch.tensor(np.asarray(E), dtype=torch.float64, device=torch.device("cuda", 0))


def _untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == PATTERN).all())


def _same_bytes(a, b, what):
    assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), what


def _check(pl, got, model_of, what):
    """Points 1 to 5 (but the launch without the failing chains) on the host
    arrays of the four launches; model_of[i] is the model of chain i."""
    T, full, tra, trz = pl.T, got["full"], got["trace_all"], got["trace_log_z"]
    for kind in KINDS[1:]:  # the three kinds of launch agree byte for byte
        for k in CHAIN:
            _same_bytes(got[kind][k], full[k], (what, kind, k))
    _same_bytes(trz["log_z_t"], tra["log_z_t"], (what, "log Z_t alone"))
    for arrays, keys in ((full, ROWS), (tra, TRACE)):  # rows no chain owns
        for k in keys:
            assert _untouched(arrays[k][pl.unowned]), (what, "unowned rows", k)
    n_failed = 0
    for i, (s0, n, sd, cid, o0) in enumerate(pl.chains):
        m = model_of[i]
        e = pl.expected(i, m)
        w = (what, "chain %d %s" % (i, pl.specs[i][:2]), "model %d" % m)
        if e["tstar"] is None:  # 5: the oracle's chain
            ref = e["ref"]
            assert full["status"][i] == 0, w
            for k in ROWS:
                np.testing.assert_array_equal(full[k][o0:o0 + T], ref[k], err_msg=str(w + (k,)))
            assert full["log_z"][i] == ref["log_z"] == tra["log_z_t"][o0 + T - 1], w
            np.testing.assert_array_equal(full["final_w"][i], ref["final_log_weights"], err_msg=str(w))
            for k in TRACE:
                assert not np.isnan(tra[k][o0:o0 + T]).any(), w + (k,)
            if e["rows"] is not None:
                R = e["rows"]["rows"]
                for k in TRACE:
                    np.testing.assert_array_equal(tra[k][o0:o0 + T][R], e["rows"][k], err_msg=str(w + (k,)))
            continue
        n_failed += 1
        ts, p0 = e["tstar"], e["p0"]
        # 1
        assert full["status"][i] == HYG_ENUMERIC, w
        assert full["log_z"][i] == -np.inf, w
        assert full["final_w"][i].shape == (pl.M * (2 * pl.K + pl.K * pl.K),) and (full["final_w"][i] == -np.inf).all(), w
        # 4
        for k in ROWS:
            assert _untouched(full[k][o0:o0 + T]), w + (k, "written")
        # 2
        t0 = pl.chains[pl.twin(i, m)][4]
        for k in TRACE:
            _same_bytes(tra[k][o0:o0 + p0], tra[k][t0:t0 + p0], w + (k, "rows before the poisoned site"))
            if e["rows"] is not None:
                np.testing.assert_array_equal(tra[k][o0 + p0:o0 + ts], e["rows"][k], err_msg=str(w + (k,)))
        if ts > 0:
            assert tra["log_z_t"][o0 + ts - 1] == e["log_z_before"], w
        # 3
        assert (tra["log_z_t"][o0 + ts:o0 + T] == -np.inf).all(), w
        assert np.isnan(tra["split_probs"][o0 + ts:o0 + T]).all() and np.isnan(tra["regime_probs"][o0 + ts:o0 + T]).all(), w
    return n_failed


def _survivors(pl):
    return [i for i in range(len(pl.chains)) if pl.expected(i, 0)["tstar"] is None]


CASES = [(s, w) for s in en.SHAPES for w in en.SHAPES[s][2]]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,width", CASES, ids=["%s-%d" % c for c in CASES])
def test_mixed_launch(oracle, shape, width):
    """One launch of every kind over all poisoned chains and their clean
    twins; then the full and the traced launch of the surviving chains alone,
    whose rows and per-chain values the mixed launch leaves as they are."""
    from hygeia_amd import _lib

    L = _need_gpu()
    pl = en.plan(oracle, shape)
    n = len(pl.chains)
    models = _models(pl, 1)
    try:
        assert models[0].global_weights == pl.is_gw
        _lib.check(L.hyg_tg_force_threads(width, 0))
        _assert_names(L, pl, models, n, width, False)
        E = _device_table(pl.E_all)
        got = Launches(models[0], pl.chains, pl.n_out).run_all(E)
        n_failed = _check(pl, got, [0] * n, f"{shape} width {width}")
        keep = _survivors(pl)
        assert n_failed == n - len(keep) >= 11 and len(keep) >= 5
        _assert_names(L, pl, models, len(keep), width, False)
        alone = Launches(models[0], [pl.chains[i] for i in keep], pl.n_out)
        for kind, keys in (("full", ROWS), ("trace_all", TRACE)):
            r = alone.run(kind, E)
            for j, i in enumerate(keep):
                o0 = pl.chains[i][4]
                for k in keys:
                    _same_bytes(got[kind][k][o0:o0 + pl.T], r[k][o0:o0 + pl.T], (shape, width, kind, i, k))
                for k in CHAIN:
                    _same_bytes(got[kind][k][i], r[k][j], (shape, width, kind, i, k))
    finally:
        L.hyg_tg_force_threads(0, 0)
        for m in models:
            m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(en.SHAPES))
def test_multi_model_and_tail_overlap(oracle, shape):
    """The mixed launch through the multi-model entries, two models
    alternating over the chains (failing chains under both), each chain
    against the oracle under its own theta; the full launch with the tail
    overlap on and off (K = 12: on a pretended 6-CU device, where the launch
    splits into the full rounds and the rest)."""
    from hygeia_amd import _lib

    L = _need_gpu()
    pl = en.plan(oracle, shape)
    n = len(pl.chains)
    order = [i % 2 for i in range(n)]
    models = _models(pl, 2)
    try:
        # on the CPU first: the models matter, and chains fail under both
        assert pl.clean[(0, 0)]["log_z"] != pl.clean[(0, 1)]["log_z"]
        failing = [order[i] for i in range(n) if pl.expected(i, order[i])["tstar"] is not None]
        assert failing.count(0) >= 5 and failing.count(1) >= 5
        if shape == "k12":
            _lib.check(L.hyg_tg_set_device_cus(0, 6))
            assert L.hyg_tg_chains_per_cu(models[0].handle, n) == 1 and n > 6 and n % 6 != 0  # the split applies
        width = {"k12": 512, "gw": 0}.get(shape, 512)
        _assert_names(L, pl, models, n, width, True)
        E = _device_table(pl.E_all)
        launches = Launches(models, pl.chains, pl.n_out, chain_model=order)
        got = launches.run_all(E)
        _check(pl, got, order, f"{shape} multi-model")
        assert got["full"]["log_z"][0] != got["full"]["log_z"][1]  # the clean twins of one identity: two models
        _lib.check(L.hyg_tg_set_tail_overlap(0))
        off = launches.run("full", E)
        for k in ROWS + CHAIN:
            _same_bytes(off[k], got["full"][k], (shape, "tail overlap off", k))
    finally:
        L.hyg_tg_set_tail_overlap(1)
        L.hyg_tg_set_device_cus(0, 0)
        for m in models:
            m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["generic", "pipeline", "gw"])
def test_repeatable_and_nothing_left_behind(oracle, shape):
    """A second launch of every kind gives the bytes of the first, history
    workspace included; then the same objects and workspaces run every chain
    over clean rows and every chain is the oracle's clean one: no status and no
    history of a failed chain outlasts its launch."""
    L = _need_gpu()
    pl = en.plan(oracle, shape)
    n, T = len(pl.chains), pl.T
    models = _models(pl, 1)
    try:
        E = _device_table(pl.E_all)
        launches = Launches(models[0], pl.chains, pl.n_out)
        launches.obj["full"].ws.zero_()  # bytes no chain writes (a record's unused ancestors) compare equal
        first = launches.run_all(E)
        ws = launches.obj["full"].ws.cpu().numpy()
        assert (first["full"]["status"] == HYG_ENUMERIC).sum() >= 11
        again = launches.run_all(E)
        for kind in KINDS:
            for k in first[kind]:
                _same_bytes(again[kind][k], first[kind][k], (shape, kind, k))
        # the history records; behind them a GW shape keeps each chain's weights and sort keys, a scratch whose
        # bytes at the end of a launch are not part of any contract
        steps = n * T
        scratch = L.hyg_tg_workspace_bytes(models[0].handle, 2, steps) - L.hyg_tg_workspace_bytes(models[0].handle, 1, steps)
        assert (scratch >= 16 * models[0].num_particles) == pl.is_gw
        records = len(ws) - (n * scratch if pl.is_gw else 0)
        assert records > 0
        _same_bytes(launches.obj["full"].ws.cpu().numpy()[:records], ws[:records], (shape, "history records"))
        clean = _device_table(np.concatenate([pl.E] * (len(pl.E_all) // T)))
        got = launches.run_all(clean)
        for kind in KINDS:
            assert (got[kind]["status"] == 0).all(), kind
            for k in CHAIN:
                _same_bytes(got[kind][k], got["full"][k], (shape, kind, k))
        for i, (s0, _, sd, cid, o0) in enumerate(pl.chains):
            ref = pl.clean[(pl.specs[i][2], 0)]
            for k in ROWS:
                np.testing.assert_array_equal(got["full"][k][o0:o0 + T], ref[k], err_msg=f"chain {i} {k}")
            assert got["full"]["log_z"][i] == ref["log_z"] == got["trace_all"]["log_z_t"][o0 + T - 1], i
            np.testing.assert_array_equal(got["full"]["final_w"][i], ref["final_log_weights"], err_msg=f"chain {i}")
            t0 = pl.chains[pl.twin(i, 0)][4]
            for k in TRACE:
                _same_bytes(got["trace_all"][k][o0:o0 + T], got["trace_all"][k][t0:t0 + T], (shape, i, k))
        R = pl.expected(0, 0)["rows"]
        o0 = pl.chains[0][4]
        for k in TRACE:
            np.testing.assert_array_equal(got["trace_all"][k][o0:o0 + T][R["rows"]], R[k], err_msg=k)
    finally:
        for m in models:
            m.close()
