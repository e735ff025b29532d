"""Forward-only and traced launches of the single-group path
(hyg_sg_filter_chains[_multi], hyg_sg_trace_chains[_multi], the host forms and
`hygeia sg_log_z`): log Z, the final particle set and the filter trace equal,
bit for bit (f64, no tolerance), the sequential restatement of the forward
recursion (tests/sg_filter_ref.py, itself tied to the C oracle in
tests/test_sg_filter_cpu.py), the C oracle's last-site marginals and the full
launch's last rows. Data and models are those of tests/test_gpu_sg_multi.py.
"""
import ctypes as C
import functools
import gzip

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import sg_filter_ref as ref  # noqa: E402
from tests.test_gpu_sg_multi import _chains, _data, _model, _params, _same  # noqa: E402

LENS = [1, 61, 300, 130, 26]
CM = [1, 2, 0, 1, 2]
SEED = 13
SHAPES = [(6, 250), (12, 250), (3, 20), (5, 7), (2, 9)]
NINF = float("-inf")


@pytest.fixture(scope="module")
def lib():
    from hygeia_amd import _lib

    L = _lib.load()
    if L.hyg_device_count() <= 0:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")
    return L


@pytest.fixture(scope="module")
def sg():
    from oracle import sg_binding

    sg_binding.lib()
    return sg_binding


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def launch(lib, handles, arr, cm, n, E, Nmax, K, rows=0, trace=None, single=False, finals=True, short=0):
    """One forward-only launch (trace None) or traced launch (trace: which of
    log_z_t, regime_probs, cp_probs to ask for) of the chains `arr`; single: the
    single-model entry with handles[0]. Every output starts from a value the
    kernel never writes. Returns numpy arrays by name (or the return code when
    `short` bytes are taken off the workspace size)."""
    from hygeia_amd import _lib

    models = (C.c_void_p * len(handles))(*[h.value for h in handles])
    cmv = (C.c_int32 * n)(*cm)
    wsb = (lib.hyg_sg_filter_workspace_bytes(handles[0], n) if single
           else lib.hyg_sg_filter_workspace_bytes_multi(models, len(handles), n))
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    dev = dict(
        log_z=torch.full((n,), float("nan"), dtype=torch.float64, device="cuda"),
        final_log_weights=torch.full((n, Nmax), float("nan"), dtype=torch.float64, device="cuda"),
        final_states=torch.full((n, Nmax, 2), -7, dtype=torch.int32, device="cuda"),
        n_particles=torch.full((n,), -7, dtype=torch.int32, device="cuda"),
        status=torch.full((n,), 99, dtype=torch.int32, device="cuda"),
        log_z_t=torch.full((max(rows, 1),), float("nan"), dtype=torch.float64, device="cuda"),
        regime_probs=torch.full((max(rows, 1), K), -5.0, dtype=torch.float64, device="cuda"),
        cp_probs=torch.full((max(rows, 1),), -5.0, dtype=torch.float64, device="cuda"))
    fin = [dev[k].data_ptr() if finals else None for k in ("final_log_weights", "final_states", "n_particles")]
    tail = [dev["log_z"].data_ptr()] + fin + [dev["status"].data_ptr(), _stream()]
    head = ([handles[0], arr, n] if single else [models, len(handles), arr, cmv, n]) + [E.data_ptr(), ws.data_ptr(),
                                                                                        wsb - short]
    if trace is None:
        rc = (lib.hyg_sg_filter_chains if single else lib.hyg_sg_filter_chains_multi)(*head, *tail)
    else:
        tr = _lib.SgTrace(*[dev[k].data_ptr() if on else None
                            for k, on in zip(("log_z_t", "regime_probs", "cp_probs"), trace)])
        rc = (lib.hyg_sg_trace_chains if single else lib.hyg_sg_trace_chains_multi)(*head, C.byref(tr), *tail)
    if short:
        return rc
    _lib.check(rc)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dev.items()}


class Shape:
    """One (K, Nmax): the data, three models, the five chains, the device
    emission table and the traced multi-model launch every test compares with."""

    def __init__(self, lib, sg, K, Nmax):
        self.lib, self.sg, self.K, self.Nmax = lib, sg, K, Nmax
        self.total = sum(LENS)
        self.meth, self.tot, mu, sgm = _data(K, self.total, 2, 12.0, 60 + K)
        self.ps = _params(sg, K, mu, sgm, Nmax, 3)
        self.Eh = sg.emission(self.ps[0], self.meth, self.tot)
        self.arr, self.begins = _chains(LENS)
        self.handles = [_model(lib, p, int(self.tot.max()), max(LENS) + 10) for p in self.ps]
        from hygeia_amd import _lib

        dm = torch.from_numpy(self.meth.view(np.int16)).cuda()
        dt = torch.from_numpy(self.tot.view(np.int16)).cuda()
        self.E = torch.empty((self.total, K), dtype=torch.float64, device="cuda")
        _lib.check(lib.hyg_sg_emission(self.handles[0], dm.data_ptr(), dt.data_ptr(), 2, self.total,
                                       self.E.data_ptr(), _stream()))
        self.traced = self.run(trace=(True, True, True))
        self._refs = {}

    def run(self, **kw):
        return launch(self.lib, self.handles, self.arr, CM, len(LENS), self.E, self.Nmax, self.K, rows=self.total,
                      **kw)

    def ref(self, i):
        """the restatement of chain i (computed once)"""
        if i not in self._refs:
            b, n = self.begins[i], LENS[i]
            self._refs[i] = ref.forward(self.ps[CM[i]], self.Eh[b:b + n], SEED, self.arr[i].chain_id)
        return self._refs[i]


_SHAPES = []


@functools.lru_cache(maxsize=None)
def _shape_cached(K, Nmax):
    from hygeia_amd import _lib
    from oracle import sg_binding

    _SHAPES.append(Shape(_lib.load(), sg_binding, K, Nmax))
    return _SHAPES[-1]


@pytest.fixture
def shape(request, lib, sg):
    return _shape_cached(*request.param)


@pytest.fixture(scope="module", autouse=True)
def _free_shapes():
    """the shapes' models live as long as the module's tests"""
    yield
    for s in _SHAPES:
        for h in s.handles:
            s.lib.hyg_sg_model_destroy(h)
    del _SHAPES[:]
    _shape_cached.cache_clear()


def check_against_ref(out, i, row0, n, f, Nmax, what):
    """chain i of a launch (trace rows row0 .. row0 + n) against a restatement f"""
    assert out["status"][i] == f["status"], what
    _same(out["log_z_t"][row0:row0 + n], f["log_z_t"], (what, "log_z_t"))
    _same(out["regime_probs"][row0:row0 + n], f["regime_probs"], (what, "regime_probs"))
    _same(out["cp_probs"][row0:row0 + n], f["cp_probs"], (what, "cp_probs"))
    N = f["log_weights"].shape[0]
    assert out["n_particles"][i] == N, what
    lw = np.full(Nmax, NINF)
    lw[:N] = f["log_weights"]
    st = np.full((Nmax, 2), -1, np.int32)
    st[:N] = f["states"]
    _same(out["final_log_weights"][i], lw, (what, "final_log_weights"))
    assert np.array_equal(out["final_states"][i], st), (what, "final_states")
    _same(out["log_z"][i:i + 1], np.array([f["log_z"]]), (what, "log_z"))


@pytest.mark.parametrize("shape", SHAPES, indirect=True)
def test_traced_launch_equals_restatement(shape):
    """1. every output of the traced multi-model launch, bit for bit. At
    Nmax = 250 the restatement runs for chains 0, 1 and 4; the 300- and
    130-site chains are held by the oracle and self-consistency tests."""
    out = shape.traced
    assert np.all(out["status"] == 0), out["status"]
    for i in ([0, 1, 4] if shape.Nmax == 250 else range(len(LENS))):
        check_against_ref(out, i, shape.begins[i], LENS[i], shape.ref(i), shape.Nmax, (shape.K, shape.Nmax, i))
    for i, (b, n) in enumerate(zip(shape.begins, LENS)):
        assert out["log_z"][i] == out["log_z_t"][b + n - 1], i
    # the launch resamples at the capped shapes: the set is full at the end of the long chains
    assert out["n_particles"][2] == min(shape.Nmax, shape.K * LENS[2])


@pytest.mark.parametrize("shape", SHAPES, indirect=True)
def test_trace_rows_equal_oracle_and_full_launch(shape, sg):
    """2. regime_probs row n - 1 is the C oracle's last row on the prefix of n
    sites (the 61-site chain, shapes (6, 250) and (3, 20)); for all five chains
    the last row is the full launch's."""
    out = shape.traced
    if (shape.K, shape.Nmax) in ((6, 250), (3, 20)):
        i = 1
        b = shape.begins[i]
        for n in range(1, LENS[i] + 1):
            o = sg.chain(shape.ps[CM[i]], shape.Eh[b:b + n], SEED, shape.arr[i].chain_id)
            assert o["status"] == 0
            _same(out["regime_probs"][b + n - 1], o["regime_probs"][n - 1], ("oracle prefix", n))
    from hygeia_amd import _lib

    lib, n = shape.lib, len(LENS)
    models = (C.c_void_p * 3)(*[h.value for h in shape.handles])
    cmv = (C.c_int32 * n)(*CM)
    wsb = lib.hyg_sg_workspace_bytes_multi(models, 3, n, 1024)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    probs = torch.full((shape.total, shape.K), float("nan"), dtype=torch.float64, device="cuda")
    st = torch.full((n,), 99, dtype=torch.int32, device="cuda")
    _lib.check(lib.hyg_sg_run_chains_multi(models, 3, shape.arr, cmv, n, shape.E.data_ptr(), ws.data_ptr(), wsb, 1024,
                                           probs.data_ptr(), st.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert np.all(st.cpu().numpy() == 0)
    full = probs.cpu().numpy()
    for i, (b, m) in enumerate(zip(shape.begins, LENS)):
        _same(out["regime_probs"][b + m - 1], full[b + m - 1], ("full launch", i))


@pytest.mark.parametrize("shape", SHAPES, indirect=True)
def test_prefix_chains_reproduce_log_z_t(shape):
    """3. a forward-only launch whose chains are the prefixes 1 .. 61 of one
    chain (same seed, same chain id): log_z[n - 1] == log_z_t[n - 1]."""
    from hygeia_amd import _lib

    i, T = 1, LENS[1]
    b = int(shape.begins[i])
    arr = (_lib.SgChain * T)()
    for n in range(1, T + 1):
        arr[n - 1] = _lib.SgChain(b, n, 0, SEED, shape.arr[i].chain_id, 0)
    out = launch(shape.lib, shape.handles, arr, [CM[i]] * T, T, shape.E, shape.Nmax, shape.K)
    assert np.all(out["status"] == 0)
    _same(out["log_z"], shape.traced["log_z_t"][b:b + T], "prefix log_z")
    assert np.array_equal(out["n_particles"], np.minimum(shape.Nmax, shape.K * np.arange(1, T + 1)))


FINALS = ("log_z", "final_log_weights", "final_states", "n_particles", "status")


@pytest.mark.parametrize("shape", SHAPES, indirect=True)
def test_untraced_single_and_partial_traces(shape):
    """4. untraced == traced for all returned arrays; the single-model entries
    equal the multi entries with one model; a trace with one or two NULL
    pointers leaves the others' bits unchanged."""
    full = shape.traced
    un = shape.run()
    for k in FINALS:
        _same(un[k].astype(np.float64), full[k].astype(np.float64), ("untraced", k))
    assert np.all(np.isnan(un["log_z_t"])) and np.all(un["regime_probs"] == -5.0) and np.all(un["cp_probs"] == -5.0)
    # log Z alone: the optional outputs may be NULL
    bare = shape.run(finals=False)
    _same(bare["log_z"], full["log_z"], "log_z without the optional outputs")
    assert np.all(bare["n_particles"] == -7) and np.all(np.isnan(bare["final_log_weights"]))
    for mask in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        part = shape.run(trace=mask)
        for k, on, blank in zip(("log_z_t", "regime_probs", "cp_probs"), mask, (None, -5.0, -5.0)):
            if on:
                _same(part[k], full[k], ("partial trace", mask, k))
            elif blank is None:
                assert np.all(np.isnan(part[k])), (mask, k)
            else:
                assert np.all(part[k] == blank), (mask, k)
        for k in FINALS:
            _same(part[k].astype(np.float64), full[k].astype(np.float64), ("partial trace", mask, k))
    h1 = [shape.handles[1]]
    kw = dict(rows=shape.total)
    for tr in (None, (True, True, True)):
        one = launch(shape.lib, h1, shape.arr, [0] * len(LENS), len(LENS), shape.E, shape.Nmax, shape.K, trace=tr,
                     single=True, **kw)
        mul = launch(shape.lib, h1, shape.arr, [0] * len(LENS), len(LENS), shape.E, shape.Nmax, shape.K, trace=tr, **kw)
        for k in one:
            _same(one[k].astype(np.float64), mul[k].astype(np.float64), ("single vs multi", tr, k))
        for i in (0, 3):  # the chains that run under model 1 in the shared launch
            assert one["log_z"][i] == full["log_z"][i]
    # the refusals that need a device to come last: a short workspace enqueues nothing
    from hygeia_amd import _lib

    assert shape.run(short=1) == _lib.HYG_EINVAL
    assert b"workspace too small" in shape.lib.hyg_last_error()


def test_exact_resort_path(lib, sg):
    """5. hyg_sg_force_key_drop(52): the packed sort's keys collide and the
    exact re-sort runs; the bits are those of the production keys."""
    shape = _shape_cached(6, 250)
    assert lib.hyg_sg_force_key_drop(52) == 0
    try:
        out = shape.run(trace=(True, True, True))
    finally:
        lib.hyg_sg_force_key_drop(0)
    for k in out:
        _same(out[k].astype(np.float64), shape.traced[k].astype(np.float64), ("key drop", k))
    for i in (0, 1, 4):
        check_against_ref(out, i, shape.begins[i], LENS[i], shape.ref(i), 250, ("key drop", i))


def test_more_chains_than_one_batch(lib, sg):
    """6. 700 chains of 40 sites at K = 6 over three models in mixed order,
    forward-only: more workgroups than 2 x 256 CUs hold at once. Nmax = 50, so
    that the chains resample from site 8 on and their seeds matter. Ten chains
    equal the restatement, all equal a launch in reversed order."""
    from hygeia_amd import _lib

    K, Nmax, T, n = 6, 50, 40, 700
    meth, tot, mu, sgm = _data(K, 400, 2, 12.0, 91)
    ps = _params(sg, K, mu, sgm, Nmax, 3)
    Eh = sg.emission(ps[0], meth, tot)
    handles = [_model(lib, p, int(tot.max()), T + 10) for p in ps]
    try:
        dm = torch.from_numpy(meth.view(np.int16)).cuda()
        dt = torch.from_numpy(tot.view(np.int16)).cuda()
        E = torch.empty((400, K), dtype=torch.float64, device="cuda")
        _lib.check(lib.hyg_sg_emission(handles[0], dm.data_ptr(), dt.data_ptr(), 2, 400, E.data_ptr(), _stream()))
        cm = [(i * 7 + i // 5) % 3 for i in range(n)]
        begin = [(i * 13) % (400 - T) for i in range(n)]
        arr, rev = (_lib.SgChain * n)(), (_lib.SgChain * n)()
        for i in range(n):
            arr[i] = _lib.SgChain(begin[i], T, 0, SEED + i % 11, (i << 32) | 5, 0)
            rev[n - 1 - i] = arr[i]
        out = launch(lib, handles, arr, cm, n, E, Nmax, K)
        assert np.all(out["status"] == 0) and np.all(out["n_particles"] == Nmax)
        back = launch(lib, handles, rev, cm[::-1], n, E, Nmax, K)
        for k in FINALS:
            _same(out[k].astype(np.float64), back[k][::-1].astype(np.float64), ("reversed", k))
        for i in (0, 1, 255, 256, 511, 512, 513, 600, 698, 699):
            f = ref.forward(ps[cm[i]], Eh[begin[i]:begin[i] + T], SEED + i % 11, (i << 32) | 5, marginals=False)
            assert f["status"] == 0 and out["log_z"][i] == f["log_z"], i
            _same(out["final_log_weights"][i], f["log_weights"], ("spot", i))
            assert np.array_equal(out["final_states"][i], f["states"]), i
        assert len(set(out["log_z"].tolist())) > 600  # the chains differ
    finally:
        for h in handles:
            lib.hyg_sg_model_destroy(h)


def test_enumeric_chain_and_its_neighbours(lib, sg):
    """7. HYG_ENUMERIC: the K = 2 model of tests/test_sg_filter_cpu.py
    (enumeric_case: an empty transition matrix and a hazard that exits at d = 6,
    for which the C oracle returns HYG_ENUMERIC) makes every weight of site 6
    -inf. Its chain reports the status, the rows before site 6 are the
    restatement's, the rows from it hold -inf / NaN, and the other chains of the
    launch are untouched."""
    from hygeia_amd import _lib
    from tests.test_sg_filter_cpu import enumeric_case

    K, Nmax, T = 2, 9, 40
    bad, Eh = enumeric_case(T, Nmax)
    assert sg.chain(bad, Eh[:26], SEED, 7)["status"] == -2
    from hygeia_amd import synthetic as syn

    mu, sgm = syn.regime_params(K)
    good = _params(sg, K, mu, sgm, Nmax, 2)
    d = syn.simulate(T, 2, 1, K=K, seed=5, coverage=12.0, omega=0.9, u=3)  # the counts of enumeric_case
    meth, tot = np.ascontiguousarray(d["meth_control"]), np.ascontiguousarray(d["tot_control"])
    ps = [good[0], good[1], bad]
    handles = [_model(lib, p, int(tot.max()), T + 10) for p in ps]
    try:
        dm = torch.from_numpy(meth.view(np.int16)).cuda()
        dt = torch.from_numpy(tot.view(np.int16)).cuda()
        E = torch.empty((T, K), dtype=torch.float64, device="cuda")
        _lib.check(lib.hyg_sg_emission(handles[0], dm.data_ptr(), dt.data_ptr(), 2, T, E.data_ptr(), _stream()))
        assert np.array_equal(E.cpu().numpy(), Eh)
        # (site_begin, n_sites, model): chains 1 and 3 run under the failing model, chain 3 ends before site 6
        spec = [(0, 26, 0), (0, 26, 2), (10, 20, 1), (3, 4, 2)]
        arr = (_lib.SgChain * 4)()
        row = 0
        rows = []
        for i, (b, n, _) in enumerate(spec):
            arr[i] = _lib.SgChain(b, n, 0, SEED, 7 + i, row)
            rows.append(row)
            row += n
        out = launch(lib, handles, arr, [m for _, _, m in spec], 4, E, Nmax, K, rows=row, trace=(True, True, True))
        assert out["status"].tolist() == [0, _lib.HYG_ENUMERIC, 0, 0]
        for i, (b, n, m) in enumerate(spec):
            f = ref.forward(ps[m], Eh[b:b + n], SEED, 7 + i)
            check_against_ref(out, i, rows[i], n, f, Nmax, ("enumeric", i))
        r1 = rows[1]
        assert np.all(np.isfinite(out["log_z_t"][r1:r1 + 6])) and np.all(out["log_z_t"][r1 + 6:r1 + 26] == NINF)
        assert np.all(np.isnan(out["regime_probs"][r1 + 6:r1 + 26]))
        assert np.all(np.isnan(out["cp_probs"][r1 + 6:r1 + 26]))
        assert out["log_z"][1] == NINF and out["n_particles"][1] == 0 and np.all(out["final_states"][1] == -1)
        assert np.all(out["final_log_weights"][1] == NINF)
        # the same launch without the failing chain: the others' bits do not change
        keep = [0, 2, 3]
        sub = (_lib.SgChain * 3)(*[arr[i] for i in keep])
        alone = launch(lib, handles, sub, [spec[i][2] for i in keep], 3, E, Nmax, K, rows=row, trace=(True, True, True))
        for j, i in enumerate(keep):
            n = spec[i][1]
            for k in ("log_z_t", "regime_probs", "cp_probs"):
                _same(alone[k][rows[i]:rows[i] + n], out[k][rows[i]:rows[i] + n], ("alone", i, k))
            assert alone["log_z"][j] == out["log_z"][i]
        # untraced: the same status and finals
        un = launch(lib, handles, arr, [m for _, _, m in spec], 4, E, Nmax, K)
        for k in FINALS:
            _same(un[k].astype(np.float64), out[k].astype(np.float64), ("untraced enumeric", k))
    finally:
        for h in handles:
            lib.hyg_sg_model_destroy(h)


def test_log_z_is_unbiased_under_resampling(lib, sg):
    """8. K = 3, Nmax = 12, T = 150, 512 seeds in one forward-only launch: with
    Z* from the exact numpy recursion the mean of exp(log_z_i - log Z*) lies
    within 4 sample standard errors of 1 (Z is an unbiased estimate under the
    optimal resampling). Data: coverage 12, omega 0.9, simulation seed 77, for
    which the restatement run on seeds 0 .. 63 on the CPU gives a per-chain
    relative standard deviation of 0.0094 (mean 1.0018), far below 2."""
    from hygeia_amd import _lib
    from hygeia_amd import synthetic as syn

    K, Nmax, T, n = 3, 12, 150, 512
    mu, sgm = syn.regime_params(K)
    d = syn.simulate(T, 2, 1, K=K, seed=77, coverage=12.0, omega=0.9, u=3)
    meth, tot = np.ascontiguousarray(d["meth_control"]), np.ascontiguousarray(d["tot_control"])
    p = sg.make_params(K=K, mu=mu, sigma=sgm, omega=[0.9] * K, u=3, Nmax=Nmax, kappa=2.0)
    Eh = sg.emission(p, meth, tot)
    z_star = ref.exact_log_z(p, Eh)
    h = _model(lib, p, int(tot.max()), T + 10)
    try:
        dm = torch.from_numpy(meth.view(np.int16)).cuda()
        dt = torch.from_numpy(tot.view(np.int16)).cuda()
        E = torch.empty((T, K), dtype=torch.float64, device="cuda")
        _lib.check(lib.hyg_sg_emission(h, dm.data_ptr(), dt.data_ptr(), 2, T, E.data_ptr(), _stream()))
        arr = (_lib.SgChain * n)()
        for i in range(n):
            arr[i] = _lib.SgChain(0, T, 0, i, 0, 0)
        out = launch(lib, [h], arr, [0] * n, n, E, Nmax, K, single=True)
    finally:
        lib.hyg_sg_model_destroy(h)
    assert np.all(out["status"] == 0) and np.all(out["n_particles"] == Nmax)  # the launch really resamples
    ratio = np.exp(out["log_z"] - z_star)
    assert len(set(ratio.tolist())) > n // 2  # the seeds matter
    se = ratio.std(ddof=1) / np.sqrt(n)
    print(f"log Z* = {z_star!r}; mean ratio {ratio.mean()!r}, sd {ratio.std(ddof=1):.4g}, se {se:.4g}")
    assert se < 0.1
    assert abs(ratio.mean() - 1.0) <= 4 * se, (ratio.mean(), se)
    for s in (0, 63, 511):  # and the launch is the restatement's chain
        assert out["log_z"][s] == ref.forward(p, Eh, s, 0, marginals=False)["log_z"], s


def test_sg_log_z_command_end_to_end(lib, sg, tmp_path):
    """9. `hygeia sg_log_z` on a two-chromosome tree with two parameter
    directories, --u 3,5 --seeds 1,2 --trace: every log_z of the TSV is the
    C-ABI launch's, the summary its log-mean-exp sum, every npz the trace. One
    parameter directory and the seed come from `estimate_genome` runs of the
    same tree: the last regime_probs row is the last row of that run's
    regimes_{chrom}.csv.gz (the smoothed estimate of the last site is the
    filtering one) after R formatting."""
    from hygeia_amd import _lib, cli, single_group
    from hygeia_amd.evidence import log_mean_exp
    from tests.test_sg_filter_cpu import _tsv, _write_par
    from tests.test_sg_multi_cpu import _write_chrom

    data, est, par_b, reg, out = (tmp_path / x for x in ("data", "est", "par_b", "reg", "out"))
    data.mkdir()
    par_b.mkdir()
    sizes = {"3": 64, "8": 41}
    for i, (chrom, rows) in enumerate(sizes.items()):
        _write_chrom(str(data), chrom, rows, seed=20 + i)
        _write_par(str(par_b), chrom, i)
    common = ["--data_dir", str(data), "--n_particles", "50", "--randomise_rng_seed", "FALSE"]
    assert cli.main(["estimate_genome", "--output_dir", str(est), "--estimate_parameters", "--rng_seed", "4",
                     "--n_steps_without_parameter_update", "10", "--u", "3"] + common) == 0
    assert cli.main(["estimate_genome", "--output_dir", str(reg), "--estimate_regime_probabilities", "--rng_seed", "1",
                     "--parameters_dir", str(est), "--u", "3"] + common) == 0
    assert cli.main(["sg_log_z", "--data_dir", str(data), "--output_dir", str(out), "--n_particles", "50",
                     "--parameters_dir", f"{est},{par_b}", "--u", "3,5", "--seeds", "1,2", "--trace"]) == 0
    head, rows = _tsv(out / "sg_log_z.tsv")
    assert len(rows) == 2 * 2 * 2 * 2 and all(r[6] == "HYG_OK" for r in rows)
    K = 6
    f = single_group.parse_flags([], single_group.SG_LOG_Z_FLAGS)
    _, _, alpha, beta = single_group._known_parameters(f)
    for chrom, n_rows in sizes.items():
        src = lambda n: str(data / f"{n}_{chrom}.txt.gz")  # noqa: E731
        tot = single_group.read_csv_matrix(src("n_total_reads_control")).astype(np.uint16)
        meth = single_group.read_csv_matrix(src("n_methylated_reads_control")).astype(np.uint16)
        T = n_rows - 1  # the readers take the first row as the header
        for i, d in enumerate((est, par_b)):
            par = lambda n: str(d / f"{n}_{chrom}.csv.gz")  # noqa: E731
            kappa = single_group.read_csv_matrix(par("kappa"))[:, 0]
            theta = single_group.theta_from_model(single_group.read_csv_matrix(par("p")),
                                                  single_group.read_csv_matrix(par("omega"))[:, 0])
            for u in (3, 5):
                p = _lib.SgParams()
                lib.hyg_sg_params_default(C.byref(p))
                p.n_regimes, p.minimum_duration, p.num_particles_max, p.theta_len = K, u, 50, K * K
                for r in range(K):
                    p.alpha[r], p.beta[r], p.kappa[r] = float(alpha[r]), float(beta[r]), float(kappa[r])
                for j, v in enumerate(theta):
                    p.theta[j] = float(v)
                h = C.c_void_p()
                _lib.check(lib.hyg_sg_model_create(C.byref(p), max(int(tot.max()), 1), T + 10, C.byref(h)))
                try:
                    dm = torch.from_numpy(meth.view(np.int16)).cuda()
                    dt = torch.from_numpy(tot.view(np.int16)).cuda()
                    E = torch.empty((T, K), dtype=torch.float64, device="cuda")
                    _lib.check(lib.hyg_sg_emission(h, dm.data_ptr(), dt.data_ptr(), 2, T, E.data_ptr(), _stream()))
                    arr = (_lib.SgChain * 2)(_lib.SgChain(0, T, 0, 1, 0, 0), _lib.SgChain(0, T, 0, 2, 0, T))
                    o = launch(lib, [h], arr, [0, 0], 2, E, 50, K, rows=2 * T, trace=(True, True, True), single=True)
                finally:
                    lib.hyg_sg_model_destroy(h)
                for j, seed in enumerate((1, 2)):
                    row = [r for r in rows if r[:4] == [chrom, str(d), str(u), str(seed)]]
                    assert len(row) == 1 and int(row[0][4]) == T and float(row[0][5]) == o["log_z"][j], row
                    z = np.load(out / f"sg_filter_{chrom}_{i}_{u}_{seed}.npz")
                    for k in ("log_z_t", "regime_probs", "cp_probs"):
                        _same(z[k], o[k][j * T:(j + 1) * T], ("npz", chrom, i, u, seed, k))
    head, srows = _tsv(out / "sg_log_z_summary.tsv")
    assert len(srows) == 4
    for s in srows:
        per = [log_mean_exp(np.array([float(r[5]) for r in rows if r[0] == c and r[1] == s[0] and r[2] == s[1]]))
               for c in sizes]
        assert float(s[2]) == sum(per) and s[3:] == ["2", "2"]
    # estimate_genome's chain: its parameters, its seed, chain id 0
    for chrom in sizes:
        with gzip.open(reg / f"regimes_{chrom}.csv.gz", "rt") as fh:
            lines = fh.read().splitlines()
        cols = np.array([[x for x in ln.split(",")] for ln in lines[1:]])
        last = np.load(out / f"sg_filter_{chrom}_0_3_1.npz")["regime_probs"][-1]
        for r in range(K):
            col = np.array([float(x) for x in cols[:, 1 + r]])
            col[-1] = last[r]
            assert single_group.r_format_column(col)[-1] == cols[-1, 1 + r], (chrom, r)
