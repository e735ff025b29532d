"""Multi-model launches of the single-group path (hyg_sg_run_chains_multi,
hyg_sg_run_chains_pe_multi, hyg_sg_run_chains_host_multi): chains that each
name their own model equal, bit for bit (f64, no tolerance anywhere), the CPU
oracle's chain under that model (oracle/sg_binding.py chain / chain_pe) and
single-model launches of the same chains. The shapes are the smallest at which
each path can go wrong; each first shows on the CPU that the oracle's chain
differs between two of its models, so a kernel that ignores the index fails.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LENS = [1, 45, 300, 900, 120, 640, 3]
SEED = 13


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


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _pe(use_adam, normalise, every, lr_fac):
    from hygeia_amd import _lib

    pe = _lib.SgPeParams()
    pe.use_adam, pe.normalise_gradients, pe.n_steps_without_update = use_adam, normalise, every
    pe.learning_rate_exponent, pe.learning_rate_factor = 0.1, lr_fac
    return pe


def _model(lib, p, max_reads, max_dur):
    from hygeia_amd import _lib

    pp = _lib.SgParams.from_buffer_copy(bytes(p))
    h = C.c_void_p()
    _lib.check(lib.hyg_sg_model_create(C.byref(pp), int(max_reads), int(max_dur), C.byref(h)))
    return h


def _data(K, T, S, cov, seed):
    from hygeia_amd import synthetic as syn

    mu, sgm = syn.regime_params(K)
    d = syn.simulate(T, S, 1, K=K, seed=seed, coverage=cov, omega=0.9, u=3)
    return np.ascontiguousarray(d["meth_control"]), np.ascontiguousarray(d["tot_control"]), mu, sgm


def _P(K, k):
    """Transition matrix k: rows tilted towards a different neighbour per model."""
    P = np.full((K, K), 1.0)
    for r in range(K):
        P[r, (r + 1 + k) % K] += 1.5 + k
    np.fill_diagonal(P, 0.0)
    return P / P.sum(axis=1, keepdims=True)


def _params(sg, K, mu, sgm, Nmax, n, kappa_fixed=True, shared_kappa=False, eps_last=None):
    """n models with distinct P, omega and kappa (shared_kappa: models 0 and 2
    have one kappa vector, bit for bit); eps_last: one more model, model 0 with
    another epsilon."""
    omegas = [0.9, 0.6, 0.75, 0.8]
    ps = []
    for k in range(n):
        kk = 0 if (shared_kappa and k == 2) else k
        kappa = [1.5 + 0.5 * kk + 0.1 * r for r in range(K)]
        ps.append(sg.make_params(K=K, mu=mu, sigma=sgm, P=_P(K, k), omega=[omegas[k]] * K, u=3, Nmax=Nmax,
                                 kappa=kappa, kappa_fixed=kappa_fixed))
    if eps_last is not None:
        kappa = [1.5 + 0.1 * r for r in range(K)]
        ps.append(sg.make_params(K=K, mu=mu, sigma=sgm, P=_P(K, 0), omega=[omegas[0]] * K, u=3, Nmax=Nmax,
                                 kappa=kappa, kappa_fixed=kappa_fixed, epsilon=eps_last))
    return ps


def _chains(lens, seed=SEED):
    from hygeia_amd import _lib

    arr = (_lib.SgChain * len(lens))()
    begins = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    for i, (b, n) in enumerate(zip(begins, lens)):
        arr[i].site_begin, arr[i].n_sites = int(b), int(n)
        arr[i].seed, arr[i].chain_id, arr[i].out_begin = seed, (i << 32) | 9, int(b)
    return arr, begins


class _Dev:
    """The device side of one shape: counts, emission table (formed with models[0])."""

    def __init__(self, lib, handles, meth, tot, K):
        from hygeia_amd import _lib

        self.lib, self.K, (self.total, self.S) = lib, K, tot.shape
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        dm = torch.from_numpy(meth.view(np.int16)).cuda()
        dt = torch.from_numpy(tot.view(np.int16)).cuda()
        self.E = torch.empty((self.total, K), dtype=torch.float64, device="cuda")
        _lib.check(lib.hyg_sg_emission(handles[0], dm.data_ptr(), dt.data_ptr(), self.S, self.total, self.E.data_ptr(),
                                       self.stream))

    def _outs(self, n, rows, dim):
        probs = torch.full((self.total, self.K), float("nan"), dtype=torch.float64, device="cuda")
        theta = torch.full((max(rows, 1), max(dim, 1)), float("nan"), dtype=torch.float64, device="cuda")
        st = torch.full((n,), 99, dtype=torch.int32, device="cuda")
        return probs, theta, st

    def multi(self, handles, cm, arr, n, cap, pe=None, rows=0, dim=0, short=0):
        """One multi-model launch; short: bytes taken off the workspace size passed."""
        from hygeia_amd import _lib

        lib = self.lib
        models = (C.c_void_p * len(handles))(*[h.value for h in handles])
        cmv = (C.c_int32 * n)(*cm)
        wsb = (lib.hyg_sg_pe_workspace_bytes_multi(models, len(handles), arr, n, cap) if pe is not None
               else lib.hyg_sg_workspace_bytes_multi(models, len(handles), n, cap))
        assert wsb > 0
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        probs, theta, st = self._outs(n, rows, dim)
        if pe is None:
            rc = lib.hyg_sg_run_chains_multi(models, len(handles), arr, cmv, n, self.E.data_ptr(), ws.data_ptr(),
                                             wsb - short, cap, probs.data_ptr(), st.data_ptr(), self.stream)
        else:
            rc = lib.hyg_sg_run_chains_pe_multi(models, len(handles), C.byref(pe), arr, cmv, n, self.E.data_ptr(),
                                                ws.data_ptr(), wsb - short, cap, probs.data_ptr(), theta.data_ptr(),
                                                st.data_ptr(), self.stream)
        if short:
            return rc
        _lib.check(rc)
        torch.cuda.synchronize()
        return probs.cpu().numpy(), theta.cpu().numpy(), st.cpu().numpy()

    def single(self, h, arr, n, cap, pe=None, rows=0, dim=0):
        """One single-model launch of the chains `arr`."""
        from hygeia_amd import _lib

        lib = self.lib
        wsb = lib.hyg_sg_pe_workspace_bytes(h, arr, n, cap) if pe is not None else lib.hyg_sg_workspace_bytes(h, n, cap)
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        probs, theta, st = self._outs(n, rows, dim)
        if pe is None:
            _lib.check(lib.hyg_sg_run_chains(h, arr, n, self.E.data_ptr(), ws.data_ptr(), wsb, cap, probs.data_ptr(),
                                             st.data_ptr(), self.stream))
        else:
            _lib.check(lib.hyg_sg_run_chains_pe(h, C.byref(pe), arr, n, self.E.data_ptr(), ws.data_ptr(), wsb, cap,
                                                probs.data_ptr(), theta.data_ptr(), st.data_ptr(), self.stream))
        torch.cuda.synchronize()
        return probs.cpu().numpy(), theta.cpu().numpy(), st.cpu().numpy()


def _same(a, b, what):
    bad = np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b))))
    assert bad.size == 0, (what, bad[:5], a[tuple(bad[0])], b[tuple(bad[0])])


def _oracle_pe(sg, p, pe, E, seed, chain_id):
    ope = sg.make_pe(use_adam=bool(pe.use_adam), normalise_gradients=bool(pe.normalise_gradients),
                     every=pe.n_steps_without_update, lr_exponent=pe.learning_rate_exponent,
                     lr_factor=pe.learning_rate_factor)
    return sg.chain_pe(p, ope, E, seed, chain_id)


def _plain_shape(lib, sg, K, Nmax, key_drop=0):
    """Shape 1: seven chains over three models (distinct P, omega, kappa, hazard
    table lengths) and a fourth that differs in epsilon only, in mixed order.
    At these omega the hazard does not reach its exit, so a table is as long
    as its model's max_duration allows: each model gets the max_duration of its
    own longest chain, below the launch's longest chain for all but one."""
    total = sum(LENS)
    meth, tot, mu, sgm = _data(K, total, 2, 12.0, 40 + K)
    ps = _params(sg, K, mu, sgm, Nmax, 3, eps_last=0.2)
    cm = [2, 0, 1, 2, 3, 0, 1]
    max_dur = [max(n for n, m in zip(LENS, cm) if m == k) + 10 for k in range(4)]
    dcaps = [sg.hazard(p, 0, d + 1)[2] for p, d in zip(ps, max_dur)]
    assert len(set(dcaps[:3])) == 3 and max_dur[1] < max(LENS), (dcaps, max_dur)
    Eh = sg.emission(ps[0], meth, tot)
    arr, begins = _chains(LENS)
    # on the CPU: the index matters (models 0 / 1 on chain 2, epsilon on chain 4)
    b, n = begins[2], LENS[2]
    assert not np.array_equal(sg.chain(ps[0], Eh[b:b + n], SEED, arr[2].chain_id)["regime_probs"],
                              sg.chain(ps[1], Eh[b:b + n], SEED, arr[2].chain_id)["regime_probs"])
    b, n = begins[4], LENS[4]
    assert not np.array_equal(sg.chain(ps[0], Eh[b:b + n], SEED, arr[4].chain_id)["regime_probs"],
                              sg.chain(ps[3], Eh[b:b + n], SEED, arr[4].chain_id)["regime_probs"])
    handles = [_model(lib, p, int(tot.max()), d) for p, d in zip(ps, max_dur)]
    try:
        dev = _Dev(lib, handles, meth, tot, K)
        if key_drop:
            assert lib.hyg_sg_force_key_drop(key_drop) == 0
        try:
            out, _, status = dev.multi(handles, cm, arr, len(LENS), 1024)
        finally:
            if key_drop:
                lib.hyg_sg_force_key_drop(0)
        assert np.all(status == 0), status
        for i, (b, n) in enumerate(zip(begins, LENS)):
            ref = sg.chain(ps[cm[i]], Eh[b:b + n], SEED, arr[i].chain_id)
            assert ref["status"] == 0
            _same(out[b:b + n], ref["regime_probs"], ("oracle", K, i))
        if not key_drop:
            from hygeia_amd import _lib

            for k, h in enumerate(handles):  # the same chains through the single-model entry, a launch per model
                idx = [i for i in range(len(LENS)) if cm[i] == k]
                sub = (_lib.SgChain * len(idx))(*[arr[i] for i in idx])
                one, _, st1 = dev.single(h, sub, len(idx), 1024)
                assert np.all(st1 == 0)
                for i in idx:
                    _same(out[begins[i]:begins[i] + LENS[i]], one[begins[i]:begins[i] + LENS[i]], ("single", K, i))
    finally:
        for h in handles:
            lib.hyg_sg_model_destroy(h)


@pytest.mark.parametrize("K,Nmax", [(6, 250), (12, 250), (3, 20), (5, 7)])
def test_multi_model_chains_bit_exact(lib, sg, K, Nmax):
    _plain_shape(lib, sg, K, Nmax)


def test_multi_model_exact_resort_path(lib, sg):
    """hyg_sg_force_key_drop(52): the packed sort's keys collide and the exact
    re-sort runs, under the multi-model build."""
    _plain_shape(lib, sg, 6, 250, key_drop=52)


PE_LENS = [1, 61, 300, 130, 26]
PE_CM = [1, 2, 0, 1, 2]


def _pe_shape(lib, sg, K, Nmax, pe, kappa_fixed, shared_kappa=False, single_too=False):
    total = sum(PE_LENS)
    meth, tot, mu, sgm = _data(K, total, 2, 12.0, 60 + K)
    ps = _params(sg, K, mu, sgm, Nmax, 3, kappa_fixed=kappa_fixed, shared_kappa=shared_kappa)
    dim = K * K if kappa_fixed else K * (K + 1)
    th0 = [np.array(p.theta[:dim]) for p in ps]
    assert not np.array_equal(th0[0], th0[1]) and not np.array_equal(th0[1], th0[2])
    if not kappa_fixed:
        lk = [t[K * K:] for t in th0]
        assert not np.array_equal(lk[0], lk[1])
        assert np.array_equal(lk[0], lk[2]) == shared_kappa  # two models, one lgk / dgk table
    Eh = sg.emission(ps[0], meth, tot)
    arr, begins = _chains(PE_LENS)
    b, n = begins[2], PE_LENS[2]
    r0 = _oracle_pe(sg, ps[0], pe, Eh[b:b + n], SEED, arr[2].chain_id)
    r1 = _oracle_pe(sg, ps[1], pe, Eh[b:b + n], SEED, arr[2].chain_id)
    assert not np.array_equal(r0["regime_probs"], r1["regime_probs"])
    assert not np.array_equal(r0["theta"], r1["theta"])
    every = pe.n_steps_without_update
    rows = [1 + (n - 1) // every for n in PE_LENS]
    handles = [_model(lib, p, int(tot.max()), max(PE_LENS) + 10) for p in ps]
    try:
        dev = _Dev(lib, handles, meth, tot, K)
        out, th, status = dev.multi(handles, PE_CM, arr, len(PE_LENS), 512, pe, sum(rows), dim)
        assert np.all(status == 0), status
        r = 0
        for i, (b, n) in enumerate(zip(begins, PE_LENS)):
            ref = _oracle_pe(sg, ps[PE_CM[i]], pe, Eh[b:b + n], SEED, arr[i].chain_id)
            assert ref["status"] == 0 and ref["theta"].shape == (rows[i], dim)
            _same(out[b:b + n], ref["regime_probs"], ("probs", K, i))
            _same(th[r:r + rows[i]], ref["theta"], ("theta", K, i))
            r += rows[i]
        assert not np.array_equal(th[sum(rows[:2])], th[sum(rows[:3]) - 1])  # chain 2's theta moved
    finally:
        for h in handles:
            lib.hyg_sg_model_destroy(h)


@pytest.mark.parametrize("K,adam,norm,every", [(6, 1, 0, 25), (12, 1, 0, 25), (4, 0, 1, 60)])
def test_multi_model_estimation_kappa_fixed(lib, sg, K, adam, norm, every):
    _pe_shape(lib, sg, K, 250, _pe(adam, norm, every, 0.01 if adam else 1e-4), True)


@pytest.mark.parametrize("K", [6, 4])
def test_multi_model_estimation_kappa_estimated(lib, sg, K):
    _pe_shape(lib, sg, K, 250, _pe(1, 0, 25, 0.01), False, shared_kappa=True)


def test_one_model_through_the_multi_entries(lib, sg):
    """n_models = 1: the bits of the single-model entries (device and host forms)."""
    from hygeia_amd import _lib

    K, lens = 6, [200, 1, 77]
    total = sum(lens)
    meth, tot, mu, sgm = _data(K, total, 2, 12.0, 71)
    p = _params(sg, K, mu, sgm, 250, 1)[0]
    pe = _pe(1, 0, 25, 0.01)
    rows = [1 + (n - 1) // 25 for n in lens]
    arr, begins = _chains(lens)
    h = _model(lib, p, int(tot.max()), max(lens) + 10)
    try:
        dev = _Dev(lib, [h], meth, tot, K)
        a, _, sa = dev.multi([h], [0, 0, 0], arr, 3, 256)
        b, _, sb = dev.single(h, arr, 3, 256)
        assert np.all(sa == 0) and np.all(sb == 0)
        _same(a, b, "run_chains")
        a, ta, sa = dev.multi([h], [0, 0, 0], arr, 3, 256, pe, sum(rows), K * K)
        b, tb, sb = dev.single(h, arr, 3, 256, pe, sum(rows), K * K)
        assert np.all(sa == 0) and np.all(sb == 0)
        _same(a, b, "run_chains_pe probs")
        _same(ta, tb, "run_chains_pe theta")
        # the host form: with and without estimation, against the one-chain host entries
        models = (C.c_void_p * 1)(h.value)
        cm = (C.c_int32 * 3)(0, 0, 0)
        for with_pe in (False, True):
            hp = np.full((total, K), np.nan)
            ht = np.full((sum(rows), K * K), np.nan)
            st = np.full(3, 99, np.int32)
            _lib.check(lib.hyg_sg_run_chains_host_multi(models, 1, C.byref(pe) if with_pe else None, _ptr(meth),
                                                        _ptr(tot), 2, total, arr, cm, 3, total, _ptr(hp), _ptr(ht),
                                                        _ptr(st)))
            assert np.all(st == 0)
            r = 0
            for i, (b0, n) in enumerate(zip(begins, lens)):
                one = np.full((n, K), np.nan)
                t1 = np.full((rows[i], K * K), np.nan)
                m1, n1 = np.ascontiguousarray(meth[b0:b0 + n]), np.ascontiguousarray(tot[b0:b0 + n])
                if with_pe:
                    _lib.check(lib.hyg_sg_run_chain_host_pe(h, C.byref(pe), _ptr(m1), _ptr(n1), 2, n, SEED,
                                                            arr[i].chain_id, _ptr(one), _ptr(t1)))
                    _same(ht[r:r + rows[i]], t1, ("host theta", i))
                else:
                    _lib.check(lib.hyg_sg_run_chain_host(h, _ptr(m1), _ptr(n1), 2, n, SEED, arr[i].chain_id,
                                                         _ptr(one)))
                _same(hp[b0:b0 + n], one, ("host probs", with_pe, i))
                r += rows[i]
    finally:
        lib.hyg_sg_model_destroy(h)


def test_more_chains_than_one_batch(lib, sg):
    """300 chains of 40 sites over three models in mixed order: the launch is
    split into batches, and the index array follows the batching offset."""
    K, n, T = 6, 300, 40
    meth, tot, mu, sgm = _data(K, n * T, 2, 12.0, 83)
    ps = _params(sg, K, mu, sgm, 250, 3)
    cm = [(i * 7 + i // 5) % 3 for i in range(n)]
    lens = [T] * n
    arr, begins = _chains(lens)
    Eh = sg.emission(ps[0], meth, tot)
    assert not np.array_equal(sg.chain(ps[0], Eh[:T], SEED, arr[0].chain_id)["regime_probs"],
                              sg.chain(ps[1], Eh[:T], SEED, arr[0].chain_id)["regime_probs"])
    handles = [_model(lib, p, int(tot.max()), T + 10) for p in ps]
    try:
        dev = _Dev(lib, handles, meth, tot, K)
        out, _, status = dev.multi(handles, cm, arr, n, 64)
        assert np.all(status == 0), status
        for i, b in enumerate(begins):
            ref = sg.chain(ps[cm[i]], Eh[b:b + T], SEED, arr[i].chain_id)
            _same(out[b:b + T], ref["regime_probs"], ("chain", i))
    finally:
        for h in handles:
            lib.hyg_sg_model_destroy(h)


def test_too_small_a_workspace_is_refused(lib, sg):
    K, lens = 6, [30, 50]
    meth, tot, mu, sgm = _data(K, sum(lens), 2, 12.0, 91)
    ps = _params(sg, K, mu, sgm, 250, 2)
    arr, _ = _chains(lens)
    handles = [_model(lib, p, int(tot.max()), 60) for p in ps]
    try:
        dev = _Dev(lib, handles, meth, tot, K)
        assert dev.multi(handles, [1, 0], arr, 2, 128, short=1) == -1
        assert b"hyg_sg_workspace_bytes_multi" in lib.hyg_last_error()
        assert dev.multi(handles, [1, 0], arr, 2, 128, _pe(1, 0, 25, 0.01), 4, K * K, short=1) == -1
        assert b"hyg_sg_pe_workspace_bytes_multi" in lib.hyg_last_error()
    finally:
        for h in handles:
            lib.hyg_sg_model_destroy(h)
