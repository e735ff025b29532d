"""Joint segmentations of the single-group path on the GPU
(hyg_sg_history_chains_multi, hyg_sg_sample_paths_multi, their host form and
`hygeia sg_sample_genome`): the history rows and the paths equal, bit for bit,
the reference of tests/sg_sample_ref.py (tied to tests/sg_filter_ref.py and to
the exact posterior in tests/test_sg_sample_cpu.py).
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import sg_filter_ref as fref  # noqa: E402
from tests import sg_sample_ref as sr  # noqa: E402
from tests.test_gpu_sg_multi import _model, _same  # noqa: E402

SEED = 5
# (K, u, N_max, T): (a) growth only; (b) optimal-resampling and keep-top steps;
# (c) the full-width set from t = 15, a ragged last wave; (d) as (c), all four waves full
SHAPES = {"a": (2, 1, 250, 48), "b": (3, 2, 12, 90), "c": (16, 1, 250, 24), "d": (16, 1, 256, 20)}
LW_FILL, ST_FILL, PATH_FILL = -123.25, 0xABCDEF01, 77


@pytest.fixture(scope="module")
def lib():
    from hygeia_amd import _lib

    L = _lib.load()
    if L.hyg_device_count() <= 0:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")
    return L


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _emission(lib, h, meth, tot, K):
    from hygeia_amd import _lib

    T, S = tot.shape
    dm = torch.from_numpy(np.ascontiguousarray(meth, np.uint16).view(np.int16)).cuda()
    dt = torch.from_numpy(np.ascontiguousarray(tot, np.uint16).view(np.int16)).cuda()
    E = torch.empty((T, K), dtype=torch.float64, device="cuda")
    _lib.check(lib.hyg_sg_emission(h, dm.data_ptr(), dt.data_ptr(), S, T, E.data_ptr(), _stream()))
    return E


def _chain_array(specs):
    """specs: (site_begin, n_sites, seed, chain_id, out_begin)"""
    from hygeia_amd import _lib

    arr = (_lib.SgChain * len(specs))()
    for i, (b, n, seed, cid, ob) in enumerate(specs):
        arr[i] = _lib.SgChain(b, n, 0, seed, cid, ob)
    return arr


def run_history(lib, handles, arr, cm, E, Nmax, rows, plain=False):
    """The history launch of the chains `arr` (plain: hyg_sg_filter_chains_multi
    instead, no history). Every output starts from a value the kernel never writes."""
    from hygeia_amd import _lib

    n = len(cm)
    models = (C.c_void_p * len(handles))(*[h.value for h in handles])
    cmv = (C.c_int32 * n)(*cm)
    wsb = lib.hyg_sg_filter_workspace_bytes_multi(models, len(handles), n)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    dev = dict(
        log_z=torch.full((n,), float("nan"), dtype=torch.float64, device="cuda"),
        final_log_weights=torch.full((n, Nmax), float("nan"), dtype=torch.float64, device="cuda"),
        final_states=torch.full((n, Nmax, 2), -7, dtype=torch.int32, device="cuda"),
        n_particles=torch.full((n,), -7, dtype=torch.int32, device="cuda"),
        status=torch.full((n,), 99, dtype=torch.int32, device="cuda"),
        h_lw=torch.full((rows, Nmax), LW_FILL, dtype=torch.float64, device="cuda"),
        h_st=torch.from_numpy(np.full((rows, Nmax), ST_FILL, np.uint32).view(np.int32)).cuda(),
        h_n=torch.full((rows,), -9, dtype=torch.int32, device="cuda"))
    head = [models, len(handles), arr, cmv, n, E.data_ptr(), ws.data_ptr(), wsb]
    tail = [dev[k].data_ptr() for k in ("log_z", "final_log_weights", "final_states", "n_particles", "status")]
    if plain:
        _lib.check(lib.hyg_sg_filter_chains_multi(*head, *tail, _stream()))
    else:
        hist = _lib.SgHistory(dev["h_lw"].data_ptr(), dev["h_st"].data_ptr(), dev["h_n"].data_ptr())
        _lib.check(lib.hyg_sg_history_chains_multi(*head, C.byref(hist), *tail, _stream()))
    torch.cuda.synchronize()
    return dev


def run_sample(lib, handles, arr, cm, h_lw, h_st, h_n, fwd_status, B, rows):
    """The sampler on device history arrays; returns (paths [rows][B][2], sample_status [n])."""
    from hygeia_amd import _lib

    n = len(cm)
    models = (C.c_void_p * len(handles))(*[h.value for h in handles])
    cmv = (C.c_int32 * n)(*cm)
    paths = torch.full((rows, B, 2), PATH_FILL, dtype=torch.int16, device="cuda")
    sst = torch.full((n,), 99, dtype=torch.int32, device="cuda")
    hist = _lib.SgHistory(h_lw.data_ptr(), h_st.data_ptr(), h_n.data_ptr())
    _lib.check(lib.hyg_sg_sample_paths_multi(models, len(handles), arr, cmv, n, C.byref(hist),
                                             fwd_status.data_ptr() if fwd_status is not None else None, B,
                                             paths.data_ptr(), sst.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return paths.cpu().numpy(), sst.cpu().numpy()


class Shape:
    """One shape: data, model, the reference history (computed once), the
    history launch of its one chain and the plain forward-only launch."""

    def __init__(self, lib, name):
        self.K, self.u, self.Nmax, self.T = SHAPES[name]
        self.lib = lib
        self.p, self.meth, self.tot, self.Eh = sr.synthetic_case(self.K, self.u, self.Nmax, self.T)
        self.tb = fref.Tables(self.p, self.T)
        self.ref = sr.history(self.p, self.Eh, SEED, 3, tables=self.tb)
        self.h = _model(lib, self.p, max(int(self.tot.max()), 1), self.T + 10)
        self.E = _emission(lib, self.h, self.meth, self.tot, self.K)
        assert np.array_equal(self.E.cpu().numpy(), self.Eh)
        self.arr = _chain_array([(0, self.T, SEED, 3, 0)])
        self.dev = run_history(lib, [self.h], self.arr, [0], self.E, self.Nmax, self.T)
        self.plain = run_history(lib, [self.h], self.arr, [0], self.E, self.Nmax, self.T, plain=True)


_SHAPES = []


@functools.lru_cache(maxsize=None)
def _shape_cached(name):
    from hygeia_amd import _lib

    _SHAPES.append(Shape(_lib.load(), name))
    return _SHAPES[-1]


@pytest.fixture
def shape(request, lib):
    return _shape_cached(request.param)


@pytest.fixture(scope="module", autouse=True)
def _free_shapes():
    yield
    for s in _SHAPES:
        s.lib.hyg_sg_model_destroy(s.h)
    del _SHAPES[:]
    _shape_cached.cache_clear()


def check_history(dev, row0, ref, Nmax, what):
    """rows row0 .. of a history launch against a reference history"""
    lw, st, npart = sr.history_arrays(ref, Nmax)
    T = npart.shape[0]
    g_lw = dev["h_lw"].cpu().numpy()[row0:row0 + T]
    g_st = dev["h_st"].cpu().numpy().view(np.uint32)[row0:row0 + T]
    g_n = dev["h_n"].cpu().numpy()[row0:row0 + T]
    assert np.array_equal(g_n, npart), (what, "n_particles")
    live = np.arange(Nmax)[None, :] < npart[:, None]
    # entries n >= N_t are not written: they keep the fill values
    assert np.array_equal(np.where(live, g_st, ST_FILL), np.where(live, st, ST_FILL)), (what, "states")
    assert np.all(g_st[~live] == ST_FILL) and np.all(g_lw[~live] == LW_FILL), (what, "entries beyond N_t")
    _same(np.where(live, g_lw, 0.0), np.where(live, lw, 0.0), (what, "log_weights"))


@pytest.mark.parametrize("shape", list(SHAPES), indirect=True)
def test_history_rows_equal_reference(shape):
    """1. n_particles, states and log-weight bits for n < N at every t; log_z,
    the final set, n_particles and status are the plain forward-only launch's."""
    assert shape.ref["status"] == 0
    check_history(shape.dev, 0, shape.ref, shape.Nmax, SHAPES)
    for k in ("log_z", "final_log_weights", "final_states", "n_particles", "status"):
        _same(shape.dev[k].cpu().numpy().astype(np.float64), shape.plain[k].cpu().numpy().astype(np.float64), k)
    assert shape.dev["status"].item() == 0 and shape.dev["log_z"].item() == shape.ref["log_z"]
    n_last = len(shape.ref["sets"][-1][0])
    assert shape.dev["n_particles"].item() == n_last == min(shape.Nmax, shape.K * shape.T)


@pytest.mark.parametrize("shape,B", [("a", 25), ("b", 25), ("c", 25), ("d", 25), ("a", 1024)], indirect=["shape"])
def test_paths_equal_reference(shape, B):
    """2. paths == sample(...) bit for bit: B = 25 is seven groups of four waves,
    the last with one wave."""
    want, wst = sr.sample(shape.ref["sets"], shape.tb, shape.T, B, SEED, 3)
    assert wst == 0 and np.all(want[:, :, 1] >= 0)
    got, sst = run_sample(shape.lib, [shape.h], shape.arr, [0], shape.dev["h_lw"], shape.dev["h_st"],
                          shape.dev["h_n"], shape.dev["status"], B, shape.T)
    assert sst.tolist() == [0]
    assert np.array_equal(got, want)
    assert len({got[:, b].tobytes() for b in range(B)}) > 1  # the draws differ between trajectories


def _bad_params(K, u, Nmax):
    """A model that ends in HYG_ENUMERIC (tests/test_sg_filter_cpu.py enumeric_case
    at this shape): an empty transition matrix and a hazard that exits early."""
    from oracle import sg_binding as sg

    mu, sigma = sr.case_moments(K)
    p = sg.make_params(K=K, mu=mu, sigma=sigma, omega=[1e-6] * K, u=u, Nmax=Nmax, kappa=2.0)
    for i in range(K * (K - 1)):
        p.theta[i] = float("-inf")
    return p


def test_six_chains_two_models_one_enumeric(lib):
    """3. one launch of six chains under three models at shape (b): lengths 1, 2,
    7, 40, 90 and a chain that ends in HYG_ENUMERIC; out_begin interleaves the
    chains' rows and leaves rows that no chain owns."""
    from hygeia_amd import _lib
    from oracle import sg_binding as sg

    K, u, Nmax, T = SHAPES["b"]
    B = 25
    p0, meth, tot, Eh = sr.synthetic_case(K, u, Nmax, T)
    mu, sigma = sr.case_moments(K)
    p1 = sg.make_params(K=K, mu=mu, sigma=sigma, omega=[0.8] * K, u=u, Nmax=Nmax, kappa=3.0)
    bad = _bad_params(K, u, Nmax)
    ps = [p0, p1, bad]
    handles = [_model(lib, p, max(int(tot.max()), 1), T + 10) for p in ps]
    try:
        E = _emission(lib, handles[0], meth, tot, K)
        # (site_begin, n_sites, model); rows: chain order 3, 0, 5, 1, 4, 2 with gaps of 3 unowned rows
        spec = [(5, 1, 0), (20, 2, 1), (0, 7, 0), (30, 40, 1), (0, 90, 0), (0, 40, 2)]
        order, row, ob = [3, 0, 5, 1, 4, 2], 2, {}
        for i in order:
            ob[i] = row
            row += spec[i][1] + 3
        rows = row
        chains = [(b, n, SEED, 11 + i, ob[i]) for i, (b, n, _) in enumerate(spec)]
        cm = [m for _, _, m in spec]
        arr = _chain_array(chains)
        fb = fref.forward(bad, Eh[:40], SEED, 16, marginals=False)
        assert fb["status"] == _lib.HYG_ENUMERIC and 0 < fb["t_stop"] < 40
        dev = run_history(lib, handles, arr, cm, E, Nmax, rows)
        assert dev["status"].cpu().tolist() == [0, 0, 0, 0, 0, _lib.HYG_ENUMERIC]
        got, sst = run_sample(lib, handles, arr, cm, dev["h_lw"], dev["h_st"], dev["h_n"], dev["status"], B, rows)
        assert sst.tolist() == [0, 0, 0, 0, 0, _lib.HYG_ENUMERIC]
        owned = np.zeros(rows, bool)
        g_n = dev["h_n"].cpu().numpy()
        for i, (b, n, m) in enumerate(spec):
            owned[ob[i]:ob[i] + n] = True
            if i == 5:  # the bad chain: -1 everywhere, the history rows from t_stop on are empty
                assert np.all(got[ob[i]:ob[i] + n] == -1)
                assert np.all(g_n[ob[i] + fb["t_stop"]:ob[i] + n] == 0) and np.all(g_n[ob[i]:ob[i] + fb["t_stop"]] > 0)
                continue
            one = _chain_array([(b, n, SEED, 11 + i, 0)])
            d1 = run_history(lib, [handles[m]], one, [0], E, Nmax, n)
            for k in ("h_lw", "h_st", "h_n"):
                assert torch.equal(dev[k][ob[i]:ob[i] + n], d1[k]), (i, k)
            for k in ("log_z", "final_log_weights", "final_states", "n_particles", "status"):
                _same(dev[k][i].cpu().numpy().astype(np.float64), d1[k][0].cpu().numpy().astype(np.float64), (i, k))
            g1, s1 = run_sample(lib, [handles[m]], one, [0], d1["h_lw"], d1["h_st"], d1["h_n"], d1["status"], B, n)
            assert s1.tolist() == [0] and np.array_equal(got[ob[i]:ob[i] + n], g1), i
            # and the reference, for the chains it runs in a moment
            h = sr.history(ps[m], Eh[b:b + n], SEED, 11 + i)
            check_history(dev, ob[i], h, Nmax, ("six chains", i))
            want, _ = sr.sample(h["sets"], fref.Tables(ps[m], n), n, B, SEED, 11 + i)
            assert np.array_equal(got[ob[i]:ob[i] + n], want), i
        # rows no chain owns are untouched
        assert np.all(got[~owned] == PATH_FILL) and np.all(g_n[~owned] == -9)
        assert np.all(dev["h_lw"].cpu().numpy()[~owned] == LW_FILL)
    finally:
        for h in handles:
            lib.hyg_sg_model_destroy(h)


def _hand_history(sets, Nmax):
    lw, st, npart = sr.history_arrays({"sets": sets}, Nmax)
    lw = np.where(np.isnan(lw), LW_FILL, lw)
    return (torch.from_numpy(lw).cuda(), torch.from_numpy(st.view(np.int32)).cuda(), torch.from_numpy(npart).cuda())


def test_sampler_on_hand_made_histories(lib):
    """4. no forward launch: the wrap of d modulo 2^16 and the long fill; draws
    decided by uu alone; and the kernel's guard at a row without a finite logit."""
    from hygeia_amd import _lib
    from oracle import sg_binding as sg

    K, u, Nmax = 2, 1, 3
    T = 70000
    p = sg.make_params(K=K, mu=[0.7, 0.3], sigma=[0.15, 0.15], u=u, Nmax=Nmax)
    h = _model(lib, p, 4, T + 10)
    try:
        # one particle (t + 1, 0) with lw = 0 per row: every path is d = (t + 1) mod 2^16, r = 0
        sets = [([0.0], [(t + 1, 0)]) for t in range(T)]
        arr = _chain_array([(0, T, SEED, 1, 0)])
        got, sst = run_sample(lib, [h], arr, [0], *_hand_history(sets, Nmax), None, 3, T)
        assert sst.tolist() == [0]
        want_d = ((np.arange(T, dtype=np.int64) + 1) & 0xFFFF).astype(np.uint16).view(np.int16)
        assert np.array_equal(got[:, :, 0], np.repeat(want_d[:, None], 3, axis=1)) and np.all(got[:, :, 1] == 0)
        # T = 6, two particles per row with weights 1 : 3
        T2, B = 6, 64
        tb = fref.Tables(p, T2)
        lw2 = [0.0, float(np.log(3.0))]
        sets = [(list(lw2), [(1, 0), (1, 1)] if t == 0 else [(1, t % 2), (2, (t + 1) % 2)]) for t in range(T2)]
        arr = _chain_array([(0, T2, SEED, 2, 0)])
        want, wst = sr.sample(sets, tb, T2, B, SEED, 2)
        got, sst = run_sample(lib, [h], arr, [0], *_hand_history(sets, Nmax), None, B, T2)
        assert wst == 0 and sst.tolist() == [0] and np.array_equal(got, want)
        last = got[T2 - 1, :, 0]
        assert 0 < np.sum(last == 1) < np.sum(last == 2) < B  # both particles drawn, the heavier more often
        # the same with row 2 all -inf: a path whose segment starts at site 3 draws from it
        sets[2] = ([float("-inf")] * 2, sets[2][1])
        want, wst = sr.sample(sets, tb, T2, B, SEED, 2)
        got, sst = run_sample(lib, [h], arr, [0], *_hand_history(sets, Nmax), None, B, T2)
        assert wst == _lib.HYG_ENUMERIC and sst.tolist() == [_lib.HYG_ENUMERIC] and np.array_equal(got, want)
        hit = got[3, :, 0] == 1  # a segment starts at site 3
        assert hit.any() and np.all(got[:3][:, hit] == -1) and np.all(got[3:][:, hit] != -1)
        assert np.all(got[:, ~hit] != -1)
    finally:
        lib.hyg_sg_model_destroy(h)


def _command_reference(lib, single_group, data, chrom, seeds, B, Nmax, u):
    """What sg_sample_genome must write for one chromosome, by the reference."""
    from hygeia_amd import _lib
    from oracle import sg_binding as sg

    f = single_group.parse_flags([], single_group.SG_SAMPLE_FLAGS)
    K, fixed, alpha, beta = single_group._known_parameters(f)
    src = lambda n: str(data / f"{n}_{chrom}.txt.gz")  # noqa: E731
    tot = single_group.read_csv_matrix(src("n_total_reads_control")).astype(np.uint16)
    meth = single_group.read_csv_matrix(src("n_methylated_reads_control")).astype(np.uint16)
    pos = single_group.read_csv_matrix(src("positions"))[:, 0]
    kappa, omega = single_group._numbers(f["kappa"]), single_group._numbers(f["omega"])
    theta = single_group.theta_from_model(single_group.default_p(K), omega, None)
    p = _lib.SgParams()
    lib.hyg_sg_params_default(C.byref(p))
    p.n_regimes, p.minimum_duration, p.num_particles_max, p.theta_len = K, u, Nmax, K * K
    p.resample_type, p.is_kappa_fixed = 2, 1
    for r in range(K):
        p.alpha[r], p.beta[r], p.kappa[r] = float(alpha[r]), float(beta[r]), float(kappa[r])
    for j, v in enumerate(theta):
        p.theta[j] = float(v)
    po = sg.SgParams.from_buffer_copy(bytes(p))
    T = tot.shape[0]
    E = sg.emission(po, meth, tot)
    tb = fref.Tables(po, T)
    paths, logz = [], []
    for s in seeds:
        h = sr.history(po, E, s, 0, tables=tb)
        assert h["status"] == 0
        paths.append(sr.sample(h["sets"], tb, T, B, s, 0)[0])
        logz.append(h["log_z"])
    return pos, np.concatenate(paths, axis=1), logz


def test_sg_sample_genome_end_to_end(lib, tmp_path):
    """5. two chromosomes, two seeds, --aggregate_dir: the npz and tsv files are
    the reference's; a --history_gib that forces two launches gives the same
    bytes; get_change_points --segment_size 0 runs on the aggregate files."""
    from hygeia_amd import cli, single_group
    from tests.test_sg_filter_cpu import _tsv
    from tests.test_sg_multi_cpu import _write_chrom

    data, out, agg, out2, cp = (tmp_path / x for x in ("data", "out", "agg", "out2", "cp"))
    data.mkdir()
    sizes = {"3": 61, "8": 36}  # the readers take the first row as the header: T = 60 and 35
    for i, (chrom, rows) in enumerate(sizes.items()):
        _write_chrom(str(data), chrom, rows, seed=40 + i)
    B, Nmax, u, seeds = 5, 12, 2, (1, 2)
    common = ["sg_sample_genome", "--data_dir", str(data), "--n_particles", str(Nmax), "--u", str(u), "--seeds", "1,2",
              "--n_trajectories", str(B)]
    assert cli.main(common + ["--output_dir", str(out), "--aggregate_dir", str(agg)]) == 0
    head, rows = _tsv(out / "sg_sample.tsv")
    assert head == ["chrom", "seed", "n_sites", "log_z", "status"] and len(rows) == 4
    for chrom, n_rows in sizes.items():
        pos, paths, logz = _command_reference(lib, single_group, data, chrom, seeds, B, Nmax, u)
        z = np.load(out / f"sg_paths_{chrom}.npz")
        assert z["regimes"].dtype == np.int8 and z["durations"].dtype == np.int16
        assert np.array_equal(z["positions"], pos)
        assert np.array_equal(z["regimes"], paths[:, :, 1]) and np.array_equal(z["durations"], paths[:, :, 0])
        for s, lz in zip(seeds, logz):
            row = [r for r in rows if r[:2] == [chrom, str(s)]]
            assert len(row) == 1 and row[0][2] == str(n_rows - 1) and float(row[0][3]) == lz and row[0][4] == "HYG_OK"
    # two launches: a budget that holds the longer chromosome's two seeds and not both chromosomes
    one = 2 * single_group.history_bytes(60, Nmax)
    gib = (one + 16) / 2 ** 30
    assert len(single_group.history_groups([60, 35], 2, Nmax, gib * 2 ** 30)) == 2
    assert cli.main(common + ["--output_dir", str(out2), "--history_gib", repr(gib)]) == 0
    assert (out / "sg_sample.tsv").read_bytes() == (out2 / "sg_sample.tsv").read_bytes()
    for name in ("sg_paths_3.npz", "sg_paths_8.npz"):  # (the archive's members: a zip file carries its write time)
        a, b = np.load(out / name), np.load(out2 / name)
        assert sorted(a.files) == sorted(b.files) == ["durations", "positions", "regimes"]
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (name, k)
    # the change points of the sample, with no change to get_change_points
    assert cli.main(["get_change_points", "--results_dir", str(agg), "--output_dir", str(cp), "--chroms", "3,8",
                     "--segment_size", "0"]) == 0
    ctrl = (cp / "cp_control_candidates.tsv").read_text()
    case = (cp / "cp_case_candidates.tsv").read_text()
    assert len(ctrl.splitlines()) > 1 and ctrl == case
    for kind in ("split", "merge"):
        assert len((cp / f"cp_{kind}_candidates.tsv").read_text().splitlines()) == 1, kind
