"""Forward-only single-group launches, everything that needs no GPU: the
restatement of the forward recursion (tests/sg_filter_ref.py) tied to the C
oracle and to the exact likelihood, the kernel-name entries, the refusals that
are raised before a device is looked for, and `hygeia sg_log_z` on a faked engine.
"""
import ctypes as C
import os

import numpy as np
import pytest

from hygeia_amd import _lib, cli, single_group
from hygeia_amd import synthetic as syn
from oracle import sg_binding as sg
from tests import sg_filter_ref as ref
from tests.test_sg_multi_cpu import _Models, _params, _run_args, _write_chrom

NEW = ("hyg_sg_filter_workspace_bytes", "hyg_sg_filter_workspace_bytes_multi", "hyg_sg_filter_chains",
       "hyg_sg_filter_chains_multi", "hyg_sg_trace_chains", "hyg_sg_trace_chains_multi",
       "hyg_sg_filter_chains_host_multi", "hyg_sg_trace_chains_host_multi", "hyg_sg_filter_kernel_name",
       "hyg_sg_filter_kernel_name_multi", "hyg_sg_trace_kernel_name", "hyg_sg_trace_kernel_name_multi")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _case(K, Nmax, T, seed, omega=0.9, coverage=12.0):
    mu, sgm = syn.regime_params(K)
    d = syn.simulate(T, 2, 1, K=K, seed=seed, coverage=coverage, omega=0.9, u=3)
    meth, tot = np.ascontiguousarray(d["meth_control"]), np.ascontiguousarray(d["tot_control"])
    p = sg.make_params(K=K, mu=mu, sigma=sgm, omega=[omega] * K, u=3, Nmax=Nmax, kappa=2.0)
    return p, sg.emission(p, meth, tot)


# ------------------------------------------------ the restatement's anchors
@pytest.mark.parametrize("K,Nmax,T", [(3, 20, 120), (5, 7, 60), (6, 250, 90)])
def test_restatement_equals_c_oracle(K, Nmax, T):
    """For every prefix length n the regime marginals at n - 1 are the row the
    C oracle stores for the last site of E[:n] (storeEstimates at the final
    site: the filtering marginals), and the particle counts are its nparts.
    (6, 250, 90) crosses from growing to capped at site 41."""
    p, E = _case(K, Nmax, T, 7 + K)
    f = ref.forward(p, E, 13, 9)
    assert f["status"] == 0 and f["t_stop"] == T
    for n in range(1, T + 1):
        o = sg.chain(p, E[:n], 13, 9, want_nparts=True)
        assert o["status"] == 0
        assert np.array_equal(o["regime_probs"][n - 1], f["regime_probs"][n - 1]), n
        assert np.array_equal(o["nparts"], f["nparts"][:n]), n
    assert f["nparts"][-1] == min(Nmax, K * T) and f["log_weights"].shape == (f["nparts"][-1],)
    assert f["log_z"] == f["log_z_t"][-1] == ref.lse(list(f["log_weights"]))
    assert f["cp_probs"][0] == pytest.approx(1.0, abs=1e-15)  # every particle of site 0 starts a segment
    assert np.all((f["states"][:, 0] >= 1) & (f["states"][:, 0] <= T) & (f["states"][:, 1] < K))


@pytest.mark.parametrize("K,Nmax,T", [(3, 250, 80), (6, 250, 40)])
def test_log_z_is_the_exact_likelihood_without_resampling(K, Nmax, T):
    """While N_prev + K <= Nmax the particle set enumerates every reachable
    (d, r), so log Z is the exact likelihood: the restatement against the plain
    numpy forward recursion over (d <= T, r) with the same hazard tables.
    Measured on these inputs (CPU): largest |difference| 1.137e-13 at K = 3,
    T = 80 (log Z = -337.66) and 4.263e-14 at K = 6, T = 40 (log Z = -127.21),
    i.e. below 4e-16 |log Z|: rounding only. Allowance: 4 x the larger, 4.55e-13."""
    assert K * T <= Nmax
    p, E = _case(K, Nmax, T, 31 + K)
    f = ref.forward(p, E, 1, 2, marginals=False)
    assert f["status"] == 0 and f["nparts"][-1] == K * T
    worst = 0.0
    for n in (1, 2, 3, T // 2, T - 1, T):
        worst = max(worst, abs(f["log_z_t"][n - 1] - ref.exact_log_z(p, E[:n])))
    print(f"K={K} T={T}: log Z = {f['log_z']!r}, largest |restatement - exact| = {worst:.3e}")
    assert worst <= 4.55e-13


def test_all_inf_model_is_enumeric_at_a_known_site():
    """The model of the GPU test's HYG_ENUMERIC case: K = 2 with an empty
    transition matrix (no fresh particle ever has weight) and a hazard that
    exits at d = 6 (no sojourn continues past it), so every weight of site 6 is
    -inf. The C oracle returns HYG_ENUMERIC from 7 sites on, the restatement
    stops at site 6."""
    p, E = enumeric_case()
    assert [sg.chain(p, E[:n], 3, 1)["status"] for n in (5, 6, 7, 8, 20)] == [0, 0, -2, -2, -2]
    f = ref.forward(p, E[:20], 3, 1)
    assert f["status"] == -2 and f["t_stop"] == 6 and f["log_z"] == float("-inf")
    assert np.all(np.isfinite(f["log_z_t"][:6])) and np.all(f["log_z_t"][6:] == float("-inf"))
    assert np.all(np.isnan(f["regime_probs"][6:])) and np.all(np.isnan(f["cp_probs"][6:]))


def enumeric_case(T=40, Nmax=9):
    K = 2
    mu, sgm = syn.regime_params(K)
    d = syn.simulate(T, 2, 1, K=K, seed=5, coverage=12.0, omega=0.9, u=3)
    meth, tot = np.ascontiguousarray(d["meth_control"]), np.ascontiguousarray(d["tot_control"])
    p = sg.make_params(K=K, mu=mu, sigma=sgm, omega=[1e-6] * K, u=3, Nmax=Nmax, kappa=2.0)
    p.theta[0] = p.theta[1] = float("-inf")
    return p, sg.emission(p, meth, tot)


# ------------------------------------------------------------ C ABI, no device
def test_new_entries_are_exported_and_sg_log_z_is_a_command(lib):
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert "sg_log_z" in cli.COMMANDS.split() and cli._SUBCOMMANDS["sg_log_z"][:2] == ("single_group", "sg_log_z")
    assert callable(single_group.sg_log_z) and callable(single_group.filter_many)


def _name(fn, *args):
    buf = C.create_string_buffer(128)
    need = fn(*args, buf, 128)
    assert need == len(buf.value) + 1, (need, buf.value)
    return buf.value.decode()


@pytest.mark.parametrize("K", [2, 6, 8, 9, 16])
def test_kernel_names(lib, K):
    nb = 512 if K <= 8 else 256
    with _Models(lib, [(_params(K=K), 100, 500), (_params(K=K, theta_shift=0.1), 100, 500)]) as m:
        assert _name(lib.hyg_sg_filter_kernel_name, m.h[0]) == f"sg_chain_kernel<{K},{nb},false,false,false,true,false>"
        assert _name(lib.hyg_sg_trace_kernel_name, m.h[0]) == f"sg_chain_kernel<{K},{nb},false,false,false,true,true>"
        assert _name(lib.hyg_sg_filter_kernel_name_multi, m.arr, 2) == \
            f"sg_chain_kernel<{K},{nb},false,false,true,true,false>"
        assert _name(lib.hyg_sg_trace_kernel_name_multi, m.arr, 2) == \
            f"sg_chain_kernel<{K},{nb},false,false,true,true,true>"
        # the length query, a short buffer, and the refusals
        assert lib.hyg_sg_filter_kernel_name(m.h[0], None, 0) == len(_name(lib.hyg_sg_filter_kernel_name, m.h[0])) + 1
        assert lib.hyg_sg_filter_kernel_name(m.h[0], None, -1) == _lib.HYG_EINVAL
        assert lib.hyg_sg_trace_kernel_name(None, None, 0) == _lib.HYG_EINVAL
    with _Models(lib, [(_params(K=K), 100, 500), (_params(K=K, u=2), 100, 500)]) as m:
        assert lib.hyg_sg_filter_kernel_name_multi(m.arr, 2, None, 0) == _lib.HYG_EINVAL
        assert b"minimum_duration" in lib.hyg_last_error()


def _entries(lib, models, n_models, single, ch, cm, n, buf, st, z, wsb=1 << 30, trace="full", which=range(6)):
    """Return codes of the entries `which` (0-2: filter single, multi, host; 3-5:
    the traced ones); single: a model handle for the single-model ones. Only
    entries that the case under test refuses are called: the pointers are host
    memory, which no check reads but a launch would."""
    p, zs, sp = (a.ctypes.data_as(C.c_void_p) for a in (buf, z, st))
    tr = {"full": _lib.SgTrace(p, p, p), "empty": _lib.SgTrace(None, None, None), "null": None}[trace]
    trp = C.byref(tr) if tr is not None else None
    total = buf.shape[0]
    host_tr = (None, None, None) if trace != "full" else (p, p, p)
    calls = [
        lambda: lib.hyg_sg_filter_chains(single, ch, n, p, p, wsb, p, None, None, None, sp, None),
        lambda: lib.hyg_sg_filter_chains_multi(models, n_models, ch, cm, n, p, p, wsb, p, None, None, None, sp, None),
        lambda: lib.hyg_sg_filter_chains_host_multi(models, n_models, zs, zs, 2, total, ch, cm, n, p, None, None, None,
                                                    sp),
        lambda: lib.hyg_sg_trace_chains(single, ch, n, p, p, wsb, trp, p, None, None, None, sp, None),
        lambda: lib.hyg_sg_trace_chains_multi(models, n_models, ch, cm, n, p, p, wsb, trp, p, None, None, None, sp,
                                              None),
        lambda: lib.hyg_sg_trace_chains_host_multi(models, n_models, zs, zs, 2, total, ch, cm, n, total, *host_tr, p,
                                                   None, None, None, sp),
    ]
    return [calls[i]() for i in which]


MULTI = [1, 2, 4, 5]   # the entries of _entries that take a model table
DEVICE = [0, 1, 3, 4]  # those that take a workspace


def test_refusals_before_any_device(lib):
    ch, buf, st, z = _run_args()
    E = _lib.HYG_EINVAL
    with _Models(lib, [(_params(), 100, 500), (_params(theta_shift=0.1), 100, 500)]) as m:
        for bad in ((0, 2), (-1, 0)):  # a model index out of range
            assert _entries(lib, m.arr, 2, m.h[0], ch, (C.c_int32 * 2)(*bad), 2, buf, st, z, which=MULTI) == [E] * 4
            assert b"chain_model[" in lib.hyg_last_error()
        cm = (C.c_int32 * 2)(0, 1)
        # a NULL trace and one with three NULL pointers
        for tr in ("null", "empty"):
            assert _entries(lib, m.arr, 2, m.h[0], ch, cm, 2, buf, st, z, trace=tr, which=[3, 4, 5]) == [E] * 3, tr
            assert b"null trace" in lib.hyg_last_error()
        # a workspace that is too small
        for entry, need in ((0, lib.hyg_sg_filter_workspace_bytes(m.h[0], 2)),
                            (1, lib.hyg_sg_filter_workspace_bytes_multi(m.arr, 2, 2))):
            assert _entries(lib, m.arr, 2, m.h[0], ch, cm, 2, buf, st, z, wsb=need - 1,
                            which=[entry, entry + 3]) == [E] * 2
            assert b"workspace too small" in lib.hyg_last_error()
        assert _entries(lib, m.arr, 2, m.h[0], ch, cm, 2, buf, st, z, wsb=8, which=DEVICE) == [E] * 4
        # the host trace: a chain outside the output rows, or before them
        p, zs, sp = (a.ctypes.data_as(C.c_void_p) for a in (buf, z, st))
        total = buf.shape[0]
        for ob in (-1, total - ch[1].n_sites + 1):
            ch2 = (_lib.SgChain * 2)(ch[0], ch[1])
            ch2[1].out_begin = ob
            assert lib.hyg_sg_trace_chains_host_multi(m.arr, 2, zs, zs, 2, total, ch2, cm, 2, total, p, p, p, p, None,
                                                      None, None, sp) == E
            assert b"output rows" in lib.hyg_last_error()
    # a chain longer than its own model's max_duration
    with _Models(lib, [(_params(), 100, 500), (_params(theta_shift=0.1), 100, 15)]) as m:
        cm = (C.c_int32 * 2)(0, 1)
        assert _entries(lib, m.arr, 2, m.h[1], ch, cm, 2, buf, st, z) == [E] * 6
        assert b"max_duration" in lib.hyg_last_error()
    # incompatible models
    with _Models(lib, [(_params(), 100, 500), (_params(u=2), 100, 500)]) as m:
        assert _entries(lib, m.arr, 2, m.h[0], ch, (C.c_int32 * 2)(0, 1), 2, buf, st, z, which=MULTI) == [E] * 4
        assert b"minimum_duration" in lib.hyg_last_error()
    # resample_type != 2 and more than 256 particles never become a model
    h = C.c_void_p()
    p = _params()
    p.resample_type = 1
    assert lib.hyg_sg_model_create(C.byref(p), 100, 500, C.byref(h)) == _lib.HYG_EUNSUPPORTED
    assert lib.hyg_sg_model_create(C.byref(_params(Nmax=257)), 100, 500, C.byref(h)) == _lib.HYG_EUNSUPPORTED


def test_entries_refuse_without_device(lib):
    if lib.hyg_device_count() > 0:
        pytest.skip("host without a GPU only")
    ch, buf, st, z = _run_args()
    with _Models(lib, [(_params(), 100, 500), (_params(theta_shift=0.1), 100, 500)]) as m:
        assert _entries(lib, m.arr, 2, m.h[0], ch, (C.c_int32 * 2)(1, 0), 2, buf, st, z) == [_lib.HYG_EDEVICE] * 6
        assert b"no CPU fallback" in lib.hyg_last_error()


def test_filter_workspace_is_the_header(lib):
    """no ring, no smoothing slots, nothing that grows with the chains' lengths"""
    with _Models(lib, [(_params(theta_shift=0.01 * k), 100, 500) for k in range(4)]) as m:
        one = lib.hyg_sg_filter_workspace_bytes(m.h[0], 22)
        sizes = [lib.hyg_sg_filter_workspace_bytes_multi(m.arr, k, 22) for k in range(1, 5)]
        assert 0 < one <= sizes[0] and sizes == sorted(sizes)
        assert sizes[-1] < 8192 and sizes[-1] < lib.hyg_sg_workspace_bytes_multi(m.arr, 4, 22, 1) // 100
        assert lib.hyg_sg_filter_workspace_bytes(None, 3) == 0
        assert lib.hyg_sg_filter_workspace_bytes_multi(m.arr, 0, 3) == 0
        assert lib.hyg_sg_filter_workspace_bytes_multi(m.arr, 2, -1) == 0


# ---------------------------------------------------------------- sg_log_z
@pytest.fixture
def fake_filter(monkeypatch):
    """filter_many replaced by a recorder whose log Z encodes the task"""
    calls = []

    def fake(L, K, u, alpha, beta, n_particles, tasks, trace=None, is_kappa_fixed=True):
        calls.append(dict(K=K, u=u, tasks=tasks, trace=trace, n_particles=n_particles, fixed=is_kappa_fixed))
        out = []
        for t in tasks:
            T = t["tot"].shape[0]
            z = -float(T) - 0.001 * (t["seed"] % 1000) - 10.0 * u + float(np.sum(t["theta_init"][-6:]))
            o = {"log_z": z, "status": 0, "n_particles": n_particles}
            if trace:
                o.update(log_z_t=np.linspace(0, z, T), regime_probs=np.full((T, K), 1.0 / K), cp_probs=np.zeros(T))
            out.append(o)
        return out

    monkeypatch.setattr(single_group, "filter_many", fake)
    monkeypatch.setattr(_lib, "load", lambda import_torch=True: object())
    monkeypatch.setattr(cli, "_use_task_device", lambda L: None)
    return calls


def _write_par(par, chrom, i, K=6):
    p = np.full((K, K), (1.0 + i) / 10)
    np.fill_diagonal(p, 0.0)
    single_group.write_csv(os.path.join(par, f"p_{chrom}.csv.gz"), [f"regime_{r + 1}" for r in range(K)],
                           [[repr(float(v)) for v in p[:, c]] for c in range(K)])
    single_group.write_vector(os.path.join(par, f"omega_{chrom}.csv.gz"), "omega", [0.9 - 0.1 * i] * K)
    single_group.write_vector(os.path.join(par, f"kappa_{chrom}.csv.gz"), "kappa", [2.0 + i] * K)


def _tsv(path):
    lines = open(path).read().splitlines()
    return lines[0].split("\t"), [ln.split("\t") for ln in lines[1:]]


def test_sg_log_z_grid_and_files(tmp_path, fake_filter):
    data, par, out = tmp_path / "data", tmp_path / "par", tmp_path / "out"
    data.mkdir()
    par.mkdir()
    for i, chrom in enumerate(("3", "4")):
        _write_chrom(str(data), chrom, 20 + i, seed=10 + i)
        _write_par(str(par), chrom, i)
    rc = cli.main(["sg_log_z", "--data_dir", str(data), "--output_dir", str(out), "--parameters_dir",
                   f"default,{par}", "--u", "3,5", "--seeds", "1,-73", "--n_particles", "100", "--epsilon", "0.5",
                   "--trace"])
    assert rc == 0
    # one launch per u; every (chromosome, parameter set, seed) chain in it, chain id 0
    assert [c["u"] for c in fake_filter] == [3, 5] and all(c["trace"] and c["n_particles"] == 100 for c in fake_filter)
    tasks = fake_filter[0]["tasks"]
    assert len(tasks) == 2 * 2 * 2 and all(t["chain_id"] == 0 for t in tasks)
    assert [t["seed"] for t in tasks[:2]] == [1, (-73) & (2 ** 64 - 1)]
    # the first row of every file is taken as its header, as estimate_genome reads them
    assert [t["tot"].shape for t in tasks[::4]] == [(19, 2), (20, 2)]
    assert tasks[0]["tot"] is tasks[3]["tot"]  # the chains of a chromosome share its counts
    K = 6
    assert np.array_equal(tasks[0]["theta_init"], single_group.theta_from_model(
        single_group.default_p(K), np.array([0.995, 0.975, 0.95, 0.925, 0.9, 0.9])))
    assert np.array_equal(tasks[2]["theta_init"], single_group.theta_from_model(np.full((K, K), 0.1), np.full(K, 0.9)))
    assert list(tasks[6]["kappa"]) == [3.0] * K and list(tasks[0]["kappa"]) == [2.0] * K
    head, rows = _tsv(out / "sg_log_z.tsv")
    assert head == ["chrom", "parameters", "u", "seed", "n_sites", "log_z", "status"]
    assert len(rows) == 16 and rows[0][:5] == ["3", "default", "3", "1", "19"] and rows[0][6] == "HYG_OK"
    assert rows[3][:5] == ["3", str(par), "3", "-73", "19"] and rows[8][2] == "5"
    head, srows = _tsv(out / "sg_log_z_summary.tsv")
    assert head == ["parameters", "u", "log_z", "n_chroms", "n_seeds"] and len(srows) == 4
    from hygeia_amd.evidence import log_mean_exp

    for s in srows:
        per = [log_mean_exp(np.array([float(r[5]) for r in rows if r[0] == c and r[1] == s[0] and r[2] == s[1]]))
               for c in ("3", "4")]
        assert float(s[2]) == sum(per) and s[3:] == ["2", "2"]
    names = sorted(n for n in os.listdir(out) if n.endswith(".npz"))
    assert names == sorted(f"sg_filter_{c}_{i}_{u}_{s}.npz" for c in (3, 4) for i in (0, 1) for u in (3, 5)
                           for s in (1, -73))
    z = np.load(out / "sg_filter_4_1_5_-73.npz")
    assert sorted(z.files) == ["cp_probs", "log_z_t", "regime_probs"] and z["regime_probs"].shape == (20, 6)
    assert z["log_z_t"][-1] == float([r for r in rows if r[:4] == ["4", str(par), "5", "-73"]][0][5])


def test_sg_log_z_without_trace_writes_no_npz_and_defaults(tmp_path, fake_filter):
    data, out = tmp_path / "data", tmp_path / "out"
    data.mkdir()
    _write_chrom(str(data), "7", 15, seed=3)
    assert cli.main(["sg_log_z", "--data_dir", str(data), "--output_dir", str(out)]) == 0
    assert sorted(os.listdir(out)) == ["sg_log_z.tsv", "sg_log_z_summary.tsv"]
    call = fake_filter[0]
    assert len(fake_filter) == 1 and call["u"] == 2 and not call["trace"] and call["n_particles"] == 250
    assert [t["seed"] for t in call["tasks"]] == [(-73) & (2 ** 64 - 1)]


@pytest.mark.parametrize("argv,needle", [
    (["--output_dir", "o"], "--data_dir is required"),
    (["--data_dir", "d"], "--output_dir is required"),
    (["--data_dir", "d", "--output_dir", "o", "--u", "3,x"], "invalid value for --u"),
    (["--data_dir", "d", "--output_dir", "o", "--u", "0"], "positive"),
    (["--data_dir", "d", "--output_dir", "o", "--seeds", "1,1"], "distinct"),
    (["--data_dir", "d", "--output_dir", "o", "--parameters_dir", "a,a"], "distinct"),
    (["--data_dir", "d", "--output_dir", "o", "--rng_seed", "3"], "unknown argument --rng_seed"),
])
def test_sg_log_z_flag_errors(capsys, argv, needle):
    assert cli.main(["sg_log_z"] + argv) == 1
    err = capsys.readouterr().err
    assert err.startswith("Error: ") and needle in err, err


def test_sg_log_z_reads_everything_before_writing(tmp_path, fake_filter, capsys):
    data, par, out = tmp_path / "data", tmp_path / "par", tmp_path / "out"
    data.mkdir()
    par.mkdir()
    for i, chrom in enumerate(("3", "4")):
        _write_chrom(str(data), chrom, 20, seed=i)
    _write_par(str(par), "3", 0)  # chromosome 4 has no parameter files
    rc = cli.main(["sg_log_z", "--data_dir", str(data), "--output_dir", str(out), "--parameters_dir", str(par)])
    assert rc == 1 and "chromosome 4" in capsys.readouterr().err
    assert not fake_filter and not out.exists()
    _write_chrom(str(data), "5", 12, seed=4, bad_meth=True)
    rc = cli.main(["sg_log_z", "--data_dir", str(data), "--output_dir", str(out), "--chroms", "3,5"])
    assert rc == 1 and "chromosome 5" in capsys.readouterr().err and not out.exists()
    assert cli.main(["sg_log_z", "--data_dir", str(data), "--output_dir", str(out), "--chroms", "3,3"]) == 1
