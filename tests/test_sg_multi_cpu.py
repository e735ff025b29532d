"""The single-group multi-model entries on a host without a GPU
(hyg_sg_models_compatible, the workspace sizes, argument checks of the run
entries) and `hygeia estimate_genome` over a faked run_engine_many: flags,
chromosome discovery, refusals that name the chromosome, the files written.
"""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from hygeia_amd import _lib, cli, single_group


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _params(K=6, u=3, Nmax=250, kappa_fixed=1, theta_shift=0.0, kappa=2.0, epsilon=0.01, alpha_ulp=False):
    p = _lib.SgParams()
    _lib.load().hyg_sg_params_default(C.byref(p))
    p.n_regimes, p.minimum_duration, p.num_particles_max, p.is_kappa_fixed = K, u, Nmax, kappa_fixed
    p.theta_len = K * K if kappa_fixed else K * (K + 1)
    for r in range(K):
        p.alpha[r], p.beta[r], p.kappa[r] = 2.0 + r, 3.0 + r, kappa + 0.25 * r
    for i in range(K * (K - 1)):
        p.theta[i] = -1.0 + 0.01 * i + theta_shift
    for i in range(K):
        p.theta[K * (K - 1) + i] = 2.0 + theta_shift
        if not kappa_fixed:
            p.theta[K * K + i] = float(np.log(kappa + 0.25 * i))
    if alpha_ulp:
        p.alpha[K - 1] = float(np.nextafter(p.alpha[K - 1], 100.0))
    p.epsilon = epsilon
    return p


class _Models:
    def __init__(self, lib, specs):
        self.lib, self.h = lib, []
        for p, reads, dur in specs:
            h = C.c_void_p()
            assert lib.hyg_sg_model_create(C.byref(p), reads, dur, C.byref(h)) == _lib.HYG_OK, lib.hyg_last_error()
            self.h.append(h)
        self.arr = (C.c_void_p * len(self.h))(*[h.value for h in self.h])
        self.n = len(self.h)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        for h in self.h:
            self.lib.hyg_sg_model_destroy(h)


def test_compatible_accepts_theta_kappa_epsilon_max_duration(lib):
    specs = [(_params(), 100, 500), (_params(theta_shift=0.3, kappa=3.0, epsilon=0.05), 100, 90),
             (_params(theta_shift=-0.2), 100, 2000)]
    with _Models(lib, specs) as m:
        assert lib.hyg_sg_models_compatible(m.arr, m.n) == _lib.HYG_OK
        assert lib.hyg_sg_models_compatible(m.arr, 1) == _lib.HYG_OK


@pytest.mark.parametrize("other,reads,field", [
    (dict(K=5), 100, b"n_regimes"),
    (dict(u=2), 100, b"minimum_duration"),
    (dict(Nmax=200), 100, b"num_particles_max"),
    (dict(kappa_fixed=0), 100, b"is_kappa_fixed"),
    (dict(), 101, b"max_total_reads"),
    (dict(alpha_ulp=True), 100, b"alpha"),
])
def test_compatible_refuses_and_names_the_field(lib, other, reads, field):
    with _Models(lib, [(_params(), 100, 500), (_params(theta_shift=0.1), 100, 500),
                       (_params(**other), reads, 500)]) as m:
        assert lib.hyg_sg_models_compatible(m.arr, 2) == _lib.HYG_OK
        assert lib.hyg_sg_models_compatible(m.arr, 3) == _lib.HYG_EINVAL
        msg = lib.hyg_last_error()
        assert field in msg and b"models 0 and 2" in msg, msg


def _run_args(n_chains=2, T=20, K=6):
    ch = (_lib.SgChain * n_chains)()
    for i in range(n_chains):
        ch[i].site_begin, ch[i].n_sites, ch[i].out_begin = i * T, T, i * T
    buf = np.zeros((n_chains * T, K))
    st = np.zeros(n_chains, np.int32)
    z = np.zeros((n_chains * T, 2), np.uint16)
    return ch, buf, st, z


def _all_entries(lib, models, n_models, ch, cm, n, buf, st, z):
    """Return codes of the three run entries (device pointers are never touched
    before the checks under test)."""
    pe = _lib.SgPeParams()
    lib.hyg_sg_pe_params_default(C.byref(pe))
    p = buf.ctypes.data_as(C.c_void_p)
    zs = z.ctypes.data_as(C.c_void_p)
    sp = st.ctypes.data_as(C.c_void_p)
    total = buf.shape[0]
    return [
        lib.hyg_sg_run_chains_multi(models, n_models, ch, cm, n, p, p, 1 << 30, 0, p, sp, None),
        lib.hyg_sg_run_chains_pe_multi(models, n_models, C.byref(pe), ch, cm, n, p, p, 1 << 30, 0, p, p, sp, None),
        lib.hyg_sg_run_chains_host_multi(models, n_models, None, zs, zs, 2, total, ch, cm, n, total, p, None, sp),
        lib.hyg_sg_run_chains_host_multi(models, n_models, C.byref(pe), zs, zs, 2, total, ch, cm, n, total, p, p, sp),
    ]


def test_bad_index_null_entry_and_no_models_are_einval(lib):
    ch, buf, st, z = _run_args()
    with _Models(lib, [(_params(), 100, 500), (_params(theta_shift=0.1), 100, 500)]) as m:
        for bad in ((0, 2), (-1, 0)):
            cm = (C.c_int32 * 2)(*bad)
            assert _all_entries(lib, m.arr, 2, ch, cm, 2, buf, st, z) == [_lib.HYG_EINVAL] * 4
            assert b"chain_model[" in lib.hyg_last_error()
        cm = (C.c_int32 * 2)(0, 1)
        assert _all_entries(lib, m.arr, 0, ch, cm, 2, buf, st, z) == [_lib.HYG_EINVAL] * 4
        holed = (C.c_void_p * 2)(m.h[0].value, None)
        assert _all_entries(lib, holed, 2, ch, cm, 2, buf, st, z) == [_lib.HYG_EINVAL] * 4
        assert b"null model 1" in lib.hyg_last_error()
        assert lib.hyg_sg_models_compatible(holed, 2) == _lib.HYG_EINVAL
        assert lib.hyg_sg_models_compatible(m.arr, 0) == _lib.HYG_EINVAL
        assert lib.hyg_sg_models_compatible(None, 1) == _lib.HYG_EINVAL
        # incompatible models are refused by the run entries as well
    with _Models(lib, [(_params(), 100, 500), (_params(u=2), 100, 500)]) as m:
        assert _all_entries(lib, m.arr, 2, ch, cm, 2, buf, st, z) == [_lib.HYG_EINVAL] * 4
        assert b"minimum_duration" in lib.hyg_last_error()


def test_run_entries_refuse_without_device(lib):
    if lib.hyg_device_count() > 0:
        pytest.skip("host without a GPU only")
    ch, buf, st, z = _run_args()
    cm = (C.c_int32 * 2)(1, 0)
    with _Models(lib, [(_params(), 100, 500), (_params(theta_shift=0.1), 100, 500)]) as m:
        assert _all_entries(lib, m.arr, 2, ch, cm, 2, buf, st, z) == [_lib.HYG_EDEVICE] * 4
        assert b"no CPU fallback" in lib.hyg_last_error()


def test_workspace_sizes(lib):
    ch, _, _, _ = _run_args(n_chains=5, T=300)
    specs = [(_params(theta_shift=0.01 * k), 100, 500) for k in range(6)]
    with _Models(lib, specs) as m:
        for cap in (0, 64):
            one = lib.hyg_sg_workspace_bytes(m.h[0], 5, cap)
            one_pe = lib.hyg_sg_pe_workspace_bytes(m.h[0], ch, 5, cap)
            sizes = [lib.hyg_sg_workspace_bytes_multi(m.arr, k, 5, cap) for k in range(1, 7)]
            sizes_pe = [lib.hyg_sg_pe_workspace_bytes_multi(m.arr, k, ch, 5, cap) for k in range(1, 7)]
            assert sizes[0] >= one > 0 and sizes_pe[0] >= one_pe > one
            assert sizes == sorted(sizes) and sizes_pe == sorted(sizes_pe)
            assert sizes[-1] > sizes[0] and sizes_pe[-1] > sizes_pe[0]
        assert lib.hyg_sg_workspace_bytes_multi(m.arr, 0, 5, 0) == 0
        assert lib.hyg_sg_workspace_bytes_multi(None, 1, 5, 0) == 0
        assert lib.hyg_sg_pe_workspace_bytes_multi(m.arr, 2, None, 5, 0) == 0


# --------------------------------------------------------- estimate_genome
def _write_chrom(d, chrom, rows, S=2, group="control", seed=0, bad_meth=False):
    rng = np.random.default_rng(seed)
    tot = rng.integers(1, 30, (rows, S))
    meth = (tot * rng.random((rows, S))).astype(int)
    if bad_meth:
        meth[3, 0] = tot[3, 0] + 1
    pos = np.cumsum(rng.integers(1, 50, rows))
    for name, a in ((f"positions_{chrom}", pos[:, None]), (f"n_total_reads_{group}_{chrom}", tot),
                    (f"n_methylated_reads_{group}_{chrom}", meth)):
        with gzip.open(os.path.join(d, f"{name}.txt.gz"), "wt") as fh:
            fh.write("\n".join(",".join(str(v) for v in row) for row in a) + "\n")


@pytest.fixture
def fake_engine(monkeypatch):
    """run_engine_many replaced by a recorder that returns fixed probabilities
    and, with estimation, theta rows that start at each task's theta_init."""
    calls = []

    def fake(L, K, u, alpha, beta, epsilon, n_particles, tasks, estimate_parameters, pe_flags=None,
             is_kappa_fixed=True):
        calls.append(dict(K=K, u=u, tasks=tasks, pe=estimate_parameters, fixed=is_kappa_fixed,
                          n_particles=n_particles, epsilon=epsilon))
        out = []
        for t in tasks:
            T = t["tot"].shape[0]
            probs = np.full((T, K), 1.0 / K)
            theta = None
            if estimate_parameters:
                every = int(pe_flags["n_steps_without_parameter_update"])
                theta = np.tile(np.asarray(t["theta_init"], float), (1 + (T - 1) // every, 1))
            out.append((probs, theta))
        return out

    monkeypatch.setattr(single_group, "run_engine_many", fake)
    monkeypatch.setattr(_lib, "load", lambda import_torch=True: object())
    monkeypatch.setattr(cli, "_use_task_device", lambda L: None)
    return calls


def test_estimate_genome_flags_discovery_and_files(tmp_path, fake_engine):
    data, out = tmp_path / "data", tmp_path / "out"
    data.mkdir()
    for i, (chrom, rows) in enumerate((("10", 40), ("2", 25), ("X", 12), ("1", 31))):
        _write_chrom(str(data), chrom, rows, seed=i)
    _write_chrom(str(data), "7", 9, group="case")  # not this group's: no control files
    os.remove(data / "n_methylated_reads_control_1.txt.gz")  # incomplete: not discovered
    rc = cli.main(["estimate_genome", "--data_dir", str(data), "--output_dir", str(out), "--estimate_parameters",
                   "--estimate_regime_probabilities", "--randomise_rng_seed", "FALSE", "--rng_seed", "5,6,7",
                   "--n_steps_without_parameter_update", "10", "--u", "3", "--n_particles=100"])
    assert rc == 0
    call = fake_engine[0]
    assert len(fake_engine) == 1 and call["K"] == 6 and call["u"] == 3 and call["pe"] and call["n_particles"] == 100
    # --chroms all: numbered chromosomes in numeric order, then the rest by name
    assert single_group.genome_chroms(str(data), "control") == ["2", "10", "X"]
    assert [t["seed"] for t in call["tasks"]] == [5, 6, 7] and all(t["chain_id"] == 0 for t in call["tasks"])
    # the first row of every file is taken as its header (the single command's readers)
    assert [t["tot"].shape for t in call["tasks"]] == [(24, 2), (39, 2), (11, 2)]
    th0 = [t["theta_init"] for t in call["tasks"]]
    assert np.array_equal(th0[0], np.random.default_rng(5).standard_normal(36))
    assert not np.array_equal(th0[0], th0[1]) and not np.array_equal(th0[1], th0[2])
    assert (out / "rng_seeds.csv").read_text() == "chrom,rng_seed\n2,5\n10,6\nX,7\n"
    names = sorted(os.listdir(out))
    assert names == sorted(["rng_seeds.csv"] + [f"{stem}_{c}.csv.gz" for c in ("2", "10", "X")
                                                 for stem in ("regimes", "theta_trace", "p", "kappa", "omega", "theta")])
    with gzip.open(out / "theta_10.csv.gz", "rt") as fh:
        rows = fh.read().split()
    assert rows[0] == "data" and [float(x) for x in rows[1:]] == pytest.approx(list(th0[1]), rel=1e-15)
    assert cli.read_theta(str(out), "10").shape == (36,)


def test_estimate_genome_parameters_dir_and_one_seed(tmp_path, fake_engine):
    data, par, out = tmp_path / "data", tmp_path / "par", tmp_path / "out"
    data.mkdir()
    par.mkdir()
    K = 6
    for i, chrom in enumerate(("3", "4")):
        _write_chrom(str(data), chrom, 20 + i, seed=10 + i)
        p = np.full((K, K), (1.0 + i) / 10)
        np.fill_diagonal(p, 0.0)
        single_group.write_csv(str(par / f"p_{chrom}.csv.gz"), [f"regime_{r + 1}" for r in range(K)],
                               [[repr(float(v)) for v in p[:, c]] for c in range(K)])
        single_group.write_vector(str(par / f"omega_{chrom}.csv.gz"), "omega", [0.9 - 0.1 * i] * K)
        single_group.write_vector(str(par / f"kappa_{chrom}.csv.gz"), "kappa", [2.0 + i] * K)
    rc = cli.main(["estimate_genome", "--data_dir", str(data), "--output_dir", str(out), "--chroms", "4,3",
                   "--parameters_dir", str(par), "--estimate_regime_probabilities", "--randomise_rng_seed", "FALSE",
                   "--rng_seed", "11"])
    assert rc == 0
    tasks = fake_engine[0]["tasks"]
    assert not fake_engine[0]["pe"] and [t["seed"] for t in tasks] == [11, 11]
    assert list(tasks[0]["kappa"]) == [3.0] * K and list(tasks[1]["kappa"]) == [2.0] * K
    p4 = np.full((K, K), 0.2)
    assert np.array_equal(tasks[0]["theta_init"], single_group.theta_from_model(p4, np.full(K, 0.8)))
    assert sorted(os.listdir(out)) == ["regimes_3.csv.gz", "regimes_4.csv.gz", "rng_seeds.csv"]
    assert (out / "rng_seeds.csv").read_text() == "chrom,rng_seed\n4,11\n3,11\n"


def test_estimate_genome_randomised_seeds_are_recorded(tmp_path, fake_engine):
    data, out = tmp_path / "data", tmp_path / "out"
    data.mkdir()
    for chrom in ("1", "2"):
        _write_chrom(str(data), chrom, 15)
    assert cli.main(["estimate_genome", "--data_dir", str(data), "--output_dir", str(out),
                     "--estimate_regime_probabilities"]) == 0
    seeds = [t["seed"] for t in fake_engine[0]["tasks"]]
    assert seeds[0] != seeds[1]
    assert (out / "rng_seeds.csv").read_text() == f"chrom,rng_seed\n1,{seeds[0]}\n2,{seeds[1]}\n"


def test_recorded_random_seeds_rerun_exactly(tmp_path, fake_engine):
    """A drawn seed is a full 64-bit value (almost always above 2^53, where a
    double no longer holds every integer): passed back through --rng_seed, to
    this command or to the single one, it gives the same task seed and theta_0."""
    data, out = tmp_path / "data", tmp_path / "out"
    data.mkdir()
    for chrom in ("1", "2"):
        _write_chrom(str(data), chrom, 15)
    common = ["--data_dir", str(data), "--estimate_parameters", "--n_steps_without_parameter_update", "5"]
    assert cli.main(["estimate_genome", "--output_dir", str(out)] + common) == 0
    first = fake_engine[0]["tasks"]
    recorded = [line.split(",")[1] for line in (out / "rng_seeds.csv").read_text().split()[1:]]
    assert [int(x) for x in recorded] == [t["seed"] for t in first]
    assert cli.main(["estimate_genome", "--output_dir", str(tmp_path / "again"), "--randomise_rng_seed", "FALSE",
                     "--rng_seed", ",".join(recorded)] + common) == 0
    again = fake_engine[1]["tasks"]
    for a, b in zip(first, again):
        assert a["seed"] == b["seed"] and np.array_equal(a["theta_init"], b["theta_init"])
    # a seed that no double holds, through both commands' parsers
    big = 17293822569102704641
    assert float(big) != big
    assert single_group.parse_flags(["--rng_seed", str(big)])["rng_seed"] == big
    assert single_group.parse_flags(["--rng_seed", "3.0"])["rng_seed"] == 3
    assert cli.main(["estimate_genome", "--output_dir", str(tmp_path / "big"), "--randomise_rng_seed", "FALSE",
                     "--rng_seed", f"{big},-73"] + common) == 0
    assert [t["seed"] for t in fake_engine[2]["tasks"]] == [big, (-73) & (2 ** 64 - 1)]
    assert np.array_equal(fake_engine[2]["tasks"][0]["theta_init"], np.random.default_rng(big).standard_normal(36))


def test_estimate_genome_parameter_files_of_another_length_are_refused(tmp_path, fake_engine, capsys):
    data, par, out = tmp_path / "data", tmp_path / "par", tmp_path / "out"
    data.mkdir()
    par.mkdir()
    for chrom, n in (("3", 6), ("4", 5)):
        _write_chrom(str(data), chrom, 20)
        pm = np.full((6, 6), 0.2)
        single_group.write_csv(str(par / f"p_{chrom}.csv.gz"), [f"regime_{r + 1}" for r in range(6)],
                               [[repr(float(v)) for v in pm[:, c]] for c in range(6)])
        single_group.write_vector(str(par / f"omega_{chrom}.csv.gz"), "omega", [0.9] * 6)
        single_group.write_vector(str(par / f"kappa_{chrom}.csv.gz"), "kappa", [2.0] * n)
    assert cli.main(["estimate_genome", "--data_dir", str(data), "--output_dir", str(out), "--parameters_dir",
                     str(par), "--estimate_regime_probabilities", "--randomise_rng_seed", "FALSE"]) == 1
    err = capsys.readouterr().err
    assert "chromosome 4" in err and "6 regimes" in err and not fake_engine and not out.exists()


@pytest.mark.parametrize("case,needle", [("seeds", "--rng_seed has 2 values for 3 chromosomes"),
                                         ("missing", "chromosome 9"), ("samples", "chromosome 8"),
                                         ("meth", "chromosome 5")])
def test_estimate_genome_refusals_name_the_chromosome_and_write_nothing(tmp_path, fake_engine, capsys, case, needle):
    data, out = tmp_path / "data", tmp_path / "out"
    data.mkdir()
    _write_chrom(str(data), "5", 20, bad_meth=(case == "meth"))
    _write_chrom(str(data), "8", 20, S=3 if case == "samples" else 2)
    _write_chrom(str(data), "9", 20)
    if case == "missing":
        os.remove(data / "n_total_reads_control_9.txt.gz")
    argv = ["estimate_genome", "--data_dir", str(data), "--output_dir", str(out), "--chroms", "5,8,9",
            "--estimate_regime_probabilities", "--randomise_rng_seed", "FALSE",
            "--rng_seed", "1,2" if case == "seeds" else "1,2,3"]
    assert cli.main(argv) == 1
    err = capsys.readouterr().err
    assert "hygeia estimate_genome: " in err and needle in err
    assert not fake_engine and not out.exists()


def test_estimate_genome_flag_errors(capsys):
    assert cli.main(["estimate_genome", "--output_dir", "x"]) == 1
    assert "Error: --data_dir is required" in capsys.readouterr().err
    # the per-file flags of the single command are not this command's
    assert cli.main(["estimate_genome", "--data_dir", "d", "--output_dir", "x", "--p_csv_file", "p.csv"]) == 1
    assert "unknown argument --p_csv_file" in capsys.readouterr().err
    assert "estimate_genome" in cli.COMMANDS.split() and "estimate_genome" in cli._SUBCOMMANDS
