"""Joint segmentations of the single-group path, everything that needs no GPU:
the reference of the backward simulation (tests/sg_sample_ref.py) against the
exact posterior and against tests/sg_filter_ref.py, the structure of its paths
under resampling, the refusals of the three new entries that are raised before
a device is looked for, and `hygeia sg_sample_genome` on a faked engine.
"""
import ctypes as C
import os

import numpy as np
import pytest

from hygeia_amd import _lib, changepoints, cli, single_group
from tests import sg_filter_ref as fref
from tests import sg_sample_ref as sr
from tests.test_sg_multi_cpu import _Models, _params, _run_args, _write_chrom

NEW = ("hyg_sg_history_chains_multi", "hyg_sg_sample_paths_multi", "hyg_sg_sample_chains_host_multi")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ------------------------------------------------------------ the reference
@pytest.mark.parametrize("K,u,T", [(3, 2, 40), (2, 1, 48)])
def test_reference_samples_the_exact_posterior(K, u, T):
    """1. While N_prev + K <= N_max at every step the sets enumerate every
    reachable state and the draws are exact: the frequencies of r_t = r and of
    "a segment starts at t" over B = 1024 draws against the exact smoothing
    marginals (a plain forward-backward over (d, r) in numpy). Per cell with
    exact probability p in (0.02, 0.98), z = (f - p) / sqrt(p (1 - p) / B) must
    have |z| < 5 (two-sided 6e-7 per cell), over at least 40 regime cells.
    Measured (CPU): K = 3: 94 regime cells, max |z| 1.39, 11 start cells, max
    |z| 1.45; K = 2: 48 regime cells, max |z| 2.07, 10 start cells, max |z| 3.12."""
    Nmax, B, seed = 250, 1024, 5
    assert K * T <= Nmax
    p, _, _, E = sr.synthetic_case(K, u, Nmax, T)
    tb = fref.Tables(p, T)
    h = sr.history(p, E, seed, 0, tables=tb)
    assert h["status"] == 0 and [len(s[0]) for s in h["sets"]] == [K * (t + 1) for t in range(T)]
    paths, status = sr.sample(h["sets"], tb, T, B, seed, 0)
    assert status == 0
    regime, start = sr.exact_marginals(tb, E)
    assert np.allclose(regime.sum(axis=1), 1.0, atol=1e-9)

    def worst(freq, prob):
        use = (prob > 0.02) & (prob < 0.98)
        z = (freq[use] - prob[use]) / np.sqrt(prob[use] * (1 - prob[use]) / B)
        return int(use.sum()), float(np.abs(z).max())

    fr = np.stack([(paths[:, :, 1] == r).mean(axis=1) for r in range(K)], axis=1)
    n_reg, z_reg = worst(fr, regime)
    n_st, z_st = worst((paths[:, :, 0] == 1).mean(axis=1), start)
    print(f"K={K}: {n_reg} regime cells, max |z| {z_reg:.2f}; {n_st} start cells, max |z| {z_st:.2f}")
    assert n_reg >= 40 and n_st >= 1
    assert z_reg < 5 and z_st < 5


def test_structure_under_resampling():
    """2. K = 3, u = 2, N_max = 12, T = 90, B = 64: every path starts with d = 1
    at site 0; d is the previous d + 1 with r unchanged, or 1 with another r;
    at a change the previous state had d >= u."""
    K, u, Nmax, T, B = 3, 2, 12, 90, 64
    p, _, _, E = sr.synthetic_case(K, u, Nmax, T)
    tb = fref.Tables(p, T)
    h = sr.history(p, E, 5, 0, tables=tb)
    assert h["status"] == 0 and len(h["sets"][-1][0]) == Nmax
    paths, status = sr.sample(h["sets"], tb, T, B, 5, 0)
    assert status == 0
    d, r = paths[:, :, 0].astype(int), paths[:, :, 1].astype(int)
    assert np.all(d[0] == 1) and np.all((r >= 0) & (r < K))
    cont = (d[1:] == d[:-1] + 1) & (r[1:] == r[:-1])
    change = (d[1:] == 1) & (r[1:] != r[:-1]) & (d[:-1] >= u)
    assert np.all(cont ^ change)
    assert change.any() and len({paths[:, b].tobytes() for b in range(B)}) >= 10


@pytest.mark.parametrize("K,u,Nmax,T", [(3, 2, 12, 40), (2, 1, 250, 20), (16, 1, 250, 17)])
def test_history_is_the_forward_of_every_prefix(K, u, Nmax, T):
    """`history` restates the forward in one pass: the set of step t is the
    final set of the chain cut after t (the draws are keyed by t), log Z_t its log Z."""
    p, _, _, E = sr.synthetic_case(K, u, Nmax, T)
    h = sr.history(p, E, 5, 3)
    for t in range(T):
        f = fref.forward(p, E[:t + 1], 5, 3, marginals=False)
        lw, st = h["sets"][t]
        assert f["status"] == 0 and np.array_equal(f["log_weights"], np.array(lw)), t
        assert np.array_equal(f["states"], np.array(st, np.int32).reshape(-1, 2)), t
        assert f["log_z"] == h["log_z_t"][t], t
    assert h["log_z"] == h["log_z_t"][-1]


def test_history_stops_at_the_enumeric_site():
    from tests.test_sg_filter_cpu import enumeric_case

    p, E = enumeric_case()
    h = sr.history(p, E[:20], 3, 1)
    assert h["status"] == -2 and h["t_stop"] == 6 and all(len(s[0]) == 0 for s in h["sets"][6:])
    assert sr.history_arrays(h, 9)[2].tolist() == [2, 4, 6, 8, 9, 9] + [0] * 14


def test_sample_guards():
    """a row without a finite logit and a sojourn longer than the sites before it: -1 below, HYG_ENUMERIC"""
    p, _, _, _ = sr.synthetic_case(2, 1, 3, 6)
    tb = fref.Tables(p, 6)
    sets = [([0.0], [(t + 1, 0)]) for t in range(6)]
    paths, st = sr.sample(sets, tb, 6, 2, 1, 0)
    assert st == 0 and paths[:, 0, 0].tolist() == [1, 2, 3, 4, 5, 6]
    sets[5] = ([0.0], [(9, 0)])
    paths, st = sr.sample(sets, tb, 6, 2, 1, 0)
    assert st == -2 and np.all(paths == -1)
    sets[5] = ([0.0], [(2, 0)])
    sets[3] = ([float("-inf")], [(4, 1)])
    paths, st = sr.sample(sets, tb, 6, 2, 1, 0)
    assert st == -2 and np.all(paths[:4] == -1) and paths[4:, 1].tolist() == [[1, 0], [2, 0]]


# ------------------------------------------------------------ C ABI, no device
def _calls(lib, models, n_models, ch, cm, n, buf, st, z, hist="full", B=25, rows=None, wsb=1 << 30, which=range(3)):
    """Return codes of the three entries (0: history, 1: sampler, 2: host form).
    The pointers are host memory, which no check reads but a launch would."""
    p, zs, sp = (a.ctypes.data_as(C.c_void_p) for a in (buf, z, st))
    h = {"full": _lib.SgHistory(p, p, p), "part": _lib.SgHistory(p, None, p), "null": None}[hist]
    hp = C.byref(h) if h is not None else None
    total = buf.shape[0]
    rows = total if rows is None else rows
    calls = [
        lambda: lib.hyg_sg_history_chains_multi(models, n_models, ch, cm, n, p, p, wsb, hp, p, None, None, None, sp,
                                                None),
        lambda: lib.hyg_sg_sample_paths_multi(models, n_models, ch, cm, n, hp, None, B, p, None, None),
        lambda: lib.hyg_sg_sample_chains_host_multi(models, n_models, zs, zs, 2, total, ch, cm, n, B, rows, p, p, sp),
    ]
    return [calls[i]() for i in which]


def test_new_entries_are_exported_and_the_command_is_registered(lib):
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert "sg_sample_genome" in cli.COMMANDS.split()
    assert cli._SUBCOMMANDS["sg_sample_genome"] == ("single_group", "sg_sample_genome", "Error: ")
    assert callable(single_group.sg_sample_genome) and callable(single_group.sample_many)


def test_refusals_before_any_device(lib):
    ch, buf, st, z = _run_args()
    E = _lib.HYG_EINVAL
    with _Models(lib, [(_params(), 100, 500), (_params(theta_shift=0.1), 100, 500)]) as m:
        cm = (C.c_int32 * 2)(0, 1)
        for bad in ((0, 2), (-1, 0)):  # a model index out of range
            assert _calls(lib, m.arr, 2, ch, (C.c_int32 * 2)(*bad), 2, buf, st, z) == [E] * 3
            assert b"chain_model[" in lib.hyg_last_error()
        # a NULL history, or one with a NULL array
        for hist in ("null", "part"):
            assert _calls(lib, m.arr, 2, ch, cm, 2, buf, st, z, hist=hist, which=[0, 1]) == [E] * 2, hist
            assert b"null history" in lib.hyg_last_error()
        # n_trajectories outside [1, 1024]
        for B in (0, -3, 1025):
            assert _calls(lib, m.arr, 2, ch, cm, 2, buf, st, z, B=B, which=[1, 2]) == [E] * 2, B
            assert b"n_trajectories" in lib.hyg_last_error()
        # a workspace that is too small
        need = lib.hyg_sg_filter_workspace_bytes_multi(m.arr, 2, 2)
        assert _calls(lib, m.arr, 2, ch, cm, 2, buf, st, z, wsb=need - 1, which=[0]) == [E]
        assert b"workspace too small" in lib.hyg_last_error()
        # the host form: an out_begin range outside out_rows, or before it
        total = buf.shape[0]
        for ob, rows in ((-1, total), (total - ch[1].n_sites + 1, total), (ch[1].out_begin, total - 1)):
            ch2 = (_lib.SgChain * 2)(ch[0], ch[1])
            ch2[1].out_begin = ob
            assert _calls(lib, m.arr, 2, ch2, cm, 2, buf, st, z, rows=rows, which=[2]) == [E]
            assert b"output rows" in lib.hyg_last_error()
        # a negative out_begin on the device entries, no chains array, no models
        ch2 = (_lib.SgChain * 2)(ch[0], ch[1])
        ch2[0].out_begin = -1
        assert _calls(lib, m.arr, 2, ch2, cm, 2, buf, st, z, which=[0, 1]) == [E] * 2
        assert _calls(lib, m.arr, 2, None, cm, 2, buf, st, z) == [E] * 3
        assert _calls(lib, None, 2, ch, cm, 2, buf, st, z) == [E] * 3
        assert _calls(lib, m.arr, 0, ch, cm, 2, buf, st, z) == [E] * 3
    with _Models(lib, [(_params(), 100, 500), (_params(theta_shift=0.1), 100, 15)]) as m:  # a chain too long
        assert _calls(lib, m.arr, 2, ch, (C.c_int32 * 2)(0, 1), 2, buf, st, z) == [E] * 3
        assert b"max_duration" in lib.hyg_last_error()
    with _Models(lib, [(_params(), 100, 500), (_params(u=2), 100, 500)]) as m:  # incompatible models
        assert _calls(lib, m.arr, 2, ch, (C.c_int32 * 2)(0, 1), 2, buf, st, z) == [E] * 3
        assert b"minimum_duration" in lib.hyg_last_error()


def test_entries_refuse_without_device(lib):
    if lib.hyg_device_count() > 0:
        pytest.skip("host without a GPU only")
    ch, buf, st, z = _run_args()
    with _Models(lib, [(_params(), 100, 500), (_params(theta_shift=0.1), 100, 500)]) as m:
        assert _calls(lib, m.arr, 2, ch, (C.c_int32 * 2)(1, 0), 2, buf, st, z) == [_lib.HYG_EDEVICE] * 3
        assert b"no CPU fallback" in lib.hyg_last_error()
        assert _calls(lib, m.arr, 1, ch, (C.c_int32 * 2)(0, 0), 2, buf, st, z) == [_lib.HYG_EDEVICE] * 3  # n_models = 1


# ------------------------------------------------------------ sg_sample_genome
@pytest.fixture
def fake_sampler(monkeypatch):
    """sample_many replaced by a recorder whose paths encode the task"""
    calls = []

    def fake(L, K, u, alpha, beta, n_particles, tasks, n_trajectories, is_kappa_fixed=True):
        calls.append(dict(K=K, u=u, tasks=tasks, B=n_trajectories, n_particles=n_particles, fixed=is_kappa_fixed))
        out = []
        for t in tasks:
            T = t["tot"].shape[0]
            paths = np.empty((T, n_trajectories, 2), np.int16)
            paths[:, :, 0] = (np.arange(T)[:, None] + 1) % 7 + 1
            paths[:, :, 1] = (np.arange(n_trajectories)[None, :] + t["seed"] % K) % K
            out.append({"paths": paths, "log_z": -float(T) - 0.5 * (t["seed"] % 1000), "status": 0})
        return out

    monkeypatch.setattr(single_group, "sample_many", fake)
    monkeypatch.setattr(_lib, "load", lambda import_torch=True: object())
    monkeypatch.setattr(cli, "_use_task_device", lambda L: None)
    return calls


def _tsv(path):
    lines = open(path).read().splitlines()
    return lines[0].split("\t"), [ln.split("\t") for ln in lines[1:]]


def test_sg_sample_genome_files_and_grouping(tmp_path, fake_sampler):
    data, out, agg = tmp_path / "data", tmp_path / "out", tmp_path / "agg"
    data.mkdir()
    sizes = {"3": 21, "4": 41, "9": 31}
    for i, (chrom, rows) in enumerate(sizes.items()):
        _write_chrom(str(data), chrom, rows, seed=10 + i)
    # histories: 2 seeds x (12 x 100 + 4) bytes x (20, 40, 30) sites; the budget holds 40 + 20 sites
    gib = 2 * single_group.history_bytes(60, 100) / 2 ** 30
    rc = cli.main(["sg_sample_genome", "--data_dir", str(data), "--output_dir", str(out), "--aggregate_dir", str(agg),
                   "--seeds", "1,-73", "--n_particles", "100", "--n_trajectories", "4", "--history_gib", repr(gib)])
    assert rc == 0
    # longest first, first fit: (4, 3) then (9); every seed of a chromosome in its launch, chain id 0
    assert [[t["tot"].shape[0] for t in c["tasks"]] for c in fake_sampler] == [[40, 40, 20, 20], [30, 30]]
    assert all(c["B"] == 4 and c["n_particles"] == 100 and c["u"] == 2 for c in fake_sampler)
    tasks = fake_sampler[0]["tasks"]
    assert [t["seed"] for t in tasks[:2]] == [1, (-73) & (2 ** 64 - 1)] and all(t["chain_id"] == 0 for t in tasks)
    assert tasks[0]["tot"] is tasks[1]["tot"]
    assert sorted(os.listdir(out)) == ["sg_paths_3.npz", "sg_paths_4.npz", "sg_paths_9.npz", "sg_sample.tsv"]
    head, rows = _tsv(out / "sg_sample.tsv")
    assert head == ["chrom", "seed", "n_sites", "log_z", "status"]
    assert [r[:3] for r in rows] == [[c, s, str(n - 1)] for c, n in sizes.items() for s in ("1", "-73")]
    assert all(r[4] == "HYG_OK" for r in rows) and float(rows[0][3]) == -20.5
    z = np.load(out / "sg_paths_4.npz")
    assert sorted(z.files) == ["durations", "positions", "regimes"]
    assert z["regimes"].shape == (40, 8) and z["regimes"].dtype == np.int8 and z["durations"].dtype == np.int16
    # trajectory p = seed index x B + b
    s2 = ((-73) & (2 ** 64 - 1)) % 6
    assert z["regimes"][0].tolist() == [(b + 1) % 6 for b in range(4)] + [(b + s2) % 6 for b in range(4)]
    # the aggregate matrices, read back by get_change_points' reader
    assert sorted(os.listdir(agg)) == sorted(f"{stem}_chrom_{c}.csv.gz" for c in sizes for stem in (
        "control_regimes", "case_regimes", "control_durations", "case_durations", "merge_states"))
    for group in ("control", "case"):
        pos, reg = changepoints._matrix(str(agg), f"{group}_regimes", "4")
        assert np.array_equal(pos, z["positions"].astype(np.int64)) and np.array_equal(reg, z["regimes"])
        assert np.array_equal(changepoints._matrix(str(agg), f"{group}_durations", "4")[1], z["durations"])
    assert np.all(changepoints._matrix(str(agg), "merge_states", "4")[1] == 1)


def test_aggregate_matrices_keep_wrapped_durations(tmp_path):
    """a synthetic paths array with durations beyond 2^15 (stored modulo 2^16): equal values after the round trip"""
    T, P = 9, 5
    pos = np.arange(T) * 17 + 3
    dur = ((np.arange(T)[:, None] * 9000 + np.arange(P)[None, :]) & 0xFFFF).astype(np.uint16).view(np.int16)
    reg = ((np.arange(T)[:, None] + np.arange(P)[None, :]) % 6).astype(np.int8)
    assert (dur < 0).any()
    single_group.write_aggregate_matrices(str(tmp_path), "X", pos, reg, dur)
    p2, r2 = changepoints._matrix(str(tmp_path), "case_regimes", "X")
    assert np.array_equal(p2, pos) and np.array_equal(r2, reg)
    assert np.array_equal(changepoints._matrix(str(tmp_path), "control_durations", "X")[1], dur)


def test_history_groups_and_the_refusal():
    hb = single_group.history_bytes
    assert hb(1, 250) == 3004 and hb(10, 12) == 1480
    lens = [50, 90, 10, 90, 40]
    g = single_group.history_groups(lens, 1, 250, hb(100, 250))
    assert g == [[1, 2], [3], [0, 4]]  # longest first, first fit; a group never exceeds the budget
    assert single_group.history_groups(lens, 1, 250, hb(10 ** 6, 250)) == [[1, 3, 0, 4, 2]]
    assert single_group.history_groups(lens, 3, 250, 3 * hb(90, 250)) == [[1], [3], [0, 4], [2]]
    with pytest.raises(single_group.GenomeError) as e:
        single_group.history_groups(lens, 2, 250, 2 * hb(90, 250) - 1, names=["a", "b", "c", "d", "e"])
    assert "chromosome b" in str(e.value) and str(2 * hb(90, 250)) in str(e.value) and \
        str(2 * hb(90, 250) - 1) in str(e.value)


def test_sg_sample_genome_refuses_a_chromosome_beyond_the_budget(tmp_path, fake_sampler, capsys):
    data, out = tmp_path / "data", tmp_path / "out"
    data.mkdir()
    _write_chrom(str(data), "3", 21, seed=1)
    _write_chrom(str(data), "4", 41, seed=2)
    gib = single_group.history_bytes(39, 250) / 2 ** 30
    rc = cli.main(["sg_sample_genome", "--data_dir", str(data), "--output_dir", str(out), "--history_gib", repr(gib)])
    err = capsys.readouterr().err
    assert rc == 1 and "chromosome 4" in err and str(single_group.history_bytes(40, 250)) in err
    assert not fake_sampler and not out.exists()


@pytest.mark.parametrize("argv,needle", [
    (["--output_dir", "o"], "--data_dir is required"),
    (["--data_dir", "d"], "--output_dir is required"),
    (["--data_dir", "d", "--output_dir", "o", "--u", "3,5"], "invalid value for --u"),
    (["--data_dir", "d", "--output_dir", "o", "--u", "0"], "positive"),
    (["--data_dir", "d", "--output_dir", "o", "--seeds", "1,1"], "distinct"),
    (["--data_dir", "d", "--output_dir", "o", "--parameters_dir", "a,b"], "one directory"),
    (["--data_dir", "d", "--output_dir", "o", "--n_trajectories", "0"], "n_trajectories"),
    (["--data_dir", "d", "--output_dir", "o", "--n_trajectories", "1025"], "n_trajectories"),
    (["--data_dir", "d", "--output_dir", "o", "--history_gib", "0"], "history_gib"),
    (["--data_dir", "d", "--output_dir", "o", "--trace"], "unknown argument --trace"),
])
def test_sg_sample_genome_flag_errors(capsys, argv, needle):
    assert cli.main(["sg_sample_genome"] + argv) == 1
    err = capsys.readouterr().err
    assert err.startswith("Error: ") and needle in err, err


def test_sg_sample_genome_reads_everything_before_writing(tmp_path, fake_sampler, capsys):
    data, out, agg = tmp_path / "data", tmp_path / "out", tmp_path / "agg"
    data.mkdir()
    _write_chrom(str(data), "3", 20, seed=0)
    _write_chrom(str(data), "5", 12, seed=4, bad_meth=True)
    rc = cli.main(["sg_sample_genome", "--data_dir", str(data), "--output_dir", str(out), "--aggregate_dir", str(agg)])
    assert rc == 1 and "chromosome 5" in capsys.readouterr().err
    assert not fake_sampler and not out.exists() and not agg.exists()
    assert cli.main(["sg_sample_genome", "--data_dir", str(data), "--output_dir", str(out), "--chroms", "3,3"]) == 1


def test_sample_many_checks_n_trajectories():
    for B in (0, 1025):
        with pytest.raises(ValueError):
            single_group.sample_many(None, 6, 2, None, None, 250, [], B)
