"""CPU tests of the Monte-Carlo EM layer (hygeia_amd/em.py, hyg_tg_transition_stats'
argument checks): the M-step's closed forms, EM monotonicity of the exact log Z
with an exact E-step (tests/tg_exact_model.py), recovery of the settings from
paths sampled from the prior (tests/em_model.py), rho_case against
ExactModel.rho, and the C ABI / command surface."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import em_model as emm  # noqa: E402
from tg_exact_model import ExactModel  # noqa: E402

from hygeia_amd import _lib, em  # noqa: E402

K, U = 3, 2
MU, SIGMA = [0.15, 0.5, 0.85], [0.08, 0.12, 0.08]
THETA = np.array([0.3, -0.2, 0.1, 0.4, -0.5, 0.2] + [math.log(0.8 / 0.2), math.log(0.7 / 0.3), math.log(0.85 / 0.15)])
TRUTH = dict(omega_case=0.8, merge_log_prob=math.log(0.1), split_prob=0.01)


def _exact(settings, u=U):
    return ExactModel(K, MU, SIGMA, THETA, u=u, omega_case=settings["omega_case"],
                      merge_log_prob=settings["merge_log_prob"], split_prob=settings["split_prob"])


def _exact_rho(ex, d):
    try:
        return ex.rho(1, 0, d)
    except ValueError:  # log1p(-1): the float32 cdf is 1, where the model's rule gives 0.1
        return 0.1


def _stats(n00=0, n01=0, n10=0, n11=0, trials=(), events=(), dcap=8):
    tr, ev = np.zeros(dcap + 1, dtype=np.int64), np.zeros(dcap + 1, dtype=np.int64)
    tr[:len(trials)], ev[:len(events)] = trials, events
    return np.array([[n00, n01], [n10, n11]], dtype=np.int64), tr, ev


# ------------------------------------------------------------------ M-step
def test_m_step_closed_forms():
    cur = dict(omega_case=0.5, merge_log_prob=math.log(0.5), split_prob=0.2)
    # the hazard at d == u is the pmf at 0, (1 - omega)^kappa: with trials at d == u only, the maximiser of
    # e log rho + (n - e) log(1 - rho) has (1 - omega)^2 = e / n
    new, rec = em.m_step(_stats(900, 100, 30, 970, trials=(0, 0, 1000), events=(0, 0, 40)), cur, U, 2.0, em.SETTINGS)
    assert new["split_prob"] == 30 / 1000
    assert new["merge_log_prob"] == math.log(100 / 1000)
    assert abs(new["omega_case"] - (1.0 - math.sqrt(40 / 1000))) < 1e-6
    assert all(rec[n]["updated"] for n in em.SETTINGS)
    assert rec["q_after"] > rec["q_before"]
    assert rec["q_after"] == em.q_omega(*_stats(trials=(0, 0, 1000), events=(0, 0, 40))[1:], new["omega_case"], 2.0, U)
    # a subset
    new, rec = em.m_step(_stats(900, 100, 30, 970, trials=(0, 0, 1000), events=(0, 0, 40)), cur, U, 2.0,
                         ["split_prob"])
    assert new == dict(cur, split_prob=0.03)
    assert rec["omega_case"] == {"updated": False, "reason": "not fitted"} and rec["q_after"] == rec["q_before"]
    with pytest.raises(ValueError):
        em.m_step(_stats(), cur, U, 2.0, ["kappa"])


def test_m_step_degenerate_counts_keep_the_current_value():
    cur = dict(omega_case=0.6, merge_log_prob=math.log(0.3), split_prob=0.2)
    new, rec = em.m_step(_stats(), cur, U, 2.0, em.SETTINGS)  # no trial at all
    assert new == cur
    assert all(not rec[n]["updated"] and rec[n]["reason"] == "no trial" for n in em.SETTINGS)
    # updates that would hit 0 or 1
    new, rec = em.m_step(_stats(50, 0, 0, 70), cur, U, 2.0, em.SETTINGS)
    assert new == cur and "open interval" in rec["split_prob"]["reason"] and \
        "open interval" in rec["merge_log_prob"]["reason"]
    new, rec = em.m_step(_stats(0, 50, 70, 0), cur, U, 2.0, em.SETTINGS)
    assert new == cur and not rec["split_prob"]["updated"] and not rec["merge_log_prob"]["updated"]
    # the hazard never fired: Q grows towards omega = 1, which is outside
    new, rec = em.m_step(_stats(trials=(0, 0, 10, 10), events=(0, 0, 0, 0)), cur, U, 2.0, em.SETTINGS)
    assert new["omega_case"] == 0.6 and "open interval" in rec["omega_case"]["reason"]
    # it always fired at d == u: towards omega = 0
    new, rec = em.m_step(_stats(trials=(0, 0, 10), events=(0, 0, 10)), cur, U, 2.0, em.SETTINGS)
    assert new["omega_case"] == 0.6 and not rec["omega_case"]["updated"]
    # an event below u has probability 0 under every omega: Q is -inf everywhere
    new, rec = em.m_step(_stats(trials=(0, 5, 10), events=(0, 1, 3)), cur, U, 2.0, em.SETTINGS)
    assert new["omega_case"] == 0.6 and rec["q_before"] == -math.inf
    # bins without a trial are skipped, zero counts are dropped before the log: rho = 0 below u costs nothing
    assert math.isfinite(em.q_omega(np.array([7, 7, 5]), np.array([0, 0, 2]), 0.7, 2.0, U))


def test_m_step_never_lowers_q_whatever_the_search_does():
    rng = np.random.default_rng(3)
    for _ in range(20):
        tr = rng.integers(0, 50, 40)
        tr[:U] = 0
        ev = rng.binomial(tr, 0.15)
        cur = dict(omega_case=float(rng.uniform(0.05, 0.95)), merge_log_prob=-1.0, split_prob=0.5)
        new, rec = em.m_step(_stats(trials=tr, events=ev, dcap=39), cur, U, 2.0, ["omega_case"])
        assert rec["q_after"] >= rec["q_before"]
        assert rec["q_after"] == em.q_omega(tr, ev, new["omega_case"], 2.0, U)


# ---------------------------------------------- EM with an exact E-step
def _reads(path, rng, samples=2, cov=12):
    merged, control, case = path
    T = merged.shape[0]
    out = []
    for st in (control, case):
        tot = rng.poisson(cov, size=(T, samples))
        out += [rng.binomial(tot, np.array(MU)[st[:, 0, 1]][:, None]), tot]
    return out  # meth_c, tot_c, meth_k, tot_k


def test_em_with_an_exact_e_step_never_lowers_the_exact_log_z():
    """K = 3, u = 2, 12 sites, two samples per group; the expected statistics
    from the exact pairwise smoothing marginals; five iterations from a wrong
    start. A statistic that misclassifies a branch (a forced change counted as
    a hazard trial, say) is not the complete-data likelihood's and breaks the
    ascent."""
    T, r_ph = 12, 0
    truth = _exact(TRUTH)
    meth_c, tot_c, meth_k, tot_k = _reads(emm.sample_paths(truth, T, 1, 5), np.random.default_rng(6))
    E = truth.emission(meth_c, tot_c, meth_k, tot_k)

    def rho(d, omega, kappa, u):
        ex = ExactModel(K, MU, SIGMA, THETA, u=u, omega_case=omega, kappa=kappa)
        return np.array([_exact_rho(ex, int(x)) for x in d])

    cur = dict(omega_case=0.5, merge_log_prob=math.log(0.5), split_prob=0.2)
    log_z = []
    for _ in range(5):
        lz, _, _, pair = _exact(cur).forward_backward(E, r_ph)
        log_z.append(lz)
        cur, rec = em.m_step(emm.expected_stats(pair, U, T + 1), cur, U, 2.0, em.SETTINGS, rho=rho)
        assert rec["q_after"] >= rec["q_before"]
    log_z.append(_exact(cur).log_z(E, r_ph))
    print(log_z, cur)
    assert log_z[1] > log_z[0] + 1e-3
    assert all(b >= a - 1e-9 for a, b in zip(log_z, log_z[1:]))


def test_a_misclassified_branch_is_seen_by_the_restatement():
    """em_model's classification against ExactModel itself: a transition is a
    hazard trial exactly where the case part's log density moves with
    omega_case, and a table cell exactly where the density moves with the
    merge / split probabilities."""
    a, b = _exact(TRUTH), _exact(dict(TRUTH, omega_case=0.6))
    c = _exact(dict(TRUTH, split_prob=0.3, merge_log_prob=math.log(0.4)))
    merged, control, case = emm.sample_paths(a, 60, 40, 11)
    seen = set()
    for p in range(40):
        for t in range(1, 60):
            x, y = emm.state(merged, control, case, t - 1, p), emm.state(merged, control, case, t, p)
            la, lb, lc = a.log_trans(x, y), b.log_trans(x, y), c.log_trans(x, y)
            assert la > -np.inf  # the sampler's paths are legal
            cell, d, fired = emm.classify(x, y, U)
            assert (d is not None and d >= U) == (la != lb), (x, y)
            assert (cell is not None) == (la != lc), (x, y)
            seen.add((cell, d is not None, fired, a.case_branch(x, y)))
    assert {s[3] for s in seen} == {1, 2, 3, 4} and {s[0] for s in seen} == {None, 0, 1, 2, 3}


# ---------------------------------------------------------------- recovery
def test_settings_recovered_from_paths_of_the_prior():
    """256 legal paths of 2 000 sites from the prior at the truth: each fitted
    setting within 4 standard errors (binomial for the two ratios, from their
    own trial counts; observed information of Q for omega_case)."""
    truth = _exact(TRUTH, u=3)
    merged, control, case = emm.sample_paths(truth, 2000, 256, 17)
    table, trials, events = emm.transition_stats(merged, control, case, [(0, 2000)], 3, 1024)
    start = dict(omega_case=0.5, merge_log_prob=math.log(0.5), split_prob=0.2)
    new, rec = em.m_step((table, trials, events), start, 3, 2.0, em.SETTINGS)
    assert all(rec[n]["updated"] for n in em.SETTINGS)
    for got, want, n in ((new["split_prob"], 0.01, table[1].sum()),
                         (math.exp(new["merge_log_prob"]), 0.1, table[0].sum())):
        se = math.sqrt(got * (1.0 - got) / n)
        print(got, want, se, n)
        assert n > 1000 and abs(got - want) < 4 * se
    w, h = new["omega_case"], 1e-4
    q = lambda v: em.q_omega(trials, events, v, 2.0, 3)  # noqa: E731
    info = -(q(w + h) - 2.0 * q(w) + q(w - h)) / h ** 2
    se = 1.0 / math.sqrt(info)
    print(w, se, int(trials.sum()), int(events.sum()))
    assert info > 0 and se < 0.01 and abs(w - 0.8) < 4 * se


# ------------------------------------------------------------------ hazard
def test_rho_case_against_the_exact_model():
    """d = 0 .. 4096, omega in {0.5, 0.8, 0.95}, u = 3, kappa = 2. ExactModel
    rounds the cdf to float32 and rho_case does not, so the two differ by the
    rounding of the survival: over the rows whose float32 survival is above
    2^-20 the largest relative difference measured is 2.78e-2 (omega = 0.95,
    326 rows; 1.28e-2 at 0.8 over 75 rows, 4.5e-15 at 0.5 over 24 rows; half a
    float32 ulp of the cdf, 2^-25, over a survival just above 2^-20 is 2^-5 =
    3.1e-2 at worst). Asserted: ten times the measured figure. Below u
    both are 0, at d == u both are (1 - omega)^kappa."""
    from scipy import stats

    worst = 0.0
    for omega in (0.5, 0.8, 0.95):
        ex = ExactModel(K, MU, SIGMA, THETA, u=3, omega_case=omega)
        d = np.arange(4097)
        got = em.rho_case(d, omega, 2.0, 3)
        want = np.array([_exact_rho(ex, int(x)) for x in d])
        assert (got[:3] == 0).all() and (want[:3] == 0).all()
        assert abs(got[3] - (1.0 - float(np.float32(omega))) ** 2) < 1e-7
        assert np.isfinite(got).all() and (got[3:] > 0).all() and (got < 1).all()
        surv32 = 1.0 - stats.nbinom(float(np.float32(2.0)), 1.0 - float(np.float32(omega))).cdf(d - 4).astype(np.float32)
        rows = (d >= 3) & ((d == 3) | (surv32 > 2.0 ** -20))
        assert rows.sum() > 20
        # rho_case at the float32 omega the model holds
        got32 = em.rho_case(d, float(np.float32(omega)), 2.0, 3)
        rel = np.abs(got32[rows] - want[rows]) / want[rows]
        print(omega, int(rows.sum()), float(rel.max()))
        worst = max(worst, float(rel.max()))
    assert worst <= 10 * 2.78e-2


def test_rho_case_needs_numpy_alone():
    import subprocess

    code = ("import sys; import hygeia_amd.em as em, numpy as np; "
            "assert em.rho_case(np.arange(6), 0.8, 2.0, 3)[3] > 0; "
            "bad = [m for m in sys.modules if m.split('.')[0] in ('scipy', 'torch', 'oracle', 'tests')]; "
            "assert not bad, bad")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root)


# --------------------------------------------------------------------- ABI
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


DUMMY = 0x1000  # never dereferenced: the checks come before any device work


def _call(lib, **kw):
    a = dict(merged=DUMMY, control=DUMMY, kase=DUMMY, B=5, groups=((0, 10), (10, 20)), block_rows=(0, 40, 10, 50),
             n_seeds=2, n_sites=30, n_groups=None, minimum_duration=3, dcap=1024, stats=DUMMY)
    a.update(kw)
    g = (_lib.DmpGroup * max(len(a["groups"]), 1))(*[_lib.DmpGroup(x, y) for x, y in a["groups"]]) \
        if a["groups"] is not None else None
    br = (C.c_int64 * max(len(a["block_rows"]), 1))(*a["block_rows"]) if a["block_rows"] is not None else None
    n_groups = len(a["groups"]) if a["n_groups"] is None else a["n_groups"]
    return lib.hyg_tg_transition_stats(a["merged"], a["control"], a["kase"], a["B"], g, br, n_groups, a["n_seeds"],
                                       a["n_sites"], a["minimum_duration"], a["dcap"], a["stats"], None)


@pytest.mark.parametrize("kw,word", [
    (dict(merged=None), "null"), (dict(control=None), "null"), (dict(kase=None), "null"), (dict(stats=None), "stats"),
    (dict(dcap=0), "dcap"), (dict(dcap=4097), "dcap"), (dict(dcap=-1), "dcap"),
    (dict(minimum_duration=-1), "minimum_duration"),
    (dict(groups=((10, 20), (0, 10))), "sorted"), (dict(groups=((0, 11), (10, 20))), "disjoint"),
    (dict(groups=((0, 10), (10, 21))), "outside"), (dict(block_rows=(0, 40, -1, 50)), "block row"),
    (dict(groups=None, n_groups=2), "null"), (dict(block_rows=None), "null"), (dict(n_groups=-1), "groups"),
    (dict(B=0), "B"), (dict(n_seeds=0), "n_seeds"), (dict(B=4096, n_seeds=5, block_rows=(0,) * 10), "trajectories"),
    (dict(n_sites=-1), "n_sites"),
])
def test_transition_stats_argument_errors(lib, kw, word):
    assert _call(lib, **kw) == _lib.HYG_EINVAL
    err = lib.hyg_last_error().decode()
    assert err.startswith("hyg_tg_transition_stats:") and word in err


def test_valid_arguments_without_a_device(lib):
    if lib.hyg_device_count() > 0:
        return  # with a device the dummy pointers would be read: tests/test_gpu_em.py covers the entry
    assert _call(lib) == _lib.HYG_EDEVICE
    assert _call(lib, dcap=1) == _lib.HYG_EDEVICE and _call(lib, dcap=4096, minimum_duration=0) == _lib.HYG_EDEVICE


def test_fit_genome_is_a_command_and_parses_its_flags(tmp_path, capsys):
    from hygeia_amd import cli

    assert "fit_genome" in cli.COMMANDS.split() and cli._SUBCOMMANDS["fit_genome"][:2] == ("em", "main")
    assert "hyg_tg_transition_stats" in _lib.EXPORTS and callable(em.main)
    d = {n: v for n, _, v, _ in em.fit_flags()}
    assert d["iterations"] == 10 and d["dcap"] == 1024 and d["fit"] == "omega_case,merge_log_prob,split_prob"
    assert {"batches", "seeds", "chroms", "omega_case", "num_samples_backward"} <= set(d)
    f = cli.parse_flags(["--iterations=3", "--fit", "split_prob", "--dcap", "64", "--batches", "0,2"], em.fit_flags())
    assert f["iterations"] == 3 and f["fit"] == "split_prob" and f["dcap"] == 64 and f["batches"] == "0,2"
    for bad in (["--fit", "kappa"], ["--dcap", "0"], ["--dcap", "5000"], ["--iterations", "0"],
                ["--split_prob", "1.0"], ["--merge_log_prob", "0.0"], ["--num_resampled_particles", "50,60"],
                ["--nosuchflag", "1"]):
        rc = cli.main(["fit_genome", "--results_dir", str(tmp_path / "o"), "--data_dir", str(tmp_path)] + bad)
        assert rc == 1 and "FATAL Flags parsing error" in capsys.readouterr().err
        assert not (tmp_path / "o").exists()
    assert em.serialize_settings(dict(omega_case=0.75, merge_log_prob=-2.5, split_prob=0.02)) == \
        "--omega_case=0.75\n--merge_log_prob=-2.5\n--split_prob=0.02"
