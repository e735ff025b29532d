"""The forward's gather window (hyg_tg_set_gather_window): ancestors gathered
ahead by sorted position on the top-set path, bit for bit the CPU oracle.

On a step that resamples through the top set, the waves behind wave 0 compute
the ancestors of the first `window` sorted positions while wave 0 searches the
parents, and the gather copies them. Every output must stay what the oracle
computes, at every workgroup width, with the window off (0), at 8 (with M = 50
parents inside and outside the window share wave 0 on nearly every optimal
step) and at the default; and for a launch of chains of mixed lengths.

The shapes are the smallest at which the paths differ: the compiled shape
K = 6, M = 50, B = 25 (its own kernel builds) at coverage 100 and, shorter, at
coverage 1 000 (unbiased-fallback steps), and one generic shape. The CPU test
below shows, from the oracle's step modes, that each case holds the step kinds
it is there for, so that no GPU case passes vacuously.
"""
import numpy as np
import pytest

# K, M, B, T, S, coverage, data seed, inference seed (test_gpu_two_group.CASES 0, 1, 3)
CASES = {
    "c3": (6, 50, 25, 1500, 4, 100.0, 11, 0),
    "c3_cov1000": (6, 50, 25, 800, 4, 1000.0, 12, 1),
    "generic": (4, 20, 8, 700, 3, 60.0, 14, 3),
}
WIDTHS = [256, 512, 768]
WINDOWS = [0, 8, -1]  # off, hits and misses in one wave, the default
# the mixed-length launch: chains over the "c3" case's sites
MIXED_LENGTHS = [700, 37, 1, 300, 250, 2, 210]
KEEP, OPTIMAL, UNBIASED = 0, 1, 2

_cache = {}


def _case(oracle, name):
    """Data, parameters, emission table and the oracle's chain of a case: computed once."""
    if name not in _cache:
        from hygeia_amd import synthetic as syn

        K, M, B, T, S, cov, dseed, seed = CASES[name]
        mu, sg = syn.regime_params(K)
        d = syn.simulate(T, S, S, K=K, seed=dseed, coverage=cov, split_frac=0.1)
        p = oracle.make_params(K=K, M=M, B=B, mu=mu, sigma=sg)
        E = oracle.emission(p, d["meth_control"], d["tot_control"], d["meth_case"], d["tot_case"])
        ref = oracle.chain(p, E, seed, 1000 + seed, want_modes=True)
        assert ref["status"] == 0
        _cache[name] = {"mu": mu, "sg": sg, "d": d, "p": p, "E": E, "ref": ref, "model": None}
    return _cache[name]


def _mixed_chains():
    chains, site = [], 0
    for i, n in enumerate(MIXED_LENGTHS):
        chains.append((site, n, 5 + i % 2, 900 + i, site))
        site += n
    return chains, site


def _kinds(ref):
    """Step kinds of steps 1 .. T-1 (step 0 is the initial step)."""
    return ref["modes"][1:] // 65536


def _keep_or_init_then_optimal(kinds):
    if len(kinds) == 0:
        return False
    before = np.concatenate(([KEEP], kinds[:-1]))  # step 1 follows the initial step
    return bool(((kinds == OPTIMAL) & (before == KEEP)).any())


@pytest.mark.parametrize("name", list(CASES))
def test_cases_hold_their_step_kinds(oracle, name):
    """No GPU: each case has optimal and keep-all steps, an optimal step directly
    behind a keep-all or the initial one, and (coverage 1 000) unbiased steps."""
    kinds = _kinds(_case(oracle, name)["ref"])
    assert (kinds == OPTIMAL).sum() > 100 and (kinds == KEEP).sum() > 0, np.bincount(kinds, minlength=3)
    assert _keep_or_init_then_optimal(kinds)
    if name == "c3_cov1000":
        assert (kinds == UNBIASED).sum() > 0, np.bincount(kinds, minlength=3)


def test_mixed_launch_holds_its_step_kinds(oracle):
    """No GPU: the chains of the mixed-length launch have optimal steps and
    keep-all steps, and one of them an optimal step behind a keep-all one."""
    c = _case(oracle, "c3")
    chains, _ = _mixed_chains()
    kinds = [_kinds(oracle.chain(c["p"], c["E"][s0:s0 + n], sd, cid, want_modes=True))
             for (s0, n, sd, cid, _) in chains]
    assert sum(int((k == OPTIMAL).sum()) for k in kinds) > 100
    assert sum(int((k == KEEP).sum()) for k in kinds) > 0
    assert any(_keep_or_init_then_optimal(k) for k in kinds)
    assert sum(1 for k in kinds if (k == OPTIMAL).any()) >= 4  # chains that end at different steps


def test_gather_window_range():
    """No GPU: the entry takes 0 (off) to 256 (the largest top set) and -1 (the default)."""
    from hygeia_amd import _lib

    L = _lib.load()
    try:
        assert [L.hyg_tg_set_gather_window(w) for w in (0, 8, 256, -1)] == [0, 0, 0, 0]
        assert L.hyg_tg_set_gather_window(257) < 0 and L.hyg_tg_set_gather_window(-2) < 0
    finally:
        L.hyg_tg_set_gather_window(-1)


@pytest.fixture
def launch_settings():
    """Pins the forward / backward width and the gather window for one test and
    restores the automatic width and the default window afterwards."""
    from hygeia_amd import _lib

    L = _lib.load()
    if L.hyg_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")

    def apply(width, window):
        _lib.check(L.hyg_tg_force_threads(width, width))
        _lib.check(L.hyg_tg_set_gather_window(window))

    yield apply
    L.hyg_tg_force_threads(0, 0)
    L.hyg_tg_set_gather_window(-1)


def _model(c, name):
    if c["model"] is None:
        from hygeia_amd import two_group

        K, M, B, T = CASES[name][:4]
        d = c["d"]
        theta = np.array(c["p"].theta[: c["p"].theta_len])
        c["model"] = two_group.CaseControlModel(c["mu"], c["sg"], theta, num_resampled_ancestors=M,
                                                num_samples_backward=B,
                                                max_total_reads=int(max(d["tot_control"].max(), d["tot_case"].max())),
                                                max_duration=T + 5)
    return c["model"]


@pytest.mark.gpu
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("name", list(CASES))
def test_chain_bit_exact_every_window(oracle, launch_settings, name, width, window):
    from hygeia_amd import two_group

    c = _case(oracle, name)
    d, ref = c["d"], c["ref"]
    seed = CASES[name][7]
    model = _model(c, name)
    launch_settings(width, window)
    res, fw, ex = two_group.run({"control": d["meth_control"], "case": d["meth_case"]},
                                {"control": d["tot_control"], "case": d["tot_case"]}, model, seed, 1000 + seed)
    pr = res.particle
    np.testing.assert_array_equal(pr["merged_state"], ref["merged"])
    np.testing.assert_array_equal(pr["control_state"], ref["control"])
    np.testing.assert_array_equal(pr["case_state"], ref["case"])
    np.testing.assert_array_equal(ex["split_probs"], ref["split_probs"])
    np.testing.assert_array_equal(ex["regime_probs"], ref["regime_probs"])
    assert ex["log_z"] == ref["log_z"]
    np.testing.assert_array_equal(fw, ref["final_log_weights"])


@pytest.mark.gpu
def test_mixed_length_launch_bit_exact(oracle, launch_settings):
    """Seven chains of 1 to 700 sites in one launch (run_chains_host), automatic
    width and default window: each chain's rows are its own oracle run's."""
    from hygeia_amd import two_group

    c = _case(oracle, "c3")
    d = c["d"]
    chains, rows = _mixed_chains()
    launch_settings(0, -1)
    r = two_group.run_chains_host({"control": d["meth_control"], "case": d["meth_case"]},
                                  {"control": d["tot_control"], "case": d["tot_case"]}, _model(c, "c3"), chains,
                                  rows, final_weights=True)
    assert (r["status"] == 0).all()
    for i, (s0, n, sd, cid, o0) in enumerate(chains):
        ref = oracle.chain(c["p"], c["E"][s0:s0 + n], sd, cid)
        np.testing.assert_array_equal(r["merged"][o0:o0 + n], ref["merged"])
        np.testing.assert_array_equal(r["control"][o0:o0 + n], ref["control"])
        np.testing.assert_array_equal(r["case"][o0:o0 + n], ref["case"])
        np.testing.assert_array_equal(r["split_probs"][o0:o0 + n], ref["split_probs"])
        np.testing.assert_array_equal(r["regime_probs"][o0:o0 + n], ref["regime_probs"])
        assert r["log_z"][i] == ref["log_z"]
        np.testing.assert_array_equal(r["final_w"][i], ref["final_log_weights"])
