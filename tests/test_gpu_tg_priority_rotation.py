"""Rotating wave priorities (hyg_tg_set_priority_rotation) change when a wave
issues, never what it computes.

One launch holds 600 copies of one chain: same sites, seed and chain id, each
with its own output rows. 600 workgroups put two or three chains on every CU of
an MI355X, so the copies sit in every wave slot and take every base priority,
and a copy runs through some tens of priority epochs (500 steps of about 13 us
against epochs of 0.33 ms). Every copy must give the oracle's chain, bit for
bit, with rotation on and off; and a launch of chains of mixed lengths, whose
chains end in the middle of an epoch, must too.

Cases as tests/test_gpu_tg_gather_window.py: the compiled shape K = 6, M = 50,
B = 25 at coverage 100 and at coverage 1 000 (unbiased-fallback steps), and one
generic shape; that file's CPU tests show the step kinds these sites hold.
"""
import numpy as np
import pytest

# K, M, B, T, S, coverage, data seed, inference seed
CASES = {
    "c3": (6, 50, 25, 500, 4, 100.0, 11, 0),
    "c3_cov1000": (6, 50, 25, 500, 4, 1000.0, 12, 1),
    "generic": (4, 20, 8, 500, 3, 60.0, 14, 3),
}
COPIES = 600
MIXED_LENGTHS = [500, 37, 1, 300, 250, 2, 210, 499, 64, 65]

_cache = {}


def _case(oracle, name):
    """Data, parameters, emission table, model and the oracle's chain of a case: computed once."""
    if name not in _cache:
        from hygeia_amd import synthetic as syn
        from hygeia_amd import two_group

        K, M, B, T, S, cov, dseed, seed = CASES[name]
        mu, sg = syn.regime_params(K)
        d = syn.simulate(T, S, S, K=K, seed=dseed, coverage=cov, split_frac=0.1)
        p = oracle.make_params(K=K, M=M, B=B, mu=mu, sigma=sg)
        E = oracle.emission(p, d["meth_control"], d["tot_control"], d["meth_case"], d["tot_case"])
        ref = oracle.chain(p, E, seed, 1000 + seed)
        assert ref["status"] == 0
        theta = np.array(p.theta[: p.theta_len])
        model = two_group.CaseControlModel(mu, sg, theta, num_resampled_ancestors=M, num_samples_backward=B,
                                           max_total_reads=int(max(d["tot_control"].max(), d["tot_case"].max())),
                                           max_duration=T + 5)
        _cache[name] = {"d": d, "p": p, "E": E, "ref": ref, "model": model}
    return _cache[name]


@pytest.fixture
def rotation():
    """Sets the switch for one test and restores the default (on) afterwards."""
    from hygeia_amd import _lib

    L = _lib.load()
    if L.hyg_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")

    def apply(on):
        _lib.check(L.hyg_tg_set_priority_rotation(on))

    yield apply
    L.hyg_tg_set_priority_rotation(1)


def _run(c, chains, rows):
    from hygeia_amd import two_group

    d = c["d"]
    r = two_group.run_chains_host({"control": d["meth_control"], "case": d["meth_case"]},
                                  {"control": d["tot_control"], "case": d["tot_case"]}, c["model"], chains, rows,
                                  final_weights=True)
    assert (r["status"] == 0).all()
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("on", [1, 0])
@pytest.mark.parametrize("name", list(CASES))
def test_every_copy_is_the_oracles_chain(oracle, rotation, name, on):
    c = _case(oracle, name)
    ref, T, seed = c["ref"], CASES[name][3], CASES[name][7]
    chains = [(0, T, seed, 1000 + seed, i * T) for i in range(COPIES)]
    rotation(on)
    r = _run(c, chains, COPIES * T)
    for out, want in (("merged", "merged"), ("control", "control"), ("case", "case"),
                      ("split_probs", "split_probs"), ("regime_probs", "regime_probs")):
        got = r[out].reshape((COPIES, T) + r[out].shape[1:])
        np.testing.assert_array_equal(got, np.broadcast_to(ref[want], got.shape), err_msg=out)
    assert (r["log_z"] == ref["log_z"]).all()
    fw = np.asarray(r["final_w"])
    np.testing.assert_array_equal(fw, np.broadcast_to(ref["final_log_weights"], fw.shape))


@pytest.mark.gpu
def test_mixed_lengths_equal_with_and_without_rotation(oracle, rotation):
    """Chains of 1 to 500 sites, 30 of each length: the launch's arrays with
    rotation on equal those with rotation off, and each chain its oracle run."""
    c = _case(oracle, "c3")
    chains, rows = [], 0
    for rep in range(30):
        for i, n in enumerate(MIXED_LENGTHS):
            chains.append(((37 * i) % (500 - n + 1), n, 5 + i % 2, 900 + i, rows))
            rows += n
    rotation(1)
    a = _run(c, chains, rows)
    rotation(0)
    b = _run(c, chains, rows)
    for k in ("merged", "control", "case", "split_probs", "regime_probs", "log_z", "final_w"):
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=k)
    for i, (s0, n, sd, cid, o0) in enumerate(chains[: len(MIXED_LENGTHS)]):
        ref = oracle.chain(c["p"], c["E"][s0:s0 + n], sd, cid)
        np.testing.assert_array_equal(a["merged"][o0:o0 + n], ref["merged"])
        np.testing.assert_array_equal(a["regime_probs"][o0:o0 + n], ref["regime_probs"])
        assert a["log_z"][i] == ref["log_z"]
