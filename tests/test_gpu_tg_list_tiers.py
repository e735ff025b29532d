"""The forward's candidate lists walked per 64 entries (hyg_tg_set_fine_list_walk):
bit for bit the CPU oracle, and the same launch with the switch off.

The 256-thread forward kernels with their weights in LDS walk a wave's list, in
the step's log-sum-exp and in the gather of the top set, in whole chunks of 256
entries and then the rest in a 128-entry and a 64-entry pass (list_walk in
tg_dev.h) instead of one more whole chunk. Per entry nothing changes and
the sums are exact integer sums, so every output must stay what the oracle
computes. (The two-tier lists these cases were first laid out for were measured
and not kept; the cases cover the walk alike: lists
that end in every kind of rest, lists shorter than one sub-chunk, the initial
step, a top set that is the whole list.)

Cases: the compiled shape K = 6, M = 50, B = 25 at coverage 100 and 1 000
(unbiased-fallback steps, longer lists); a generic shape whose N = M (2K + K^2)
= 120 never exceeds one sort, so the top set is always the whole list and every
wave's list is a single partial sub-chunk; one launch of seven chains of 1 to 300
sites; the forward-only, traced and two-round launches, whose kernels share the
body; and the switch off at 512 and 768 threads, which have no fine walk. The
CPU tests show with the oracle that the lists of each case end in the rests they
are there for, so that no GPU case passes vacuously.
"""
import math

import numpy as np
import pytest

# K, M, B, T, S, coverage, data seed, inference seed
CASES = {
    "c3": (6, 50, 25, 2000, 4, 100.0, 11, 0),
    "c3_cov1000": (6, 50, 25, 2000, 4, 1000.0, 12, 1),
    "whole_list": (3, 8, 4, 600, 3, 60.0, 15, 2),
}
# the mixed-length launch: chains over the "c3" case's sites
MIXED_LENGTHS = [300, 1, 65, 2, 130, 37, 210]
# steps whose lists the CPU test looks at: the chain of the first t sites ends
# with the weights that step t of a longer chain lists
PREFIXES = [1, 2, 3, 5, 9, 17, 33, 65, 129, 257, 400]
NT, LR = 256, 4  # threads and list entries per lane of a whole chunk at 256 threads

_cache = {}


def _case(oracle, name):
    """Data, parameters, emission table and the oracle's chain of a case: computed once, read-only."""
    if name not in _cache:
        from hygeia_amd import synthetic as syn

        K, M, B, T, S, cov, dseed, seed = CASES[name]
        mu, sg = syn.regime_params(K)
        d = syn.simulate(T, S, S, K=K, seed=dseed, coverage=cov, split_frac=0.1)
        p = oracle.make_params(K=K, M=M, B=B, mu=mu, sigma=sg)
        E = oracle.emission(p, d["meth_control"], d["tot_control"], d["meth_case"], d["tot_case"])
        ref = oracle.chain(p, E, seed, 1000 + seed)
        assert ref["status"] == 0
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = {"mu": mu, "sg": sg, "d": d, "p": p, "E": E, "ref": ref, "model": None}
    return _cache[name]


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


def _obs(c):
    d = c["d"]
    return ({"control": d["meth_control"], "case": d["meth_case"]}, {"control": d["tot_control"], "case": d["tot_case"]})


def _mixed_chains():
    chains, site = [], 0
    for i, n in enumerate(MIXED_LENGTHS):
        chains.append((site, n, 5 + i % 2, 900 + i, site))
        site += n
    return chains, site


def _wave_lists(w, M):
    """Lengths of the four waves' lists of a step that lists the weights w: the
    candidates with w - max >= sig_thresh (include/hyg_model.h), candidate n in
    wave (n % 256) / 64."""
    thr = float(np.float32(-(110.0 + math.log(M))))
    n = np.flatnonzero(w - w.max() >= thr)
    return np.bincount((n % NT) // 64, minlength=NT // 64)


def _rests(oracle, name, lengths=PREFIXES):
    """(whole chunks, sub-chunks of the rest) of every wave's list at the steps `lengths`."""
    c = _case(oracle, name)
    M, seed = CASES[name][1], CASES[name][7]
    out = []
    for t in lengths:
        r = oracle.chain(c["p"], c["E"][:t], seed, 1000 + seed)
        for cnt in _wave_lists(r["final_log_weights"], M):
            nsub = (int(cnt) + 63) // 64
            out.append((nsub // LR, nsub % LR))
    return out


def test_compiled_shape_lists_end_in_every_rest(oracle):
    """No GPU: among the steps looked at, lists with whole chunks and with none,
    and rests of 0, 1, 2 and 3 sub-chunks (both, one or neither of the passes)."""
    rests = _rests(oracle, "c3") + _rests(oracle, "c3_cov1000")
    assert {r for _, r in rests} == {0, 1, 2, 3}, sorted(set(rests))
    assert any(f >= 1 for f, _ in rests) and any(f == 0 and r > 0 for f, r in rests)
    assert any(f >= 1 and r > 0 for f, r in rests)  # a whole chunk and a rest behind it


def test_whole_list_shape_fits_one_sort(oracle):
    """No GPU: N = 120 candidates, at most 64 per wave: the top set is always the
    whole list, and a wave's list is one partial sub-chunk (or empty)."""
    K, M = CASES["whole_list"][:2]
    assert M * (2 * K + K * K) == 120
    rests = _rests(oracle, "whole_list", [2, 9, 65, 300])
    assert set(rests) <= {(0, 0), (0, 1)} and (0, 1) in rests


def test_mixed_launch_has_the_first_step_and_short_lists(oracle):
    """No GPU: the launch has chains of one site (no step), two sites (the step
    behind the initial one: K^2 candidates, few of them finite) and longer ones."""
    assert sorted(MIXED_LENGTHS)[:2] == [1, 2] and 65 in MIXED_LENGTHS and max(MIXED_LENGTHS) == 300
    c = _case(oracle, "c3")
    K, M = CASES["c3"][:2]
    first = oracle.chain(c["p"], c["E"][:1], 5, 900)["final_log_weights"]
    lists = _wave_lists(first, M)
    assert 1 <= lists.sum() <= K * K and (lists == 0).any()  # a wave with an empty list beside one with entries


@pytest.fixture
def settings():
    """Pins the width and the list walk for one test; the automatic width and the default walk afterwards."""
    from hygeia_amd import _lib

    L = _lib.load()
    if L.hyg_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")

    def apply(width, fine):
        _lib.check(L.hyg_tg_force_threads(width, width))
        _lib.check(L.hyg_tg_set_fine_list_walk(fine))

    yield apply
    L.hyg_tg_force_threads(0, 0)
    L.hyg_tg_set_fine_list_walk(1)


def _assert_fine_build(model, n_chains):
    """The launch that follows runs the 256-thread forward, the build that has the fine walk
    (a launch of few chains would take 512 threads by itself, and whole chunks with them)."""
    from hygeia_amd import _lib

    assert _lib.load().hyg_tg_threads_per_chain(model.handle, n_chains) == 256


def _assert_chain(res, fw, ex, ref):
    pr = res.particle
    np.testing.assert_array_equal(pr["merged_state"], ref["merged"])
    np.testing.assert_array_equal(pr["control_state"], ref["control"])
    np.testing.assert_array_equal(pr["case_state"], ref["case"])
    np.testing.assert_array_equal(ex["split_probs"], ref["split_probs"])
    np.testing.assert_array_equal(ex["regime_probs"], ref["regime_probs"])
    assert ex["log_z"] == ref["log_z"]
    np.testing.assert_array_equal(fw, ref["final_log_weights"])


@pytest.mark.gpu
@pytest.mark.parametrize("width,fine", [(256, 1), (256, 0), (512, 0), (768, 0)])
@pytest.mark.parametrize("name", list(CASES))
def test_chain_bit_exact(oracle, settings, name, width, fine):
    """On and off at 256 threads, off at 512 and 768: each the oracle's chain, so each the other's."""
    from hygeia_amd import two_group

    c = _case(oracle, name)
    seed = CASES[name][7]
    model = _model(c, name)
    settings(width, fine)
    if width == 256:
        _assert_fine_build(model, 1)
    obs, tot = _obs(c)
    res, fw, ex = two_group.run(obs, tot, model, seed, 1000 + seed)
    _assert_chain(res, fw, ex, c["ref"])


@pytest.mark.gpu
@pytest.mark.parametrize("fine", [1, 0])
def test_mixed_length_launch_bit_exact(oracle, settings, fine):
    """Seven chains of 1 to 300 sites in one launch at 256 threads (the automatic width of so
    few chains is 512, which has no fine walk): each chain's rows are its own oracle run's."""
    from hygeia_amd import two_group

    c = _case(oracle, "c3")
    chains, rows = _mixed_chains()
    settings(256, fine)
    _assert_fine_build(_model(c, "c3"), len(chains))
    obs, tot = _obs(c)
    r = two_group.run_chains_host(obs, tot, _model(c, "c3"), chains, rows, final_weights=True)
    assert (r["status"] == 0).all()
    for i, (s0, n, sd, cid, o0) in enumerate(chains):
        ref = oracle.chain(c["p"], c["E"][s0:s0 + n], sd, cid)
        for k in ("merged", "control", "case", "split_probs", "regime_probs"):
            np.testing.assert_array_equal(r[k][o0:o0 + n], ref[k], err_msg=f"chain {i} {k}")
        assert r["log_z"][i] == ref["log_z"]
        np.testing.assert_array_equal(r["final_w"][i], ref["final_log_weights"])


@pytest.mark.gpu
@pytest.mark.parametrize("trace", [None, "all"])
def test_forward_only_and_traced_launch(oracle, settings, trace):
    """The forward-only and the traced build of the first case: the oracle's log Z
    and final weights, and every array equal with the switch on and off."""
    from hygeia_amd import two_group

    c = _case(oracle, "c3")
    T, seed = CASES["c3"][3], CASES["c3"][7]
    obs, tot = _obs(c)
    got = []
    for fine in (1, 0):
        settings(256, fine)
        _assert_fine_build(_model(c, "c3"), 1)
        kw = {"trace": trace, "n_out_rows": T} if trace else {}
        got.append(two_group.filter_chains_host(obs, tot, _model(c, "c3"), [(0, T, seed, 1000 + seed, 0)],
                                                final_weights=True, **kw))
    on, off = got
    assert on["status"][0] == 0 and on["log_z"][0] == c["ref"]["log_z"]
    np.testing.assert_array_equal(on["final_w"][0], c["ref"]["final_log_weights"])
    assert sorted(on) == sorted(off)
    for k in on:
        assert np.asarray(on[k]).tobytes() == np.asarray(off[k]).tobytes(), k
    if trace:
        assert on["log_z_t"][T - 1] == c["ref"]["log_z"]


@pytest.mark.gpu
def test_two_round_launch(oracle):
    """The resuming build: the ten-chain launch of tests/test_gpu_tg_forward_rounds.py forced into
    two rounds, with the switch on and off: equal byte for byte, and the oracle's."""
    import test_gpu_tg_forward_rounds as fr
    from hygeia_amd import _lib

    L = fr._need_gpu()
    c = fr._case(oracle, "c3")
    models = fr._models("c3", c, 1)
    try:
        _lib.check(L.hyg_tg_set_device_cus(0, fr.CUS))
        _lib.check(L.hyg_tg_set_forward_rounds(2))
        assert fr._two_rounds_planned(L, models[0])
        _assert_fine_build(models[0], len(fr.LENGTHS))  # (two rounds are planned at 256 threads only)
        _lib.check(L.hyg_tg_set_fine_list_walk(1))
        on = fr._launch("c3", c, models)
        _lib.check(L.hyg_tg_set_fine_list_walk(0))
        off = fr._launch("c3", c, models)
    finally:
        L.hyg_tg_set_fine_list_walk(1)
        L.hyg_tg_set_forward_rounds(1)
        L.hyg_tg_set_device_cus(0, 0)
        for m in models:
            m.close()
    fr._assert_same(on, off, "two rounds, fine walk on / off")
    for i, ((s0, n, sd, cid, o0), ref) in enumerate(zip(fr._chains("c3")[0], fr._refs(oracle, "c3"))):
        for k in ("merged", "control", "case", "split_probs", "regime_probs"):
            np.testing.assert_array_equal(on[k][o0:o0 + n], ref[k], err_msg=f"chain {i} {k}")
        assert on["log_z"][i] == ref["log_z"], i
