"""The forward's candidate weights in batches of slots (gen_weights<NT, true> in
tg_weights.h): bit for bit the CPU oracle.

The 256-thread forward kernels with their weights in LDS take a wave's proposal
slots in batches: every LDS load of a batch first, then the weights, then the
stores, a slot past the wave's last one clamped and masked. Per weight nothing
changes, so every output must stay what the oracle computes: the trajectories,
the probabilities, log Z and the final weights. The records (the workspace) have
no oracle image; the 512- and 768-thread builds keep the slot-by-slot schedule,
so the workspace of the 256-thread launch must be theirs byte for byte.

Only the shape-specialised 256-thread builds are batched (kBatchedWeights), so
the cases that run the new code are the compiled shape K = 6, M = 50, B = 25 at
256 threads: the single chains at coverage 100 and 1 000, the mixed-length
launch, the forward-only and traced launches, the two-round and multi-model
launches. The generic shapes below run the unchanged slot-by-slot code at every
width: they guard the code that was moved around the new branch, and are the
shapes at which a batched generic build would have to hold (four waves at 256
threads, eight at 512, twelve at 768; I = 2K + K^2 slots):
  K = 2 (I = 8: at 512 threads some waves have two-change-point slots only, at
  768 some have none) with M = 8; K = 3 (I = 15, a ragged last batch) with
  M = 64, every lane an ancestor; K = 5 (I = 35); K = 7 (I = 63); M = 80, the
  one-candidate-per-thread path.
The mixed-length launch has steps with fewer than M ancestors; the forward-only,
traced, two-round and multi-model launches call the same function from other
translation units or from the resume prologue.
The CPU test shows that the cases hold the step kinds they are there for.
"""
import numpy as np
import pytest

# K, M, B, T, S, coverage, data seed, inference seed
CASES = {
    "c3": (6, 50, 25, 600, 4, 100.0, 11, 0),
    "c3_cov1000": (6, 50, 25, 600, 4, 1000.0, 12, 1),
    "k2_m8": (2, 8, 4, 300, 3, 60.0, 21, 2),
    "k3_m64": (3, 64, 8, 300, 3, 60.0, 22, 3),
    "k5": (5, 20, 8, 300, 3, 60.0, 23, 4),
    "k7": (7, 16, 8, 300, 3, 60.0, 24, 5),
    "m80": (4, 80, 8, 300, 3, 60.0, 25, 6),
}
WIDTHS = [256, 512, 768]
MIXED_LENGTHS = [300, 1, 65, 2, 130, 37, 64]
KEEP, OPTIMAL, UNBIASED = 0, 1, 2
OUT = ("merged", "control", "case", "split_probs", "regime_probs")

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
        ref = oracle.chain(p, E, seed, 1000 + seed, want_modes=True)
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


def _kinds(ref):
    return ref["modes"][1:] // 65536  # steps 1 .. T-1 (step 0 is the initial step)


@pytest.mark.parametrize("name", list(CASES))
def test_cases_hold_their_step_kinds(oracle, name):
    """No GPU: every case has optimal and keep-all steps and an optimal step
    directly behind a keep-all or the initial one; coverage 1 000 has unbiased steps."""
    K, M = CASES[name][:2]
    kinds = _kinds(_case(oracle, name)["ref"])
    assert (kinds == OPTIMAL).sum() > 50 and (kinds == KEEP).sum() > 0, np.bincount(kinds, minlength=3)
    before = np.concatenate(([KEEP], kinds[:-1]))
    assert ((kinds == OPTIMAL) & (before == KEEP)).any()
    if name == "c3_cov1000":
        assert (kinds == UNBIASED).sum() > 0, np.bincount(kinds, minlength=3)
    # the slot distributions the shapes are there for (four waves at 256 threads)
    I = 2 * K + K * K
    assert {"k2_m8": I == 8, "k3_m64": I == 15 and M == 64, "k5": I == 35, "k7": I == 63, "m80": M > 64}.get(name, True)


def test_mixed_launch_holds_short_chains(oracle):
    """No GPU: chains of one site (no step), of two (the step behind the initial
    one: K^2 < M ancestors) and longer ones with optimal steps."""
    assert sorted(MIXED_LENGTHS)[:2] == [1, 2] and sum(MIXED_LENGTHS) <= CASES["c3"][3]
    c = _case(oracle, "c3")
    kinds = [_kinds(oracle.chain(c["p"], c["E"][s0:s0 + n], sd, cid, want_modes=True))
             for (s0, n, sd, cid, _) in _mixed_chains()[0]]
    assert sum(1 for k in kinds if (k == OPTIMAL).any()) >= 4 and sum(int((k == KEEP).sum()) for k in kinds) > 0


def _gpu():
    from hygeia_amd import _lib

    L = _lib.load()
    if L.hyg_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")
    return L


@pytest.fixture
def width():
    """Pins the forward / backward width for one test; the automatic width afterwards."""
    from hygeia_amd import _lib

    L = _gpu()

    def apply(w, model=None, n_chains=1):
        _lib.check(L.hyg_tg_force_threads(w, w))
        if w == 256 and model is not None:  # the launch that follows runs the batched build
            assert L.hyg_tg_threads_per_chain(model.handle, n_chains) == 256

    yield apply
    L.hyg_tg_force_threads(0, 0)


def _launch(c, model, chains, n_out, chain_model=None):
    """One device launch with the workspace zeroed first (bytes no chain writes compare equal)."""
    import torch

    from hygeia_amd import two_group

    dev = torch.device("cuda", 0)
    d = c["d"]
    counts = [torch.from_numpy(np.ascontiguousarray(d[k]).view(np.int16)).to(dev) for k in
              ("meth_control", "tot_control", "meth_case", "tot_case")]
    dc = two_group.DeviceChains(model, chains, n_out, device=dev, final_weights=True, chain_model=chain_model)
    for a in (dc.merged, dc.control, dc.case, dc.split_probs, dc.regime_probs, dc.ws):
        a.zero_()
    dc.run(dc.emission(*counts))
    torch.cuda.synchronize()
    got = {k: getattr(dc, k).cpu().numpy() for k in OUT + ("log_z", "final_w", "status")}
    got["workspace"] = dc.ws.cpu().numpy()
    return got


def _assert_chain(got, i, o0, n, ref, what):
    assert got["status"][i] == 0, what
    for k in OUT:
        np.testing.assert_array_equal(got[k][o0:o0 + n], ref[k], err_msg=f"{what} {k}")
    assert got["log_z"][i] == ref["log_z"], what
    np.testing.assert_array_equal(got["final_w"][i], ref["final_log_weights"], err_msg=f"{what} final weights")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_chain_bit_exact_every_width(oracle, width, name):
    """One chain at 256, 512 and 768 threads: each the oracle's, and the records
    of the batched 256-thread build those of the builds that keep the old schedule."""
    c = _case(oracle, name)
    T, seed = CASES[name][3], CASES[name][7]
    model = _model(c, name)
    ws = {}
    for w in WIDTHS:
        width(w, model)
        got = _launch(c, model, [(0, T, seed, 1000 + seed, 0)], T)
        _assert_chain(got, 0, 0, T, c["ref"], f"{name} at {w} threads")
        ws[w] = got["workspace"]
    assert ws[256].tobytes() == ws[512].tobytes() and ws[256].tobytes() == ws[768].tobytes()


@pytest.mark.gpu
def test_mixed_length_launch_bit_exact(oracle, width):
    """Seven chains of 1 to 300 sites in one launch at 256 threads: each chain its
    own oracle run's, and the workspace that of the 512-thread launch."""
    c = _case(oracle, "c3")
    model = _model(c, "c3")
    chains, rows = _mixed_chains()
    ws = {}
    for w in (256, 512):
        width(w, model, len(chains))
        got = _launch(c, model, chains, rows)
        for i, (s0, n, sd, cid, o0) in enumerate(chains):
            _assert_chain(got, i, o0, n, oracle.chain(c["p"], c["E"][s0:s0 + n], sd, cid), f"chain {i} at {w}")
        ws[w] = got["workspace"]
    assert ws[256].tobytes() == ws[512].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("trace", [None, "all"])
@pytest.mark.parametrize("name", ["c3", "k3_m64"])
def test_forward_only_and_traced_launch(oracle, width, name, trace):
    """The forward-only and traced builds at 256 threads: the oracle's log Z and
    final weights, and every array of the launch the 512-thread launch's."""
    from hygeia_amd import two_group

    c = _case(oracle, name)
    T, seed = CASES[name][3], CASES[name][7]
    model = _model(c, name)
    obs, tot = _obs(c)
    kw = {"trace": trace, "n_out_rows": T} if trace else {}
    got = {}
    for w in (256, 512):
        width(w, model)
        got[w] = two_group.filter_chains_host(obs, tot, model, [(0, T, seed, 1000 + seed, 0)], final_weights=True, **kw)
    r = got[256]
    assert r["status"][0] == 0 and r["log_z"][0] == c["ref"]["log_z"]
    np.testing.assert_array_equal(r["final_w"][0], c["ref"]["final_log_weights"])
    if trace:
        assert r["log_z_t"][T - 1] == c["ref"]["log_z"]
    assert sorted(r) == sorted(got[512])
    for k in r:
        assert np.asarray(r[k]).tobytes() == np.asarray(got[512][k]).tobytes(), k


# The ten-chain launch that a pretended 4-CU device cuts into two rounds (the
# lengths and first sites that tests/test_gpu_tg_forward_rounds.py picked for
# the same data: chain 2 is cut at the last legal step, 6 ends in round 1, 8 is
# cut at step 65), over the sites of a longer run of the first case's data.
LONG = (6, 50, 25, 1500, 4, 100.0, 11)
CUS = 4
LENGTHS = [700, 640, 190, 510, 450, 400, 50, 230, 100, 600]
BEGINS = [0, 700, 40, 250, 300, 1000, 5, 565, 1300, 100]


def _long_case(oracle):
    """The data, two thetas (the uniform one moved by N(0, 1) per entry) and their oracle parameters."""
    if "long" not in _cache:
        from hygeia_amd import synthetic as syn
        from hygeia_amd import two_group

        K, M, B, T, S, cov, dseed = LONG
        mu, sg = syn.regime_params(K)
        d = syn.simulate(T, S, S, K=K, seed=dseed, coverage=cov, split_frac=0.1)
        thetas = [two_group.uniform_theta(K, 0.8) + np.random.default_rng(7100 + k).normal(0.0, 1.0, K * K)
                  for k in range(2)]
        params = [oracle.make_params(K=K, M=M, B=B, mu=mu, sigma=sg, theta=th) for th in thetas]
        E = oracle.emission(params[0], d["meth_control"], d["tot_control"], d["meth_case"], d["tot_case"])
        _cache["long"] = {"mu": mu, "sg": sg, "d": d, "thetas": thetas, "params": params, "E": E}
    return _cache["long"]


def _long_chains():
    chains, out = [], 0
    for i, (s0, n) in enumerate(zip(BEGINS, LENGTHS)):
        assert s0 + n <= LONG[3]
        chains.append((s0, n, 3 + i % 3, 700 + i, out))
        out += n
    return chains, out


def _rounds_planned(L, model):
    """Rounds and second-round blocks of the launch that follows, by the launcher's own schedule on this device."""
    import ctypes as C

    n = len(LENGTHS)
    T = np.ascontiguousarray(LENGTHS, dtype=np.int32)
    blocks = np.zeros(2, np.int32)
    order, begin, end = (np.zeros((2, n), np.int32) for _ in range(3))
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rounds = L.hyg_tg_forward_schedule(model.handle, p(T), n, 0, 0, 0, L.hyg_tg_chains_per_cu(model.handle, n), 2,
                                       p(blocks), p(order), p(begin), p(end))
    return rounds, int(blocks[1])


@pytest.mark.gpu
@pytest.mark.parametrize("n_models", [1, 2])
def test_two_round_and_multi_model_launch(oracle, n_models):
    """The resuming build (ten chains forced into two rounds on a pretended 4-CU
    device) and, with two models alternating, the multi-model builds, at 256
    threads: every chain its model's oracle run, and the workspace that of the
    same chains in one launch at 512 threads, which keeps the old schedule."""
    from hygeia_amd import _lib, two_group

    L = _gpu()
    c = _long_case(oracle)
    K, M, B, T = LONG[:4]
    d = c["d"]
    models = two_group.genome_models(c["thetas"][:n_models], c["mu"], c["sg"],
                                     int(max(d["tot_control"].max(), d["tot_case"].max())), [T + 5] * n_models,
                                     num_resampled_ancestors=M, num_samples_backward=B)
    chains, rows = _long_chains()
    order = [i % n_models for i in range(len(chains))] if n_models > 1 else None
    model = models if n_models > 1 else models[0]
    try:
        _lib.check(L.hyg_tg_set_device_cus(0, CUS))
        _lib.check(L.hyg_tg_set_forward_rounds(2))
        assert _rounds_planned(L, models[0]) == (2, 9)
        assert L.hyg_tg_threads_per_chain(models[0].handle, len(chains)) == 256
        got = _launch(c, model, chains, rows, chain_model=order)
        _lib.check(L.hyg_tg_set_forward_rounds(0))
        _lib.check(L.hyg_tg_force_threads(512, 512))
        old = _launch(c, model, chains, rows, chain_model=order)
    finally:
        L.hyg_tg_force_threads(0, 0)
        L.hyg_tg_set_forward_rounds(1)
        L.hyg_tg_set_device_cus(0, 0)
        for m in models:
            m.close()
    for i, (s0, n, sd, cid, o0) in enumerate(chains):
        ref = oracle.chain(c["params"][i % n_models], c["E"][s0:s0 + n], sd, cid)
        _assert_chain(got, i, o0, n, ref, f"chain {i} of {n_models} models")
    assert got["workspace"].tobytes() == old["workspace"].tobytes()
