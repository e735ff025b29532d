"""The forward in two rounds (hyg_tg_set_forward_rounds) computes what the one
launch computes, bit for bit.

Round 1 runs every chain to a cut of its own, round 2 resumes every chain from
its last history record in the resuming build of the forward kernel, in another
block order. Rounds are forced on a pretended 4-CU device, so that launches of
10 chains of 50 to 700 sites mix CUs of three and two chains. Every launch is
compared with the same launch at hyg_tg_set_forward_rounds(0): status, log Z,
final weights, the five output arrays and every byte of the workspace (the
history records). One launch is also compared with the CPU oracle. The last
test runs launches in which chains end in HYG_ENUMERIC in either round.

The chains (CHAINS) hold, besides ordinary ones: a chain shorter than the
earliest cut, which ends in round 1 and is absent from round 2; a chain cut at
the smallest legal step, 65; and one cut at the last legal step below its
length. The CPU test below shows with the oracle's step modes that across a
case's chains the record a chain resumes from is at least once that of an
optimal step, of a keep-all step and (coverage 1 000) of an unbiased step.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cli_trees import _theta  # noqa: E402

# K, M, B, sites, samples, coverage, data seed (test_gpu_tg_gather_window.CASES)
CASES = {
    "c3": (6, 50, 25, 1500, 4, 100.0, 11),
    "c3_cov1000": (6, 50, 25, 800, 4, 1000.0, 12),
    "generic": (4, 20, 8, 700, 3, 60.0, 14),
}
CUS = 4
# Ten chains: blocks 0, 1, 4, 5, 8, 9 sit on the three-chain CUs of round 1
# (b % 4 < 2), the others on two-chain CUs. By index: 2 is cut at the last
# legal step below its length (129 of 190), 6 ends in round 1, 8 is cut at 65.
LENGTHS = [700, 640, 190, 510, 450, 400, 50, 230, 100, 600]
# first site of each chain, per case (picked with the oracle, see the CPU test)
BEGINS = {
    "c3": [0, 700, 40, 250, 300, 1000, 5, 565, 1300, 100],
    "c3_cov1000": [0, 140, 565, 280, 300, 350, 5, 500, 600, 150],
    "generic": [0, 10, 40, 100, 200, 300, 5, 400, 600, 100],
}
KEEP, OPTIMAL, UNBIASED = 0, 1, 2
NAMES = ("merged", "control", "case", "split_probs", "regime_probs", "log_z", "final_w", "status")

_cache = {}


def _chains(name):
    chains, out = [], 0
    for i, (s0, n) in enumerate(zip(BEGINS[name], LENGTHS)):
        assert s0 + n <= CASES[name][3]
        chains.append((s0, n, 3 + i % 3, 700 + i, out))
        out += n
    return chains, out


def _case(oracle, name):
    if name not in _cache:
        from hygeia_amd import synthetic as syn

        K, M, B, T, S, cov, dseed = CASES[name]
        mu, sg = syn.regime_params(K)
        d = syn.simulate(T, S, S, K=K, seed=dseed, coverage=cov, split_frac=0.1)
        thetas = [_theta(K, k) for k in range(2)]
        params = [oracle.make_params(K=K, M=M, B=B, mu=mu, sigma=sg, theta=th) for th in thetas]
        E = oracle.emission(params[0], d["meth_control"], d["tot_control"], d["meth_case"], d["tot_case"])
        _cache[name] = dict(mu=mu, sg=sg, d=d, thetas=thetas, params=params, E=E, refs=None)
    return _cache[name]


def _refs(oracle, name):
    """The oracle's run of every chain under the first model: computed once, read-only."""
    c = _case(oracle, name)
    if c["refs"] is None:
        refs = []
        for (s0, n, sd, cid, _) in _chains(name)[0]:
            r = oracle.chain(c["params"][0], c["E"][s0:s0 + n], sd, cid, want_modes=True)
            assert r["status"] == 0
            for v in r.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            refs.append(r)
        c["refs"] = refs
    return c["refs"]


def _models(name, c, n_models):
    from hygeia_amd import two_group

    K, M, B, T = CASES[name][:4]
    d = c["d"]
    maxr = int(max(d["tot_control"].max(), d["tot_case"].max()))
    return two_group.genome_models(c["thetas"][:n_models], c["mu"], c["sg"], maxr, [T + 5] * n_models,
                                   num_resampled_ancestors=M, num_samples_backward=B)


def _schedule(L, model, lengths, cus, resident):
    n = len(lengths)
    T = np.ascontiguousarray(lengths, dtype=np.int32)
    blocks = np.zeros(2, np.int32)
    order, begin, end = (np.zeros((2, n), np.int32) for _ in range(3))
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rounds = L.hyg_tg_forward_schedule(model.handle, p(T), n, 0, 0, cus, resident, 2, p(blocks), p(order), p(begin),
                                       p(end))
    return rounds, blocks, order, begin, end


@pytest.fixture
def forced_rounds():
    """The pretended device and the library settings of one test; defaults restored afterwards."""
    from hygeia_amd import _lib

    L = _lib.load()

    def apply(rounds, rotation=1, window=-1, width=0):
        _lib.check(L.hyg_tg_set_device_cus(0, CUS))
        _lib.check(L.hyg_tg_set_forward_rounds(rounds))
        _lib.check(L.hyg_tg_set_priority_rotation(rotation))
        _lib.check(L.hyg_tg_set_gather_window(window))
        _lib.check(L.hyg_tg_force_threads(width, 0))

    yield apply
    L.hyg_tg_set_device_cus(0, 0)
    L.hyg_tg_set_forward_rounds(1)
    L.hyg_tg_set_priority_rotation(1)
    L.hyg_tg_set_gather_window(-1)
    L.hyg_tg_force_threads(0, 0)


@pytest.mark.parametrize("name", list(CASES))
def test_chains_resume_from_every_kind_of_record(oracle, forced_rounds, name):
    """No GPU: the cuts of the launch (the schedule for 4 CUs, three workgroups
    resident, at the width such a launch has) and the kind of the step whose
    record each chain resumes from."""
    from hygeia_amd import _lib

    L = _lib.load()
    c = _case(oracle, name)
    refs = _refs(oracle, name)
    models = _models(name, c, 1)
    try:
        forced_rounds(2, width=256)
        rounds, blocks, order, begin, end = _schedule(L, models[0], LENGTHS, CUS, 3)
    finally:
        for m in models:
            m.close()
    assert rounds == 2 and blocks[0] == 10 and blocks[1] == 9
    cut = end[0]
    assert cut[6] == LENGTHS[6] == 50 and 6 not in order[1][:9]  # ends in round 1
    assert cut[8] == 65  # the smallest legal cut
    assert cut[2] == 129 == (LENGTHS[2] - 2) // 64 * 64 + 1  # the last legal one below T
    kinds = [int(refs[i]["modes"][cut[i] - 1]) // 65536 for i in range(10) if cut[i] < LENGTHS[i]]
    assert len(kinds) == 9
    assert OPTIMAL in kinds and KEEP in kinds, kinds
    if name == "c3_cov1000":
        assert UNBIASED in kinds, kinds


def _launch(name, c, models, chain_model=None):
    import torch

    from hygeia_amd import two_group

    dev = torch.device("cuda", 0)
    d = c["d"]
    counts = [torch.from_numpy(np.ascontiguousarray(d[k]).view(np.int16)).to(dev) for k in
              ("meth_control", "tot_control", "meth_case", "tot_case")]
    chains, n_out = _chains(name)
    model = models if chain_model is not None else models[0]
    dc = two_group.DeviceChains(model, chains, n_out, device=dev, final_weights=True, chain_model=chain_model)
    for a in (dc.merged, dc.control, dc.case, dc.split_probs, dc.regime_probs, dc.ws):
        a.zero_()  # bytes no chain writes (a record's unused ancestors) compare equal
    E = dc.emission(*counts)
    dc.run(E)
    torch.cuda.synchronize()
    got = {k: getattr(dc, k).cpu().numpy() for k in NAMES}
    got["workspace"] = dc.ws.cpu().numpy()
    return got


def _assert_same(got, want, what):
    assert (got["status"] == 0).all() and (want["status"] == 0).all(), what
    for k in NAMES + ("workspace",):
        assert got[k].tobytes() == want[k].tobytes(), (what, k)


PATTERN = 0xA5  # the byte the outputs of a launch with failing chains hold before it


def _launch_failing(name, c, models, fails):
    """_launch with chains that fail: fails = {chain: site}. The table is the
    device emission followed by one copy of each failing chain's rows with
    every entry of that site -inf; the chain's site_begin points at its copy
    (the chains share site rows). The outputs hold PATTERN before the launch,
    the workspace zeros."""
    import torch

    from hygeia_amd import two_group

    dev = torch.device("cuda", 0)
    d = c["d"]
    counts = [torch.from_numpy(np.ascontiguousarray(d[k]).view(np.int16)).to(dev) for k in
              ("meth_control", "tot_control", "meth_case", "tot_case")]
    chains, n_out = _chains(name)
    dc = two_group.DeviceChains(models[0], chains, n_out, device=dev, final_weights=True)
    parts = [dc.emission(*counts)]
    rows = parts[0].shape[0]
    for i, site in sorted(fails.items()):
        s0, n, sd, cid, o0 = chains[i]
        assert 0 <= site < n
        copy = parts[0][s0:s0 + n].clone()
        copy[site, :] = float("-inf")
        chains[i] = (rows, n, sd, cid, o0)
        parts.append(copy)
        rows += n
    dc = two_group.DeviceChains(models[0], chains, n_out, device=dev, final_weights=True)
    for k in NAMES:
        getattr(dc, k).view(torch.uint8).fill_(PATTERN)
    dc.ws.zero_()  # bytes no chain writes (a record's unused ancestors) compare equal
    dc.run(torch.cat(parts))
    torch.cuda.synchronize()
    got = {k: getattr(dc, k).cpu().numpy() for k in NAMES}
    got["workspace"] = dc.ws.cpu().numpy()
    return got


def _assert_same_with_failures(got, want, fails, what):
    """_assert_same for a launch whose chains `fails` end in HYG_ENUMERIC (-2) and whose other chains succeed."""
    status = np.zeros(len(LENGTHS), np.int32)
    status[sorted(fails)] = -2
    np.testing.assert_array_equal(got["status"], status, err_msg=str(what))
    np.testing.assert_array_equal(want["status"], status, err_msg=str(what))
    for k in NAMES + ("workspace",):
        assert got[k].tobytes() == want[k].tobytes(), (what, k)


def _need_gpu():
    from hygeia_amd import _lib

    L = _lib.load()
    if L.hyg_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")
    return L


def _two_rounds_planned(L, model):
    """The launch that follows runs in two rounds: what the launcher's own schedule says on this device."""
    rounds, blocks, _, _, _ = _schedule(L, model, LENGTHS, 0, L.hyg_tg_chains_per_cu(model.handle, len(LENGTHS)))
    return rounds == 2 and blocks[1] == 9


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_two_rounds_equal_one_launch(oracle, forced_rounds, name):
    L = _need_gpu()
    c = _case(oracle, name)
    models = _models(name, c, 1)
    try:
        forced_rounds(0)
        one = _launch(name, c, models)
        forced_rounds(2)
        assert _two_rounds_planned(L, models[0])
        two = _launch(name, c, models)
    finally:
        for m in models:
            m.close()
    _assert_same(two, one, name)
    if name == "c3":  # and both are the oracle's
        for i, ((s0, n, sd, cid, o0), ref) in enumerate(zip(_chains(name)[0], _refs(oracle, name))):
            for k in ("merged", "control", "case", "split_probs", "regime_probs"):
                np.testing.assert_array_equal(two[k][o0:o0 + n], ref[k], err_msg=f"chain {i} {k}")
            assert two["log_z"][i] == ref["log_z"], i
            np.testing.assert_array_equal(two["final_w"][i], ref["final_log_weights"], err_msg=f"chain {i}")


@pytest.mark.gpu
def test_two_rounds_equal_one_launch_multi_model(oracle, forced_rounds):
    """The same chains over two models, alternating."""
    L = _need_gpu()
    c = _case(oracle, "c3")
    models = _models("c3", c, 2)
    order = [i % 2 for i in range(len(LENGTHS))]
    try:
        forced_rounds(0)
        one = _launch("c3", c, models, chain_model=order)
        forced_rounds(2)
        assert _two_rounds_planned(L, models[0])
        two = _launch("c3", c, models, chain_model=order)
        single = _launch("c3", c, models)
    finally:
        for m in models:
            m.close()
    _assert_same(two, one, "multi-model")
    assert two["log_z"][1] != single["log_z"][1] and two["log_z"][0] == single["log_z"][0]  # the second model is in use


@pytest.mark.gpu
@pytest.mark.parametrize("rotation,window", [(0, -1), (1, 0)])
def test_two_rounds_without_rotation_or_gather_window(oracle, forced_rounds, rotation, window):
    """Both settings reach the resuming kernel through the layout, as they reach the launch's own."""
    L = _need_gpu()
    c = _case(oracle, "c3")
    models = _models("c3", c, 1)
    try:
        forced_rounds(0, rotation, window)
        one = _launch("c3", c, models)
        forced_rounds(2, rotation, window)
        assert _two_rounds_planned(L, models[0])
        two = _launch("c3", c, models)
    finally:
        for m in models:
            m.close()
    _assert_same(two, one, (rotation, window))


@pytest.mark.gpu
@pytest.mark.parametrize("launch", ["A", "B"])
@pytest.mark.parametrize("name", ["generic", "c3"])
def test_failing_chains_in_two_rounds(oracle, forced_rounds, name, launch):
    """Chains that end in HYG_ENUMERIC (every entry of one emission row -inf) in
    a launch in two rounds. A: a chain fails at the last site of round 1 (round
    1's closing check), one inside round 1, one inside round 2 and one, which
    ends in round 1, at its last site. B: one at the first site round 2
    computes, one at the last site of a chain that runs in round 2 (round 2's
    closing check) and one at site 0. Round 2 skips a chain that failed in round
    1. Every output and every workspace byte is that of the one launch; a failed
    chain has status -2, log Z and final weights -inf and no row written; the
    others are the oracle's."""
    L = _need_gpu()
    c = _case(oracle, name)
    refs = _refs(oracle, name)
    chains = _chains(name)[0]
    models = _models(name, c, 1)
    try:
        forced_rounds(2)
        assert _two_rounds_planned(L, models[0])
        rounds, blocks, order, begin, end = _schedule(L, models[0], LENGTHS, 0,
                                                      L.hyg_tg_chains_per_cu(models[0].handle, len(LENGTHS)))
        cut = [int(x) for x in end[0]]
        assert cut[8] == 65 and cut[2] == 129 and LENGTHS[2] == 190
        assert cut[6] == LENGTHS[6] == 50 and 6 not in order[1][:blocks[1]]  # ends in round 1
        assert 64 < cut[0] and cut[0] + 37 < LENGTHS[0] - 1 and cut[4] < LENGTHS[4]
        fails = {"A": {8: 64, 2: 100, 0: cut[0] + 37, 6: 49}, "B": {8: 65, 2: 189, 4: 0}}[launch]
        for i, site in fails.items():  # on the CPU first: the chain fails, and not before that site
            s0, n, sd, cid, _ = chains[i]
            P = c["E"][s0:s0 + n].copy()
            P[site, :] = -np.inf
            assert oracle.chain(c["params"][0], P[:site + 1], sd, cid)["status"] == -2
            assert site == 0 or oracle.chain(c["params"][0], P[:site], sd, cid)["status"] == 0
        two = _launch_failing(name, c, models, fails)
        forced_rounds(0)
        one = _launch_failing(name, c, models, fails)
    finally:
        for m in models:
            m.close()
    _assert_same_with_failures(two, one, fails, (name, launch))
    for i, ((s0, n, sd, cid, o0), ref) in enumerate(zip(chains, refs)):
        rows = {k: two[k][o0:o0 + n] for k in ("merged", "control", "case", "split_probs", "regime_probs")}
        if i in fails:
            assert two["log_z"][i] == -np.inf and (two["final_w"][i] == -np.inf).all(), i
            for k, a in rows.items():
                assert (np.ascontiguousarray(a).view(np.uint8) == PATTERN).all(), (i, k)
        else:
            for k, a in rows.items():
                np.testing.assert_array_equal(a, ref[k], err_msg=f"chain {i} {k}")
            assert two["log_z"][i] == ref["log_z"], i
            np.testing.assert_array_equal(two["final_w"][i], ref["final_log_weights"], err_msg=f"chain {i}")
