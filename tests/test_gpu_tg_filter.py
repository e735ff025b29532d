"""GPU parity of the forward-only launches (hyg_tg_filter_chains*): the particle
filter in builds that record no ancestor history (tg_forward_kernel's REC =
false). Bar: log Z `==`, the final log-weights assert_array_equal and status 0,
against the CPU oracle and against the full launch (filter + backward
simulation) of the same chains.
"""
import ast
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import cli_trees  # noqa: E402
from tests import test_gpu_tg_global_w as gw  # noqa: E402  (its _setup, CASES and shared oracle chains)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    from hygeia_amd import _lib

    if _lib.load().hyg_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")


# K, M, B, T, S, coverage, data seed, inference seed, oracle steps (keep, optimal, unbiased)
OWN = {
    "c3": (6, 50, 25, 300, 3, 100.0, 51, 40, (4, 295, 0)),         # the compiled pipeline shape
    "c3_unbiased": (6, 50, 25, 250, 3, 1000.0, 52, 41, (24, 224, 1)),  # high coverage: an unbiased-fallback step
    "generic": (3, 20, 5, 300, 3, 100.0, 53, 42, (13, 286, 0)),    # no build of its own: the generic ones
    "c5": (12, 50, 25, 120, 3, 100.0, 54, 43, (22, 97, 0)),        # the compiled K = 12 shape
}
_REF = {}


def _case(oracle, name):
    """(row, mu, sigma, theta, data, oracle chain with modes) of a case: a row
    of OWN, or ("gw", i) for row i of test_gpu_tg_global_w's CASES (whose
    chains that module computes once and shares)."""
    if isinstance(name, tuple):
        mu, sg, theta, d, ref = gw._reference(oracle, name[1])
        return gw.CASES[name[1]], mu, sg, theta, d, ref
    if name not in _REF:
        K, M, B, T, S, cov, dseed, seed, _ = OWN[name]
        mu, sg, theta, d, p = gw._setup(oracle, K, M, B, T, S, cov, dseed)
        E = oracle.emission(p, d["meth_control"], d["tot_control"], d["meth_case"], d["tot_case"])
        ref = oracle.chain(p, E, seed, 1000 + seed, want_modes=True)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[name] = (mu, sg, theta, d, ref)
    return (OWN[name],) + _REF[name]


def _obs(d):
    return ({"control": d["meth_control"], "case": d["meth_case"]}, {"control": d["tot_control"], "case": d["tot_case"]})


def _maxr(d):
    return int(max(d["tot_control"].max(), d["tot_case"].max()))


def _name(model, n):
    from hygeia_amd import _lib

    L = _lib.load()
    buf = C.create_string_buffer(128)
    assert L.hyg_tg_filter_kernel_name(model.handle, n, buf, 128) > 1
    return buf.value.decode()


def _assert_chain(r, i, ref, what=""):
    assert r["status"][i] == 0, what
    assert r["log_z"][i] == ref["log_z"], what
    np.testing.assert_array_equal(r["final_w"][i], ref["final_log_weights"], err_msg=what)


def _assert_same(a, b, what=""):
    for k in ("log_z", "final_w", "status"):
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


# case, forced forward widths (0: automatic), the build each runs
SINGLE = [
    ("c3", (0, 256, 512, 768), {0: "512,6,50,25", 256: "256,6,50,25", 512: "512,6,50,25", 768: "768,6,50,25"}, False),
    ("c3_unbiased", (0, 256, 512, 768),
     {0: "512,6,50,25", 256: "256,6,50,25", 512: "512,6,50,25", 768: "768,6,50,25"}, False),
    ("generic", (64, 128, 256, 512, 768), {w: "%d,0,0,0" % w for w in (64, 128, 256, 512, 768)}, False),
    ("c5", (512, 768), {512: "512,12,50,25", 768: "768,12,50,25"}, False),
    (("gw", 0), (0,), {0: "256,0,0,0"}, True),   # K = 13, M = 50: generic GW
    (("gw", 1), (0, 512), {0: "256,0,0,0", 512: "256,0,0,0"}, True),   # the same with an unbiased step
    (("gw", 3), (0,), {0: "256,0,0,0"}, True),   # K = 6, M = 200: GW with the general weight path
]


@pytest.mark.parametrize("case,widths,builds,is_gw", SINGLE, ids=[str(s[0]) for s in SINGLE])
def test_single_chain_bit_exact(oracle, case, widths, builds, is_gw):
    from hygeia_amd import _lib, two_group

    L = _lib.load()
    (K, M, B, T, S, cov, dseed, seed, steps), mu, sg, theta, d, ref = _case(oracle, case)
    # on the CPU first: the data reaches the paths the case is here for
    assert ref["status"] == 0
    modes = ref["modes"][1:] // 65536  # 0 keep, 1 optimal, 2 unbiased
    assert tuple(int((modes == k).sum()) for k in (0, 1, 2)) == steps
    if case in ("c3_unbiased", ("gw", 1), ("gw", 3)):
        assert steps[2] >= 1
    model = gw._model(mu, sg, theta, M, B, _maxr(d), T + 5)
    obs, tot = _obs(d)
    chains = [(0, T, seed, 1000 + seed, 0)]
    try:
        assert model.global_weights == is_gw
        full = two_group.run_chains_host(obs, tot, model, chains, T, final_weights=True)
        _assert_chain(full, 0, ref, "full launch")
        for w in widths:
            _lib.check(L.hyg_tg_force_threads(w, 0))
            gwflag = "true" if is_gw else "false"
            assert _name(model, 1) == "tg_forward_kernel<%s,false,%s,false,false>" % (builds[w], gwflag)
            r = two_group.filter_chains_host(obs, tot, model, chains, final_weights=True)
            _assert_chain(r, 0, ref, f"width {w}")
            _assert_same(r, full, f"width {w} against the full launch")
            # without the final weights (NULL): the same log Z
            r2 = two_group.filter_chains_host(obs, tot, model, chains)
            assert sorted(r2) == ["log_z", "status"] and r2["log_z"][0] == ref["log_z"] and r2["status"][0] == 0
    finally:
        L.hyg_tg_force_threads(0, 0)
        model.close()


@pytest.mark.parametrize("window", [0, 8, -1])
def test_gather_window(oracle, window):
    from hygeia_amd import _lib, two_group

    L = _lib.load()
    (K, M, B, T, S, cov, dseed, seed, steps), mu, sg, theta, d, ref = _case(oracle, "c3")
    model = gw._model(mu, sg, theta, M, B, _maxr(d), T + 5)
    obs, tot = _obs(d)
    try:
        _lib.check(L.hyg_tg_set_gather_window(window))
        for w in (256, 512):
            _lib.check(L.hyg_tg_force_threads(w, 0))
            r = two_group.filter_chains_host(obs, tot, model, [(0, T, seed, 1000 + seed, 0)], final_weights=True)
            _assert_chain(r, 0, ref, f"window {window} width {w}")
    finally:
        L.hyg_tg_set_gather_window(-1)
        L.hyg_tg_force_threads(0, 0)
        model.close()


# (site_begin, n_sites, seed, chain id, out_begin): overlapping sites, T = 1 and T = 2 among them
SEVEN = [(10, 40, 3, 500, 0), (299, 1, 4, 501, 40), (150, 130, 3, 502, 41), (0, 2, 4, 503, 171), (100, 75, 5, 504, 173),
         (0, 300, 6, 505, 248), (290, 10, 7, 506, 548)]


def test_seven_chains_one_launch(oracle):
    """Mixed lengths over overlapping sites: each chain its own oracle chain and
    the full launch's; a second launch and a launch shaped for a 2-CU device
    (more chains than CUs: the 256-thread build instead of the 512-thread one)
    give the same bytes."""
    from hygeia_amd import _lib, two_group

    L = _lib.load()
    (K, M, B, T, S, cov, dseed, _, _), mu, sg, theta, d, _ = _case(oracle, "c3")
    p = oracle.make_params(K=K, M=M, B=B, mu=mu, sigma=sg)
    E = oracle.emission(p, d["meth_control"], d["tot_control"], d["meth_case"], d["tot_case"])
    refs = [oracle.chain(p, E[s0:s0 + n], seed, cid) for (s0, n, seed, cid, _) in SEVEN]
    model = gw._model(mu, sg, theta, M, B, _maxr(d), T + 5)
    obs, tot = _obs(d)
    try:
        assert _name(model, 7).startswith("tg_forward_kernel<512,6,50,25,")
        first = two_group.filter_chains_host(obs, tot, model, SEVEN, final_weights=True)
        for i, ref in enumerate(refs):
            assert ref["status"] == 0
            _assert_chain(first, i, ref, f"chain {i}")
        _assert_same(first, two_group.run_chains_host(obs, tot, model, SEVEN, 558, final_weights=True), "full launch")
        _assert_same(first, two_group.filter_chains_host(obs, tot, model, SEVEN, final_weights=True), "second launch")
        try:
            _lib.check(L.hyg_tg_set_device_cus(0, 2))
            assert _name(model, 7).startswith("tg_forward_kernel<256,6,50,25,")
            few = two_group.filter_chains_host(obs, tot, model, SEVEN, final_weights=True)
        finally:
            L.hyg_tg_set_device_cus(0, 0)
        _assert_same(first, few, "2-CU launch")
    finally:
        model.close()


def test_thousand_chains_more_workgroups_than_the_gpu_holds(oracle):
    from hygeia_amd import two_group

    K, M, B, T, n = 2, 3, 2, 16, 1000
    mu, sg, theta, d, p = gw._setup(oracle, K, M, B, 64, 2, 30.0, 55)
    E = oracle.emission(p, d["meth_control"], d["tot_control"], d["meth_case"], d["tot_case"])
    chains = [(i % (64 - T + 1), T, i % 13, 7000 + i, 0) for i in range(n)]
    want = np.array([oracle.chain(p, E[s0:s0 + T], seed, cid)["log_z"] for (s0, _, seed, cid, _) in chains])
    model = gw._model(mu, sg, theta, M, B, _maxr(d), T)
    obs, tot = _obs(d)
    try:
        assert _name(model, n).startswith("tg_forward_kernel<256,0,0,0,")  # three workgroups per CU at the most
        r = two_group.filter_chains_host(obs, tot, model, chains)
        assert (r["status"] == 0).all()
        np.testing.assert_array_equal(r["log_z"], want)
    finally:
        model.close()


# three models that differ in theta, omega_case, split_prob, merge_log_prob and max_duration
MODEL_KW = [dict(), dict(omega_case=0.7, split_prob=0.05), dict(merge_log_prob=float(np.log(0.25)), split_prob=0.02)]
MODEL_ORDER = [2, 0, 1, 1, 2, 0, 1]  # of the seven chains


@pytest.mark.parametrize("shape", [(3, 20, 5), (6, 50, 25)], ids=["K3", "pipeline"])
def test_multi_model_launch(oracle, shape):
    from hygeia_amd import _lib, two_group

    K, M, B = shape
    T = 300
    mu, sg, theta0, d, _ = gw._setup(oracle, K, M, B, T, 3, 100.0, 56)
    rng = np.random.default_rng(900 + K)
    thetas = [theta0] + [theta0 + rng.normal(0.0, 0.7, theta0.shape) for _ in range(2)]
    durations = [T + 5, 400, 1000]
    params = [oracle.make_params(K=K, M=M, B=B, mu=mu, sigma=sg, theta=th, **kw) for th, kw in zip(thetas, MODEL_KW)]
    # one emission table: the models share mu and sigma
    E = oracle.emission(params[0], d["meth_control"], d["tot_control"], d["meth_case"], d["tot_case"])
    chain_of = lambda k, c: oracle.chain(params[k], E[c[0]:c[0] + c[1]], c[2], c[3])  # noqa: E731
    # on the CPU first: the models matter (the long chain's log Z under models 0 and 1)
    assert chain_of(0, SEVEN[5])["log_z"] != chain_of(1, SEVEN[5])["log_z"]
    refs = [chain_of(k, c) for k, c in zip(MODEL_ORDER, SEVEN)]
    models = [two_group.CaseControlModel(mu, sg, th, num_resampled_ancestors=M, num_samples_backward=B,
                                         max_total_reads=_maxr(d), max_duration=md, **kw)
              for th, md, kw in zip(thetas, durations, MODEL_KW)]
    obs, tot = _obs(d)
    L = _lib.load()
    try:
        buf = C.create_string_buffer(128)
        handles = (C.c_void_p * 3)(*[m.handle for m in models])
        assert L.hyg_tg_filter_kernel_name_multi(handles, 3, 7, buf, 128) > 1
        assert buf.value.decode().endswith(",false,false,true,false>")
        r = two_group.filter_chains_host(obs, tot, models, SEVEN, final_weights=True, chain_model=MODEL_ORDER)
        for i, ref in enumerate(refs):
            assert ref["status"] == 0
            _assert_chain(r, i, ref, f"chain {i} (model {MODEL_ORDER[i]})")
        # each model's chains in a single-model forward-only launch
        for k, model in enumerate(models):
            own = [i for i, m in enumerate(MODEL_ORDER) if m == k]
            one = two_group.filter_chains_host(obs, tot, model, [SEVEN[i] for i in own], final_weights=True)
            for j, i in enumerate(own):
                assert one["log_z"][j] == r["log_z"][i] and one["status"][j] == 0
                assert one["final_w"][j].tobytes() == r["final_w"][i].tobytes()
        full = two_group.run_chains_host(obs, tot, models, SEVEN, 558, chain_model=MODEL_ORDER)
        assert full["log_z"].tobytes() == r["log_z"].tobytes() and (full["status"] == 0).all()
        # one model through the _multi entry: the single-model entry's bytes
        a = two_group.filter_chains_host(obs, tot, models[1], SEVEN, final_weights=True)
        b = two_group.filter_chains_host(obs, tot, [models[1]], SEVEN, final_weights=True, chain_model=[0] * 7)
        _assert_same(a, b, "one model through the _multi entry")
    finally:
        for m in models:
            m.close()


def _device_counts(d, dev):
    return [torch.from_numpy(np.ascontiguousarray(d[k]).view(np.int16)).to(dev)
            for k in ("meth_control", "tot_control", "meth_case", "tot_case")]


@pytest.mark.parametrize("case", ["c3", ("gw", 0)], ids=["c3", "gw"])
def test_nothing_written_outside_the_workspace(oracle, case):
    """The exact hyg_tg_filter_workspace_bytes, with a 1 MiB guard behind it:
    at T = 300 and M = 50 (250 KB of records in a full launch) a stray record
    store lands in the guard or spoils the result."""
    from hygeia_amd import _lib, two_group

    L = _lib.load()
    (K, M, B, T, S, cov, dseed, seed, _), mu, sg, theta, d, ref = _case(oracle, case)
    model = gw._model(mu, sg, theta, M, B, _maxr(d), T + 5)
    dev = torch.device("cuda", 0)
    chains = [(0, T, seed, 1000 + seed, 0)] * 2
    try:
        df = two_group.DeviceFilter(model, chains, device=dev, final_weights=True)
        assert df.ws_bytes == L.hyg_tg_filter_workspace_bytes(model.handle, 2) < 1 << 20
        guard = 1 << 20
        ws = torch.full((df.ws_bytes + guard,), 0xA5, dtype=torch.uint8, device=dev)
        E = df.emission(*_device_counts(d, dev))
        s = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(L.hyg_tg_filter_chains(model.handle, df._arr, 2, E.data_ptr(), ws.data_ptr(), df.ws_bytes,
                                          df.log_z.data_ptr(), df.final_w.data_ptr(), df.status.data_ptr(),
                                          C.c_void_p(s)))
        torch.cuda.synchronize()
        assert bool((ws[df.ws_bytes:] == 0xA5).all().item())
        r = {k: getattr(df, k).cpu().numpy() for k in ("log_z", "final_w", "status")}
        for i in range(2):
            _assert_chain(r, i, ref, f"chain {i}")
        # without final weights and status (NULL: the status goes to the header's slot), the same log Z
        df.log_z.fill_(0.0)
        _lib.check(L.hyg_tg_filter_chains(model.handle, df._arr, 2, E.data_ptr(), ws.data_ptr(), df.ws_bytes,
                                          df.log_z.data_ptr(), None, None, C.c_void_p(s)))
        torch.cuda.synchronize()
        assert bool((ws[df.ws_bytes:] == 0xA5).all().item())
        assert df.log_z.cpu().numpy().tobytes() == r["log_z"].tobytes()
        # DeviceFilter.run: the same launch on its own workspace
        df.log_z.fill_(0.0)
        df.run(E)
        torch.cuda.synchronize()
        assert df.log_z.cpu().numpy().tobytes() == r["log_z"].tobytes()
    finally:
        model.close()


def test_workspace_too_small_is_refused(oracle):
    from hygeia_amd import _lib, two_group

    L = _lib.load()
    for case in ("c3", ("gw", 0)):
        (K, M, B, T, S, cov, dseed, seed, _), mu, sg, theta, d, ref = _case(oracle, case)
        model = gw._model(mu, sg, theta, M, B, _maxr(d), T + 5)
        dev = torch.device("cuda", 0)
        try:
            df = two_group.DeviceFilter(model, [(0, T, seed, 1000 + seed, 0)], device=dev, final_weights=True)
            E = df.emission(*_device_counts(d, dev))
            df.log_z.fill_(123.0)
            df.final_w.fill_(-7.0)
            df.status.fill_(55)
            s = torch.cuda.current_stream(dev).cuda_stream
            rc = L.hyg_tg_filter_chains(model.handle, df._arr, 1, E.data_ptr(), df.ws.data_ptr(), df.ws_bytes - 1,
                                        df.log_z.data_ptr(), df.final_w.data_ptr(), df.status.data_ptr(), C.c_void_p(s))
            assert rc == _lib.HYG_EINVAL
            assert "workspace too small" in L.hyg_last_error().decode()
            torch.cuda.synchronize()
            assert df.log_z[0].item() == 123.0 and bool((df.final_w == -7.0).all().item()) and df.status[0].item() == 55
            df.run(E)  # the full workspace runs
            torch.cuda.synchronize()
            assert df.status[0].item() == 0 and df.log_z[0].item() == ref["log_z"]
        finally:
            model.close()


def test_kernel_timing_reports_no_backward(oracle):
    from hygeia_amd import _lib, two_group

    L = _lib.load()
    (K, M, B, T, S, cov, dseed, seed, _), mu, sg, theta, d, ref = _case(oracle, "generic")
    model = gw._model(mu, sg, theta, M, B, _maxr(d), T + 5)
    obs, tot = _obs(d)
    ms = (C.c_float * 3)()
    try:
        L.hyg_set_kernel_timing(1)
        two_group.run_chains_host(obs, tot, model, [(0, T, seed, 1000 + seed, 0)], T)
        _lib.check(L.hyg_tg_last_kernel_ms(ms))
        assert ms[1] > 0 and ms[2] > 0
        two_group.filter_chains_host(obs, tot, model, [(0, T, seed, 1000 + seed, 0)])
        _lib.check(L.hyg_tg_last_kernel_ms(ms))
        assert ms[1] > 0 and ms[2] == -1.0
    finally:
        L.hyg_set_kernel_timing(0)
        model.close()


def test_log_z_command_equals_infer_genome(tmp_path):
    """Every row of log_z.tsv is the number `hygeia infer_genome` writes to
    log_normalizing_constants_optimal_{seed}.txt with that row's setting."""
    from hygeia_amd import cli

    root = str(tmp_path)
    for k, (chrom, T) in enumerate((("3", 300), ("Y", 250))):
        cli_trees._write_chrom(root, chrom, T, k)
    common = ["--chroms", "all", "--seeds", "0,4", "--segment_size", "200", "--buffer_size", "20",
              "--num_samples_backward", "7", "--data_dir", os.path.join(root, "data"), "--single_group_dir",
              os.path.join(root, "sg")]
    assert cli.main(["log_z", "--omega_case", "0.7,0.8", "--split_prob", "0.01,0.05", "--results_dir",
                     os.path.join(root, "lz")] + common) == 0
    with open(os.path.join(root, "lz", "log_z.tsv")) as fh:
        head, *rows = [line.rstrip("\n").split("\t") for line in fh]
    assert head == list(("chrom", "batch", "seed", "num_resampled_particles", "minimum_duration", "omega_case",
                         "merge_log_prob", "split_prob", "n_sites", "log_z"))
    assert len(rows) == 4 * 2 * 4  # (2 + 2 tasks) x 2 seeds x 4 settings
    got = {}
    for chrom, b, sd, M, u, om, mg, sp, n, lz in rows:
        assert (M, u, float(mg)) == ("50", "3", float(np.log(0.1)))
        got[(chrom, int(b), int(sd), float(om), float(sp))] = float(lz)
    assert len(got) == len(rows)
    for om in (0.7, 0.8):
        for sp in (0.01, 0.05):
            res = os.path.join(root, f"infer_{om}_{sp}")
            assert cli.main(["infer_genome", "--omega_case", repr(om), "--split_prob", repr(sp), "--results_dir", res]
                            + common) == 0
            for chrom in ("3", "Y"):
                for b in (0, 1):
                    for sd in (0, 4):
                        with open(os.path.join(res, f"chrom_{chrom}_{b}",
                                               f"log_normalizing_constants_optimal_{sd}.txt")) as fh:
                            want = ast.literal_eval(fh.read())
                        assert got[(chrom, b, sd, om, sp)] == want[50 * 48], (chrom, b, sd, om, sp)
    # the summary: per setting, the sum over the tasks of the log of the seeds' mean Z
    with open(os.path.join(root, "lz", "log_z_summary.tsv")) as fh:
        _, *srows = [line.rstrip("\n").split("\t") for line in fh]
    assert len(srows) == 4
    for M, u, om, mg, sp, n_tasks, n_seeds, total in srows:
        assert (n_tasks, n_seeds) == ("4", "2")
        x = np.array([[got[(chrom, b, sd, float(om), float(sp))] for sd in (0, 4)]
                      for chrom in ("3", "Y") for b in (0, 1)])
        want = (np.logaddexp(x[:, 0], x[:, 1]) - np.log(2.0)).sum()
        # a handful of roundings of numbers of this size (the command sums exactly)
        assert float(total) == pytest.approx(want, rel=1e-14, abs=0.0)
