"""GPU parity of the traced forward-only launches (hyg_tg_trace_chains*): the
TRC builds of tg_forward_kernel, which store per site the running log Z and the
filtering marginals. Reference: the CPU oracle on every prefix of the chain
(tests/tg_trace_ref.py). Bar: log_z_t `==`, the two f32 arrays
assert_array_equal; log Z, final weights and status byte for byte those of the
plain forward-only launch.
"""
import ast
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import cli_trees, tg_trace_ref  # noqa: E402
from tests import test_gpu_tg_filter as flt  # noqa: E402  (its cases, shared oracle chains and chain lists)
from tests import test_gpu_tg_global_w as gw  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    from hygeia_amd import _lib

    if _lib.load().hyg_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")


TRACE_KEYS = ("log_z_t", "split_probs", "regime_probs")
_ROWS = {}


def reference_rows(oracle, case):
    """(rows compared, their reference) of a case, computed once: 0, 1, 2,
    T - 1, the steps around every change of mode and every unbiased step, every
    fifth row; all rows at K = 3."""
    key = str(case)
    if key not in _ROWS:
        (K, M, B, T, S, cov, dseed, seed, _), mu, sg, theta, d, ref = flt._case(oracle, case)
        p = oracle.make_params(K=K, M=M, B=B, mu=mu, sigma=sg)
        E = oracle.emission(p, d["meth_control"], d["tot_control"], d["meth_case"], d["tot_case"])
        R = tg_trace_ref.row_set(ref["modes"] // 65536, stride=5, every=(K == 3))
        rows = tg_trace_ref.rows(p, E, R, seed, 1000 + seed)
        for v in rows.values():
            v.setflags(write=False)
        _ROWS[key] = rows
    return _ROWS[key]


def _trace_name(model, n):
    from hygeia_amd import _lib

    buf = C.create_string_buffer(128)
    assert _lib.load().hyg_tg_trace_kernel_name(model.handle, n, buf, 128) > 1
    return buf.value.decode()


def _same_trace(a, b, what=""):
    for k in TRACE_KEYS:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


# case, forced forward widths (0: automatic), the build each runs, GW
SINGLE = [(s[0], s[1] if s[0] != ("gw", 1) else (0,), s[2], s[3]) for s in flt.SINGLE]


@pytest.mark.parametrize("case,widths,builds,is_gw", SINGLE, ids=[str(s[0]) for s in SINGLE])
def test_single_chain_trace_bit_exact(oracle, case, widths, builds, is_gw):
    from hygeia_amd import _lib, two_group

    L = _lib.load()
    (K, M, B, T, S, cov, dseed, seed, steps), mu, sg, theta, d, ref = flt._case(oracle, case)
    # on the CPU first: the data reaches the paths the case is here for, and the
    # rows compared hold probabilities away from 0 and 1
    assert ref["status"] == 0
    modes = ref["modes"][1:] // 65536
    assert tuple(int((modes == k).sum()) for k in (0, 1, 2)) == steps
    want = reference_rows(oracle, case)
    R = want["rows"]
    assert {0, 1, 2, T - 1} <= set(R.tolist()) and (K != 3 or len(R) == T)
    assert want["log_z_t"][-1] == ref["log_z"]
    inner = lambda a: int(((a > 0.01) & (a < 0.99)).sum())  # noqa: E731
    print(f"{case}: {len(R)} rows, {inner(want['split_probs'])} split and {inner(want['regime_probs'])} regime "
          "probabilities in (0.01, 0.99)")
    assert inner(want["split_probs"]) >= 1 and inner(want["regime_probs"]) >= 1
    model = gw._model(mu, sg, theta, M, B, flt._maxr(d), T + 5)
    # the same forward in the generic build: the compiled shapes are (M, B) = (50, 25), and the filter does not use B
    generic = gw._model(mu, sg, theta, M, B - 1, flt._maxr(d), T + 5) if builds[widths[0]].split(",")[1] != "0" else None
    obs, tot = flt._obs(d)
    chains = [(0, T, seed, 1000 + seed, 0)]
    first = None
    try:
        assert model.global_weights == is_gw
        for w in widths:
            _lib.check(L.hyg_tg_force_threads(w, 0))
            gwflag = "true" if is_gw else "false"
            assert _trace_name(model, 1) == "tg_forward_kernel<%s,false,%s,false,false,true>" % (builds[w], gwflag)
            r = two_group.filter_chains_host(obs, tot, model, chains, final_weights=True, trace="all", n_out_rows=T)
            assert r["status"][0] == 0
            for k in TRACE_KEYS:
                assert not np.isnan(r[k]).any(), (w, k)
            for i, t in enumerate(R):
                assert r["log_z_t"][t] == want["log_z_t"][i], (w, t)
            np.testing.assert_array_equal(r["split_probs"][R], want["split_probs"], err_msg=f"width {w}")
            np.testing.assert_array_equal(r["regime_probs"][R], want["regime_probs"], err_msg=f"width {w}")
            assert r["log_z_t"][T - 1] == r["log_z"][0] == ref["log_z"]
            # log Z, final weights and status: the plain forward-only launch's
            flt._assert_same(r, two_group.filter_chains_host(obs, tot, model, chains, final_weights=True), f"width {w}")
            # log Z_t alone (no class sums): the same bytes
            z = two_group.filter_chains_host(obs, tot, model, chains, trace="log_z", n_out_rows=T)
            assert sorted(z) == ["log_z", "log_z_t", "status"]
            assert z["log_z_t"].tobytes() == r["log_z_t"].tobytes() and z["log_z"][0] == ref["log_z"]
            # every row, between the widths, the multi-model build and the generic build
            if first is None:
                first = r
            _same_trace(r, first, f"width {w} against width {widths[0]}")
            mm = two_group.filter_chains_host(obs, tot, [model], chains, final_weights=True, chain_model=[0],
                                              trace="all", n_out_rows=T)
            _same_trace(mm, first, f"width {w}, multi-model entry")
            flt._assert_same(mm, r, f"width {w}, multi-model entry")
            if generic is not None:
                assert _trace_name(generic, 1) == "tg_forward_kernel<%d,0,0,0,false,false,false,false,true>" % (w or 512)
                g = two_group.filter_chains_host(obs, tot, generic, chains, final_weights=True, trace="all",
                                                 n_out_rows=T)
                _same_trace(g, first, f"width {w}, generic build")
                flt._assert_same(g, r, f"width {w}, generic build")
    finally:
        L.hyg_tg_force_threads(0, 0)
        model.close()
        if generic is not None:
            generic.close()


# flt.SEVEN with a gap of five rows before the fourth chain and twelve unowned rows at the end
SEVEN = [c[:4] + (c[4] + (5 if i >= 3 else 0),) for i, c in enumerate(flt.SEVEN)]
SEVEN_ROWS = 575
UNOWNED = list(range(171, 176)) + list(range(563, SEVEN_ROWS))


def _assert_owned_rows(r, singles, what):
    for i, ((s0, n, seed, cid, o0), one) in enumerate(zip(SEVEN, singles)):
        for k in TRACE_KEYS:
            assert r[k][o0:o0 + n].tobytes() == one[k].tobytes(), (what, i, k)
        assert r["log_z"][i] == one["log_z"][0] == r["log_z_t"][o0 + n - 1] and r["status"][i] == 0
        assert r["final_w"][i].tobytes() == one["final_w"][0].tobytes(), (what, i)
    for k in TRACE_KEYS:  # the sentinel of the host arrays
        assert np.isnan(r[k][UNOWNED]).all() and not np.isnan(np.delete(r[k], UNOWNED, axis=0)).any(), (what, k)


def test_seven_chains_one_launch(oracle):
    """Mixed lengths (T = 1 and T = 2 among them) over overlapping sites, each
    chain's rows at its out_begin: those of its single-chain traced launch;
    rows that no chain owns keep the sentinel. Then the same chains under three
    models in one multi-model launch."""
    from hygeia_amd import two_group

    (K, M, B, T, S, cov, dseed, _, _), mu, sg, theta, d, _ = flt._case(oracle, "c3")
    p = oracle.make_params(K=K, M=M, B=B, mu=mu, sigma=sg)
    E = oracle.emission(p, d["meth_control"], d["tot_control"], d["meth_case"], d["tot_case"])
    model = gw._model(mu, sg, theta, M, B, flt._maxr(d), T + 5)
    obs, tot = flt._obs(d)
    kw = dict(final_weights=True, trace="all")
    try:
        singles = [two_group.filter_chains_host(obs, tot, model, [(s0, n, seed, cid, 0)], n_out_rows=n, **kw)
                   for (s0, n, seed, cid, _) in SEVEN]
        # the short chains against the oracle, every row
        for i in (1, 3, 6):
            s0, n, seed, cid, _ = SEVEN[i]
            want = tg_trace_ref.rows(p, E[s0:s0 + n], range(n), seed, cid)
            for k in TRACE_KEYS:
                np.testing.assert_array_equal(singles[i][k], want[k], err_msg=f"chain {i} {k}")
        r = two_group.filter_chains_host(obs, tot, model, SEVEN, n_out_rows=SEVEN_ROWS, **kw)
        _assert_owned_rows(r, singles, "one launch")
        flt._assert_same(r, two_group.filter_chains_host(obs, tot, model, SEVEN, final_weights=True), "plain launch")
    finally:
        model.close()
    # multi-model
    rng = np.random.default_rng(900 + K)
    thetas = [theta] + [theta + rng.normal(0.0, 0.7, theta.shape) for _ in range(2)]
    models = [two_group.CaseControlModel(mu, sg, th, num_resampled_ancestors=M, num_samples_backward=B,
                                         max_total_reads=flt._maxr(d), max_duration=md, **mkw)
              for th, md, mkw in zip(thetas, [T + 5, 400, 1000], flt.MODEL_KW)]
    try:
        singles = [two_group.filter_chains_host(obs, tot, models[k], [(s0, n, seed, cid, 0)], n_out_rows=n, **kw)
                   for k, (s0, n, seed, cid, _) in zip(flt.MODEL_ORDER, SEVEN)]
        assert singles[5]["log_z_t"].tobytes() != two_group.filter_chains_host(
            obs, tot, models[1], [SEVEN[5][:4] + (0,)], n_out_rows=300, **kw)["log_z_t"].tobytes()  # the models matter
        r = two_group.filter_chains_host(obs, tot, models, SEVEN, chain_model=flt.MODEL_ORDER, n_out_rows=SEVEN_ROWS,
                                         **kw)
        _assert_owned_rows(r, singles, "multi-model launch")
    finally:
        for m in models:
            m.close()


@pytest.mark.parametrize("case", ["c3", ("gw", 0)], ids=["c3", "gw"])
def test_nothing_written_outside_the_arrays(oracle, case):
    """The exact hyg_tg_filter_workspace_bytes and the exact trace arrays of two
    chains, a 1 MiB guard behind each."""
    from hygeia_amd import _lib, two_group

    L = _lib.load()
    (K, M, B, T, S, cov, dseed, seed, _), mu, sg, theta, d, ref = flt._case(oracle, case)
    model = gw._model(mu, sg, theta, M, B, flt._maxr(d), T + 5)
    dev = torch.device("cuda", 0)
    chains = [(0, T, seed, 1000 + seed, 0), (0, T, seed, 1000 + seed, T)]
    guard = 1 << 20
    try:
        df = two_group.DeviceFilter(model, chains, device=dev, final_weights=True, trace="all", n_out_rows=2 * T)
        assert df.ws_bytes == L.hyg_tg_filter_workspace_bytes(model.handle, 2) < guard
        sizes = {"ws": df.ws_bytes, "log_z_t": 8 * 2 * T, "split_probs": 4 * 2 * T, "regime_probs": 4 * 2 * T * 2 * K}
        bufs = {k: torch.full((n + guard,), 0xA5, dtype=torch.uint8, device=dev) for k, n in sizes.items()}
        E = df.emission(*flt._device_counts(d, dev))
        s = torch.cuda.current_stream(dev).cuda_stream
        tr = _lib.TgTrace(*[bufs[k].data_ptr() for k in TRACE_KEYS])
        _lib.check(L.hyg_tg_trace_chains(model.handle, df._arr, 2, E.data_ptr(), bufs["ws"].data_ptr(), df.ws_bytes,
                                         C.byref(tr), df.log_z.data_ptr(), df.final_w.data_ptr(), df.status.data_ptr(),
                                         C.c_void_p(s)))
        torch.cuda.synchronize()
        for k, n in sizes.items():
            assert bool((bufs[k][n:] == 0xA5).all().item()), k
        got = {k: bufs[k][:sizes[k]].cpu().numpy().view({"log_z_t": np.float64}.get(k, np.float32)) for k in TRACE_KEYS}
        want = reference_rows(oracle, case)
        for c in range(2):
            assert df.status[c].item() == 0 and df.log_z[c].item() == ref["log_z"]
            np.testing.assert_array_equal(got["log_z_t"][c * T:(c + 1) * T][want["rows"]], want["log_z_t"])
            np.testing.assert_array_equal(got["split_probs"][c * T:(c + 1) * T][want["rows"]], want["split_probs"])
            np.testing.assert_array_equal(got["regime_probs"].reshape(2 * T, 2 * K)[c * T:(c + 1) * T][want["rows"]],
                                          want["regime_probs"])
        # DeviceFilter.run: the same launch on its own arrays
        df.run(E)
        torch.cuda.synchronize()
        for k in TRACE_KEYS:
            assert getattr(df, k).cpu().numpy().tobytes() == got[k].tobytes(), k
        # log Z_t alone: the other two pointers NULL
        only = _lib.TgTrace(bufs["log_z_t"].data_ptr(), None, None)
        bufs["log_z_t"].fill_(0xA5)
        _lib.check(L.hyg_tg_trace_chains(model.handle, df._arr, 2, E.data_ptr(), bufs["ws"].data_ptr(), df.ws_bytes,
                                         C.byref(only), df.log_z.data_ptr(), None, None, C.c_void_p(s)))
        torch.cuda.synchronize()
        for k, n in sizes.items():
            assert bool((bufs[k][n:] == 0xA5).all().item()), k
        assert bufs["log_z_t"][:sizes["log_z_t"]].cpu().numpy().tobytes() == got["log_z_t"].tobytes()
    finally:
        model.close()


def test_commands_write_the_trace(tmp_path):
    """`hygeia filter_genome`: each task's files hold the rows of
    filter_chains_host(trace="all") of that task; `hygeia log_z --trimmed`: every
    increment is the difference of two rows of the filter_log_z file of its task
    and seed."""
    from hygeia_amd import cli, two_group

    root = str(tmp_path)
    lengths = {"3": 300, "Y": 250}
    for k, (chrom, T) in enumerate(lengths.items()):
        cli_trees._write_chrom(root, chrom, T, k)
    common = ["--chroms", "all", "--seeds", "0,4", "--segment_size", "200", "--buffer_size", "20",
              "--num_samples_backward", "7", "--data_dir", os.path.join(root, "data"), "--single_group_dir",
              os.path.join(root, "sg")]
    res = os.path.join(root, "fg")
    assert cli.main(["filter_genome", "--results_dir", res] + common) == 0
    f = cli.parse_flags(["--results_dir", res] + common, cli.GENOME_FLAGS)
    groups = cli._genome_groups(f)
    mu, sigma, K = cli._regimes(f)
    N = 50 * 48
    max_reads = max(int(max(g[4].max(), g[6].max())) for g in groups)
    rows = {}
    for chrom, theta, tasks, meth_c, tot_c, meth_k, tot_k, _ in groups:
        assert [t[0] for t in tasks] == [0, 1]
        model = two_group.CaseControlModel(mu, sigma, theta, max_total_reads=max_reads, max_duration=300,
                                           **cli._model_kw(f, 50))
        try:
            for (b, lo, hi, r0, r1) in tasks:
                for sd in (0, 4):
                    r = two_group.filter_chains_host({"control": meth_c[lo:hi], "case": meth_k[lo:hi]},
                                                     {"control": tot_c[lo:hi], "case": tot_k[lo:hi]}, model,
                                                     [(0, hi - lo, sd, cli.chain_id(chrom, b), 0)], trace="all",
                                                     n_out_rows=hi - lo)
                    assert r["status"][0] == 0
                    d = os.path.join(res, f"chrom_{chrom}_{b}")
                    for name, key in (("filter_split_probs", "split_probs"), ("filter_regime_probs", "regime_probs"),
                                      ("filter_log_z", "log_z_t")):
                        with np.load(os.path.join(d, f"{name}_{N}_{sd}.npz")) as z:
                            got = z["arr_0"]
                        assert got.dtype == r[key].dtype and got.shape == r[key].shape
                        assert got.tobytes() == r[key].tobytes(), (chrom, b, sd, name)
                    with open(os.path.join(d, f"log_normalizing_constants_optimal_{sd}.txt")) as fh:
                        assert ast.literal_eval(fh.read()) == {N: float(r["log_z"][0])}
                    rows[(chrom, b, sd)] = (r["log_z_t"], r0, max(r0, r1))
        finally:
            model.close()
    assert cli.main(["log_z", "--trimmed", "--results_dir", os.path.join(root, "lz")] + common) == 0
    with open(os.path.join(root, "lz", "log_z_trimmed.tsv")) as fh:
        head, *lines = [line.rstrip("\n").split("\t") for line in fh]
    assert head[-2:] == ["n_trimmed_sites", "log_z_increment"] and len(lines) == 4 * 2
    total = 0
    for chrom, b, sd, M, u, om, mg, sp, n, inc in lines:
        L, r0, r1 = rows[(chrom, int(b), int(sd))]
        assert int(n) == r1 - r0 > 0
        assert float(inc) == float(L[r1 - 1]) - (float(L[r0 - 1]) if r0 > 0 else 0.0), (chrom, b, sd)
        total += int(n)
    assert total == 2 * sum(lengths.values())  # the trimmed ranges tile both chromosomes, once per seed
    with open(os.path.join(root, "lz", "log_z.tsv")) as fh:
        _, *plain = [line.rstrip("\n").split("\t") for line in fh]
    for row in plain:
        assert float(row[-1]) == float(rows[(row[0], int(row[1]), int(row[2]))][0][-1])
