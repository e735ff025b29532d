"""GPU parity of the two-group shapes whose particle arrays do not fit in LDS.

From K = 13 at M = 50 (or K = 6 at M = 200) the N_max log-weights and sort keys
of a chain exceed the 160 KiB of a CU; such a shape keeps them in a per-chain
global scratch and runs the 256-thread kernels (hyg_tg_global_weights). A shape
just under the limit fits at 256 threads only and runs there. Bar: as
tests/test_gpu_two_group.py, bit-exact against the CPU oracle.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _have_gpu():
    from hygeia_amd import _lib

    return _lib.load().hyg_device_count() > 0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not _have_gpu():
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")


def _setup(oracle, K, M, B, T, S, cov, dseed, split_frac=0.1):
    from hygeia_amd import synthetic as syn

    mu, sg = syn.regime_params(K)
    d = syn.simulate(T, S, S, K=K, seed=dseed, coverage=cov, split_frac=split_frac)
    p = oracle.make_params(K=K, M=M, B=B, mu=mu, sigma=sg)
    theta = np.array(p.theta[: p.theta_len])
    return mu, sg, theta, d, p


def _model(mu, sg, theta, M, B, max_reads, max_dur):
    from hygeia_amd import two_group

    return two_group.CaseControlModel(mu, sg, theta, num_resampled_ancestors=M, num_samples_backward=B,
                                      max_total_reads=max_reads, max_duration=max_dur)


# The smallest shapes at which these kernels can go wrong: just over the LDS
# limit, at HYG_KMAX, M > 64 (the general weight path), M = the workgroup size.
CASES = [
    # K, M, B, T, S, coverage, data seed, inference seed, oracle steps (keep, optimal, unbiased)
    (13, 50, 25, 300, 3, 60.0, 31, 20, (18, 281, 0)),    # N_max = 9 750: the first K refused before
    (13, 50, 25, 250, 6, 1000.0, 42, 31, (14, 234, 1)),  # high coverage: an unbiased-fallback step
    (12, 60, 25, 300, 3, 100.0, 35, 24, (23, 276, 0)),   # the C5 regimes with M just over the limit
    (6, 200, 25, 300, 4, 100.0, 34, 23, (11, 287, 1)),   # M > 64: general weight path, general K loop
    (14, 64, 30, 200, 2, 30.0, 36, 25, (11, 188, 0)),    # M = 64, B = 30
    (16, 50, 25, 300, 2, 100.0, 32, 21, (6, 293, 0)),    # HYG_KMAX
    (16, 256, 8, 120, 2, 30.0, 37, 26, (12, 107, 0)),    # HYG_KMAX, M = 256 threads: N_max = 73 728
    # just UNDER the limit: 163 392 B of LDS at 256 threads fit, the 512-thread layout the
    # automatic choice would take (164 000 B) does not: runs at 256 threads with its arrays in LDS
    (12, 54, 25, 300, 3, 100.0, 39, 27, (37, 262, 0)),
]
UNDER = len(CASES) - 1  # the case that keeps its particle arrays in LDS

_REF = {}


def _reference(oracle, case):
    """The oracle's chain of a case (computed once, shared, never modified)."""
    if case not in _REF:
        K, M, B, T, S, cov, dseed, seed, _ = CASES[case]
        mu, sg, theta, d, p = _setup(oracle, K, M, B, T, S, cov, dseed)
        E = oracle.emission(p, d["meth_control"], d["tot_control"], d["meth_case"], d["tot_case"])
        ref = oracle.chain(p, E, seed, 1000 + seed, want_modes=True)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[case] = (mu, sg, theta, d, ref)
    return _REF[case]


def _run_case(case, model, d):
    from hygeia_amd import two_group

    seed = CASES[case][7]
    return two_group.run({"control": d["meth_control"], "case": d["meth_case"]},
                         {"control": d["tot_control"], "case": d["tot_case"]}, model, seed, 1000 + seed)


def _assert_equal(got, ref):
    res, fw, ex = got
    pr = res.particle
    np.testing.assert_array_equal(pr["merged_state"], ref["merged"])
    np.testing.assert_array_equal(pr["control_state"], ref["control"])
    np.testing.assert_array_equal(pr["case_state"], ref["case"])
    np.testing.assert_array_equal(ex["split_probs"], ref["split_probs"])
    np.testing.assert_array_equal(ex["regime_probs"], ref["regime_probs"])
    assert ex["log_z"] == ref["log_z"]
    np.testing.assert_array_equal(fw, ref["final_log_weights"])


@pytest.mark.parametrize("case", range(len(CASES)))
def test_large_shape_chain_bit_exact(oracle, case):
    from hygeia_amd import _lib

    K, M, B, T, S, cov, dseed, seed, steps = CASES[case]
    mu, sg, theta, d, ref = _reference(oracle, case)
    assert ref["status"] == 0
    modes = ref["modes"][1:] // 65536  # 0 keep, 1 optimal, 2 unbiased
    assert tuple(int((modes == k).sum()) for k in (0, 1, 2)) == steps  # the data still reaches every path
    maxr = int(max(d["tot_control"].max(), d["tot_case"].max()))
    model = _model(mu, sg, theta, M, B, maxr, T + 5)
    L = _lib.load()
    assert L.hyg_tg_global_weights(model.handle) == (0 if case == UNDER else 1)
    assert L.hyg_tg_threads_per_chain(model.handle, 1) == 256
    assert 0 < L.hyg_tg_lds_bytes(model.handle, 256, 0) <= 160 * 1024
    _assert_equal(_run_case(case, model, d), ref)


def test_large_shape_batched_chains(oracle):
    """Five chains of different lengths, site and output offsets in one launch:
    each has its own scratch behind the records, and equals its own oracle
    chain. A second launch gives the same bytes (a missing fence would show as
    a difference), and so does a launch shaped for a 2-CU device (more chains
    than CUs)."""
    from hygeia_amd import _lib, two_group

    L = _lib.load()
    K, M, B, S = 13, 50, 25, 3
    mu, sg, theta, d, p = _setup(oracle, K, M, B, 300, S, 60.0, 31)
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(np.ascontiguousarray(d[k]).view(np.int16)).to(dev) for k in
         ("meth_control", "tot_control", "meth_case", "tot_case")}
    # (site_begin, n_sites, seed, chain id, out_begin): overlapping sites, outputs out of site order
    chains = [(10, 40, 3, 500, 208), (299, 1, 4, 501, 0), (150, 130, 3, 502, 78), (0, 2, 4, 503, 1),
              (100, 75, 5, 504, 3)]
    n_out = 250
    model = _model(mu, sg, theta, M, B, int(max(d["tot_control"].max(), d["tot_case"].max())), 200)
    assert L.hyg_tg_global_weights(model.handle) == 1
    E_ref = oracle.emission(p, d["meth_control"], d["tot_control"], d["meth_case"], d["tot_case"])
    refs = [oracle.chain(p, E_ref[s0:s0 + n], seed, cid) for (s0, n, seed, cid, o0) in chains]
    names = ("merged", "control", "case", "split_probs", "regime_probs", "log_z", "final_w", "status")

    def launch():
        dc = two_group.DeviceChains(model, chains, n_out, device=dev, final_weights=True)
        for a in (dc.merged, dc.control, dc.case, dc.split_probs, dc.regime_probs):
            a.zero_()  # rows no chain writes compare equal
        E = dc.emission(t["meth_control"], t["tot_control"], t["meth_case"], t["tot_case"])
        dc.run(E)
        torch.cuda.synchronize()
        return {k: getattr(dc, k).cpu().numpy() for k in names}

    def check(r):
        assert (r["status"] == 0).all()
        for i, (s0, n, seed, cid, o0) in enumerate(chains):
            ref = refs[i]
            for k in ("merged", "control", "case", "split_probs", "regime_probs"):
                np.testing.assert_array_equal(r[k][o0:o0 + n], ref[k], err_msg=f"chain {i} {k}")
            assert r["log_z"][i] == ref["log_z"]
            np.testing.assert_array_equal(r["final_w"][i], ref["final_log_weights"])

    first = launch()
    check(first)
    again = launch()
    for k in names:
        assert first[k].tobytes() == again[k].tobytes(), k
    try:
        _lib.check(L.hyg_tg_set_device_cus(0, 2))
        few = launch()
    finally:
        L.hyg_tg_set_device_cus(0, 0)
    check(few)
    for k in names:
        assert first[k].tobytes() == few[k].tobytes(), k


def test_forced_width_is_ignored_for_large_shapes(oracle):
    """A forced width never makes a supported shape fail: the K = 13 case, and
    the K = 12, M = 54 case whose layout fits at 256 threads only, under forced
    512 / 768 and 768 / 256 run the 256-thread forward, same bits."""
    from hygeia_amd import _lib

    L = _lib.load()
    try:
        for case in (0, UNDER):
            K, M, B, T = CASES[case][:4]
            mu, sg, theta, d, ref = _reference(oracle, case)
            model = _model(mu, sg, theta, M, B, int(max(d["tot_control"].max(), d["tot_case"].max())), T + 5)
            for fwd, bwd in ((512, 768), (768, 256)):
                _lib.check(L.hyg_tg_force_threads(fwd, bwd))
                assert L.hyg_tg_threads_per_chain(model.handle, 1) == 256
                _assert_equal(_run_case(case, model, d), ref)
    finally:
        L.hyg_tg_force_threads(0, 0)


def test_workspace_too_small_is_refused(oracle):
    """hyg_tg_run_chains checks the per-chain scratch against workspace_bytes:
    a workspace short of one chain's scratch is HYG_EINVAL before any launch
    (the outputs keep their fill)."""
    from hygeia_amd import _lib, two_group

    L = _lib.load()
    K, M, B, T = 13, 50, 25, 20
    mu, sg, theta, d, p = _setup(oracle, K, M, B, T, 2, 30.0, 31)
    model = _model(mu, sg, theta, M, B, int(max(d["tot_control"].max(), d["tot_case"].max())), T + 5)
    dev = torch.device("cuda", 0)
    chains = [(0, T, 1, 1, 0)]
    dc = two_group.DeviceChains(model, chains, T, device=dev)
    t = {k: torch.from_numpy(np.ascontiguousarray(d[k]).view(np.int16)).to(dev) for k in
         ("meth_control", "tot_control", "meth_case", "tot_case")}
    E = dc.emission(t["meth_control"], t["tot_control"], t["meth_case"], t["tot_case"])
    scratch = L.hyg_tg_workspace_bytes(model.handle, 2, T) - L.hyg_tg_workspace_bytes(model.handle, 1, T)
    assert scratch >= 16 * model.num_particles
    dc.merged.fill_(-7)
    dc.log_z.fill_(123.0)
    s = torch.cuda.current_stream(dev).cuda_stream
    rc = L.hyg_tg_run_chains(model.handle, dc._arr, 1, E.data_ptr(), dc.ws.data_ptr(), dc.ws_bytes - scratch,
                             C.byref(dc._out), C.c_void_p(s))
    assert rc == _lib.HYG_EINVAL
    assert "workspace too small" in L.hyg_last_error().decode()
    torch.cuda.synchronize()
    assert (dc.merged == -7).all().item() and dc.log_z[0].item() == 123.0  # nothing ran
    dc.run(E)  # the full workspace runs
    torch.cuda.synchronize()
    assert dc.status[0].item() == 0


def _write_inputs(d, chrom, T, K, S=2, seed=4):
    """The files `hygeia infer` reads (the layout of tests/test_cli.py's inputs):
    positions and counts under d/data, the single-group theta under d/sg."""
    import gzip

    from hygeia_amd import synthetic as syn, two_group

    data = syn.simulate(T, S, S, K=K, seed=seed, coverage=30.0)
    os.makedirs(os.path.join(d, "data"), exist_ok=True)
    os.makedirs(os.path.join(d, "sg"), exist_ok=True)
    np.savetxt(os.path.join(d, "data", f"positions_{chrom}.txt.gz"), syn.positions(T, seed).astype(np.float64), fmt="%s")
    for g in ("control", "case"):
        np.savetxt(os.path.join(d, "data", f"n_total_reads_{g}_{chrom}.txt.gz"),
                   data[f"tot_{g}"].astype(np.float64), fmt="%s", delimiter=",")
        np.savetxt(os.path.join(d, "data", f"n_methylated_reads_{g}_{chrom}.txt.gz"),
                   data[f"meth_{g}"].astype(np.float64), fmt="%s", delimiter=",")
    with gzip.open(os.path.join(d, "sg", f"theta_{chrom}.csv.gz"), "wt") as fh:
        fh.write("data\n" + "\n".join(repr(float(x)) for x in two_group.uniform_theta(K, 0.8)) + "\n")
    return data


def test_cli_infer_k13_end_to_end(tmp_path, oracle):
    """`hygeia infer` with 13 regimes (K from len(--mu)) and the default M = 50:
    the reference's files, holding the oracle's arrays."""
    from hygeia_amd import cli, synthetic as syn, two_group

    K, M, B, T = 13, 50, 8, 300
    data = _write_inputs(str(tmp_path), "7", T, K=K)
    mu, sg = (np.asarray(a, np.float32) for a in syn.regime_params(K))
    rc = cli.main(["infer", "--chrom", "7", "--batch", "0", "--segment_size", "1000", "--buffer_size", "50",
                   "--mu", ",".join(repr(float(x)) for x in mu), "--sigma", ",".join(repr(float(x)) for x in sg),
                   "--num_resampled_particles", str(M), "--num_samples_backward", str(B), "--seed", "3",
                   "--data_dir", str(tmp_path / "data"), "--single_group_dir", str(tmp_path / "sg"),
                   "--results_dir", str(tmp_path / "res")])
    assert rc == 0
    (lo, hi), (r0, r1) = cli.segment_index(T, 0, 1000, 50)
    p = oracle.make_params(K=K, M=M, B=B, mu=mu, sigma=sg, theta=two_group.uniform_theta(K, 0.8))
    E = oracle.emission(p, data["meth_control"][lo:hi], data["tot_control"][lo:hi], data["meth_case"][lo:hi],
                        data["tot_case"][lo:hi])
    ref = oracle.chain(p, E, 3, cli.chain_id("7", 0))
    assert ref["status"] == 0
    out = tmp_path / "res" / "chrom_7_0"
    N = M * (2 * K + K * K)
    ld = lambda n: np.load(out / f"{n}_{N}_3.npz")["arr_0"]  # noqa: E731
    np.testing.assert_array_equal(ld("optimal_backward_particles_merged_state"), ref["merged"][r0:r1])
    np.testing.assert_array_equal(ld("optimal_backward_particles_control_state"), ref["control"][r0:r1])
    np.testing.assert_array_equal(ld("optimal_backward_particles_case_state"), ref["case"][r0:r1])
    np.testing.assert_array_equal(ld("optimal_split_probs"), ref["split_probs"])
    np.testing.assert_array_equal(ld("optimal_regime_probs"), ref["regime_probs"])
    txt = (out / "log_normalizing_constants_optimal_3.txt").read_text()
    assert txt.startswith("{%d: " % N)
    assert float(txt.split(":")[1].strip(" }\n")) == pytest.approx(ref["log_z"], rel=1e-15)


def test_infer_many_k13_equals_single_task_runs(tmp_path):
    """`hygeia infer_many` (hyg_tg_run_chains_host, also the serve path's launch)
    with 13 regimes: every (batch, seed) chain of one launch writes the arrays
    of its single-task `hygeia infer` run."""
    from hygeia_amd import cli, synthetic as syn

    K = 13
    _write_inputs(str(tmp_path), "5", 300, K=K)
    mu, sg = (np.asarray(a, np.float32) for a in syn.regime_params(K))
    common = ["--chrom", "5", "--segment_size", "200", "--buffer_size", "20", "--num_samples_backward", "7",
              "--mu", ",".join(repr(float(x)) for x in mu), "--sigma", ",".join(repr(float(x)) for x in sg),
              "--data_dir", str(tmp_path / "data"), "--single_group_dir", str(tmp_path / "sg")]
    for b in (0, 1):  # get_chrom_segments: 1 + 300 // 200 segments
        for sd in (0, 4):
            assert cli.main(["infer", "--batch", str(b), "--seed", str(sd), "--results_dir", str(tmp_path / "one")]
                            + common) == 0
    assert cli.main(["infer_many", "--batches", "all", "--seeds", "0,4", "--results_dir", str(tmp_path / "many")]
                    + common) == 0
    one, many = tmp_path / "one", tmp_path / "many"
    assert sorted(p.name for p in one.iterdir()) == sorted(p.name for p in many.iterdir()) == ["chrom_5_0", "chrom_5_1"]
    n_npz = 0
    for d in one.iterdir():
        names = sorted(p.name for p in d.iterdir())
        assert names == sorted(p.name for p in (many / d.name).iterdir())
        for nm in names:
            if nm.endswith(".npz") and not nm.startswith("optimal_time_"):
                assert f"_{50 * (2 * K + K * K)}_" in nm  # the default M = 50: N_max = 9 750
                np.testing.assert_array_equal(np.load(d / nm)["arr_0"], np.load(many / d.name / nm)["arr_0"])
                n_npz += 1
    assert n_npz == 2 * 2 * 5  # five arrays per (batch, seed)


def test_m_above_256_still_unsupported(oracle):
    """One resampled ancestor per thread of a 256-thread workgroup: M = 300 is
    refused, and the message names M."""
    from hygeia_amd import _lib

    K, M, B, T = 6, 300, 25, 10
    mu, sg, theta, d, p = _setup(oracle, K, M, B, T, 2, 30.0, 38)
    model = _model(mu, sg, theta, M, B, int(max(d["tot_control"].max(), d["tot_case"].max())), T + 5)
    with pytest.raises(_lib.HygError) as e:
        _run_case(0, model, d)
    assert e.value.code == _lib.HYG_EUNSUPPORTED
    assert "M = 300" in str(e.value) and "256" in str(e.value)
