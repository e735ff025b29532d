"""GPU parity of multi-model launches: chains that each name their model
(hyg_tg_run_chains_multi, `hygeia infer_genome`).

Bar: bit for bit on every output (merged, control, case, split_probs,
regime_probs, log_z, final_log_weights, status) against single-model
hyg_tg_run_chains launches of the same chains, each with its own model, and for
shapes A and B against the CPU oracle as well. Every shape first shows on the
CPU that the check can fail: the oracle's chain differs between two of the
shape's models.
"""
import ctypes as C
import gzip
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cli_trees import _theta, _tree, _write_chrom  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAMES = ("merged", "control", "case", "split_probs", "regime_probs", "log_z", "final_w", "status")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    from hygeia_amd import _lib

    if _lib.load().hyg_device_count() <= 0:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")


# shape -> K, M, B, T, samples, coverage, data seed, max_duration per model, chain_model,
#          chains (site_begin, n_sites, seed, chain id, out_begin)
def _chains(T, lens, model_order):
    chains, out = [], 0
    for i, n in enumerate(lens):
        chains.append((T - n if i % 2 else 0, n, 3 + i % 3, 900 + i, out))
        out += n
    return chains, out, list(model_order)


SHAPES = {
    # index and dcap mix-ups: three models, distinct hazard-table lengths
    "A": dict(K=3, M=4, B=5, T=150, S=1, cov=30.0, dseed=51, max_dur=(151, 300, 1000),
              lens=(150, 97, 150, 64, 150, 1, 149), order=(2, 0, 1, 1, 0, 2, 0)),
    # the pipeline shape and its compiled builds
    "B": dict(K=6, M=50, B=25, T=400, S=2, cov=30.0, dseed=52, max_dur=(401, 2000),
              lens=(400, 333, 400, 257), order=(1, 0, 0, 1)),
    # K = 12: the GW backward at 256 and the tail-overlap split
    "C": dict(K=12, M=50, B=25, T=120, S=2, cov=30.0, dseed=53, max_dur=(121, 500),
              lens=(120, 120, 101), order=(0, 1, 1)),
    # forward GW
    "D": dict(K=6, M=200, B=5, T=80, S=2, cov=30.0, dseed=54, max_dur=(81, 90),
              lens=(80, 66), order=(1, 0)),
}

_SETUP = {}


def _setup(oracle, shape):
    """The shape's data, models' parameters and, per chain, the oracle's result
    under that chain's model where the shape is compared against it (computed
    once, shared, read-only)."""
    if shape in _SETUP:
        return _SETUP[shape]
    from hygeia_amd import synthetic as syn

    s = SHAPES[shape]
    K, M, B, T = s["K"], s["M"], s["B"], s["T"]
    mu, sg = syn.regime_params(K)
    d = syn.simulate(T, s["S"], s["S"], K=K, seed=s["dseed"], coverage=s["cov"])
    thetas = [_theta(K, k) for k in range(len(s["max_dur"]))]
    params = [oracle.make_params(K=K, M=M, B=B, mu=mu, sigma=sg, theta=th) for th in thetas]
    chains, n_out, order = _chains(T, s["lens"], s["order"])
    E = oracle.emission(params[0], d["meth_control"], d["tot_control"], d["meth_case"], d["tot_case"])
    # the check can fail: the first chain under two of the models differs
    s0, n, seed, cid, _ = chains[0]
    a = oracle.chain(params[0], E[s0:s0 + n], seed, cid)
    b = oracle.chain(params[1], E[s0:s0 + n], seed, cid)
    assert a["status"] == 0 and b["status"] == 0
    assert a["log_z"] != b["log_z"]
    assert not np.array_equal(a["regime_probs"], b["regime_probs"])
    assert not np.array_equal(a["control"], b["control"]) or not np.array_equal(a["merged"], b["merged"])
    refs = None
    if shape in ("A", "B"):
        refs = []
        for (s0, n, seed, cid, _), k in zip(chains, order):
            r = oracle.chain(params[k], E[s0:s0 + n], seed, cid)
            for v in r.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            refs.append(r)
    _SETUP[shape] = dict(mu=mu, sg=sg, d=d, thetas=thetas, chains=chains, n_out=n_out, order=order, refs=refs)
    return _SETUP[shape]


def _models(shape, st):
    from hygeia_amd import two_group

    s = SHAPES[shape]
    d = st["d"]
    maxr = int(max(d["tot_control"].max(), d["tot_case"].max()))
    return two_group.genome_models(st["thetas"], st["mu"], st["sg"], maxr, s["max_dur"],
                                   num_resampled_ancestors=s["M"], num_samples_backward=s["B"])


def _counts(d, dev):
    return [torch.from_numpy(np.ascontiguousarray(d[k]).view(np.int16)).to(dev) for k in
            ("meth_control", "tot_control", "meth_case", "tot_case")]


def _launch(model, chains, n_out, counts, dev, chain_model=None):
    from hygeia_amd import two_group

    dc = two_group.DeviceChains(model, chains, n_out, device=dev, final_weights=True, chain_model=chain_model)
    for a in (dc.merged, dc.control, dc.case, dc.split_probs, dc.regime_probs):
        a.zero_()  # rows no chain of this launch writes compare equal
    E = dc.emission(*counts)
    dc.run(E)
    torch.cuda.synchronize()
    return {k: getattr(dc, k).cpu().numpy() for k in NAMES}


def _single_model_launches(models, st, counts, dev):
    """The same chains through hyg_tg_run_chains, one launch per model with the
    chains that name it, assembled as the multi-model launch lays them out."""
    chains, n_out, order = st["chains"], st["n_out"], st["order"]
    whole = None
    for k, m in enumerate(models):
        mine = [i for i, o in enumerate(order) if o == k]
        r = _launch(m, [chains[i] for i in mine], n_out, counts, dev)
        if whole is None:
            whole = {name: np.zeros((len(chains),) + r[name].shape[1:], r[name].dtype)
                     if name in ("log_z", "final_w", "status") else np.zeros_like(r[name]) for name in NAMES}
        for j, i in enumerate(mine):
            _, n, _, _, o0 = chains[i]
            for name in ("merged", "control", "case", "split_probs", "regime_probs"):
                whole[name][o0:o0 + n] = r[name][o0:o0 + n]
            for name in ("log_z", "final_w", "status"):
                whole[name][i] = r[name][j]
    return whole


def _assert_same(got, want, what):
    assert (got["status"] == 0).all(), what
    for name in NAMES:
        assert got[name].tobytes() == want[name].tobytes(), (what, name)


def _assert_oracle(got, st, what):
    for i, ((s0, n, seed, cid, o0), ref) in enumerate(zip(st["chains"], st["refs"])):
        assert ref["status"] == 0
        for name in ("merged", "control", "case", "split_probs", "regime_probs"):
            np.testing.assert_array_equal(got[name][o0:o0 + n], ref[name], err_msg=f"{what} chain {i} {name}")
        assert got["log_z"][i] == ref["log_z"], (what, i)
        np.testing.assert_array_equal(got["final_w"][i], ref["final_log_weights"], err_msg=f"{what} chain {i}")


def _kernel_names(L, models, n):
    h = (C.c_void_p * len(models))(*[m.handle for m in models])
    out = []
    for backward in (0, 1):
        buf = C.create_string_buffer(96)
        assert L.hyg_tg_kernel_name_multi(h, len(models), n, backward, buf, 96) > 1
        out.append(buf.value.decode())
    return tuple(out)


def _close(models):
    for m in models:
        m.close()


def test_shape_a_model_index_and_hazard_lengths(oracle):
    """Seven chains over three models in the order [2, 0, 1, 1, 0, 2, 0], at
    the automatic widths and forced 64, 128 and 256."""
    from hygeia_amd import _lib

    L = _lib.load()
    st = _setup(oracle, "A")
    dev = torch.device("cuda", 0)
    counts = _counts(st["d"], dev)
    models = _models("A", st)
    try:
        want = _single_model_launches(models, st, counts, dev)
        _assert_oracle(want, st, "single-model launches")
        for force in (0, 64, 128, 256):
            _lib.check(L.hyg_tg_force_threads(force, force))
            if force:
                fwd, bwd = _kernel_names(L, models, len(st["chains"]))
                assert fwd == "tg_forward_kernel<%d,0,0,0,false,false,true>" % force
                assert bwd == "tg_backward_kernel<%d,0,0,0,false,false,true>" % force
            got = _launch(models, st["chains"], st["n_out"], counts, dev, chain_model=st["order"])
            _assert_same(got, want, f"forced {force}")
            _assert_oracle(got, st, f"forced {force}")
    finally:
        L.hyg_tg_force_threads(0, 0)
        _close(models)


def test_shape_b_pipeline_shape_builds(oracle):
    """K = 6, M = 50, B = 25: the compiled builds at 512 / 768 (four chains on
    the whole device) and, on a pretended 1-CU device, the 256-thread
    three-per-CU builds."""
    from hygeia_amd import _lib

    L = _lib.load()
    st = _setup(oracle, "B")
    dev = torch.device("cuda", 0)
    counts = _counts(st["d"], dev)
    models = _models("B", st)
    try:
        want = _single_model_launches(models, st, counts, dev)
        _assert_oracle(want, st, "single-model launches")
        assert _kernel_names(L, models, 4) == ("tg_forward_kernel<512,6,50,25,false,false,true>",
                                               "tg_backward_kernel<768,6,50,25,false,false,true>")
        got = _launch(models, st["chains"], st["n_out"], counts, dev, chain_model=st["order"])
        _assert_same(got, want, "automatic")
        _assert_oracle(got, st, "automatic")
        _lib.check(L.hyg_tg_set_device_cus(0, 1))
        assert _kernel_names(L, models, 4) == ("tg_forward_kernel<256,6,50,25,false,false,true>",
                                               "tg_backward_kernel<256,6,50,25,false,false,true>")
        got = _launch(models, st["chains"], st["n_out"], counts, dev, chain_model=st["order"])
        _assert_same(got, want, "1 CU")
        _assert_oracle(got, st, "1 CU")
    finally:
        L.hyg_tg_set_device_cus(0, 0)
        _close(models)


def test_shape_c_k12_gw_backward_and_tail_split(oracle):
    """K = 12 on a pretended 2-CU device: three chains run the 512-thread
    forward one per CU, split head 2 / tail 1 (each part's descriptors carry
    their chains' model index), and the GW backward at 256. Also with the tail
    overlap off."""
    from hygeia_amd import _lib

    L = _lib.load()
    st = _setup(oracle, "C")
    dev = torch.device("cuda", 0)
    counts = _counts(st["d"], dev)
    models = _models("C", st)
    try:
        want = _single_model_launches(models, st, counts, dev)
        _lib.check(L.hyg_tg_set_device_cus(0, 2))
        assert _kernel_names(L, models, 3) == ("tg_forward_kernel<512,12,50,25,false,false,true>",
                                               "tg_backward_kernel<256,12,50,25,false,true,true>")
        assert L.hyg_tg_chains_per_cu(models[0].handle, 3) == 1  # the condition of the split
        for overlap in (1, 0):
            _lib.check(L.hyg_tg_set_tail_overlap(overlap))
            got = _launch(models, st["chains"], st["n_out"], counts, dev, chain_model=st["order"])
            _assert_same(got, want, f"tail overlap {overlap}")
    finally:
        L.hyg_tg_set_tail_overlap(1)
        L.hyg_tg_set_device_cus(0, 0)
        _close(models)


def test_shape_d_forward_gw(oracle):
    """K = 6, M = 200: the particle arrays in global memory, both kernels at 256."""
    from hygeia_amd import _lib

    L = _lib.load()
    st = _setup(oracle, "D")
    dev = torch.device("cuda", 0)
    counts = _counts(st["d"], dev)
    models = _models("D", st)
    try:
        assert L.hyg_tg_global_weights(models[0].handle) == 1
        assert _kernel_names(L, models, 2) == ("tg_forward_kernel<256,0,0,0,false,true,true>",
                                               "tg_backward_kernel<256,0,0,0,false,true,true>")
        want = _single_model_launches(models, st, counts, dev)
        got = _launch(models, st["chains"], st["n_out"], counts, dev, chain_model=st["order"])
        _assert_same(got, want, "forward GW")
    finally:
        _close(models)


def test_one_model_through_the_multi_entry_equals_run_chains(oracle):
    """n_models = 1: hyg_tg_run_chains_multi gives the bits of hyg_tg_run_chains
    (device entry and host entry)."""
    from hygeia_amd import two_group

    st = _setup(oracle, "A")
    dev = torch.device("cuda", 0)
    counts = _counts(st["d"], dev)
    models = _models("A", st)
    try:
        chains, n_out = st["chains"], st["n_out"]
        want = _launch(models[1], chains, n_out, counts, dev)
        got = _launch([models[1]], chains, n_out, counts, dev, chain_model=[0] * len(chains))
        _assert_same(got, want, "one model")
        d = st["d"]
        obs = {"control": d["meth_control"], "case": d["meth_case"]}
        tot = {"control": d["tot_control"], "case": d["tot_case"]}
        h1 = two_group.run_chains_host(obs, tot, models[1], chains, n_out, final_weights=True)
        hm = two_group.run_chains_host(obs, tot, [models[1]], chains, n_out, final_weights=True,
                                       chain_model=[0] * len(chains))
        for name in NAMES:
            if name in ("log_z", "final_w", "status"):
                assert hm[name].tobytes() == h1[name].tobytes() == want[name].tobytes(), name
            else:  # (host outputs are not zeroed: compare the rows the chains write)
                for (_, n, _, _, o0) in chains:
                    assert hm[name][o0:o0 + n].tobytes() == h1[name][o0:o0 + n].tobytes() == \
                        want[name][o0:o0 + n].tobytes(), name
    finally:
        _close(models)


def test_host_entry_multi_equals_device_entry(oracle):
    """hyg_tg_run_chains_host_multi (infer_genome's launch) on shape A."""
    from hygeia_amd import two_group

    st = _setup(oracle, "A")
    models = _models("A", st)
    try:
        d = st["d"]
        r = two_group.run_chains_host({"control": d["meth_control"], "case": d["meth_case"]},
                                      {"control": d["tot_control"], "case": d["tot_case"]}, models, st["chains"],
                                      st["n_out"], final_weights=True, chain_model=st["order"])
        _assert_oracle(r, st, "host entry")
        assert (r["status"] == 0).all()
    finally:
        _close(models)


# ------------------------------------------------------------ infer_genome
def test_infer_genome_writes_the_files_of_infer_many_per_chromosome(tmp_path, monkeypatch):
    """Two chromosomes (2 400 and 1 300 sites, segments of 1 000, two seeds,
    distinct theta files): one launch writes the files of two `hygeia
    infer_many` runs with byte-identical contents (_tree), the optimal_time_*
    files excepted. With one theta
    file missing the command fails before it writes anything. (Each run
    writes to ./res of a directory of its own: the flags files hold
    --results_dir as given.)"""
    from hygeia_amd import cli

    root = str(tmp_path)
    _write_chrom(root, "21", 2400, 0)
    _write_chrom(root, "X", 1300, 1)
    common = ["--segment_size", "1000", "--buffer_size", "50", "--seeds", "0,5", "--num_samples_backward", "7",
              "--data_dir", str(tmp_path / "data"), "--single_group_dir", str(tmp_path / "sg")]
    for d in ("many", "genome", "swapped", "none"):
        os.makedirs(tmp_path / d)
    common += ["--results_dir", "res"]
    monkeypatch.chdir(tmp_path / "many")
    for c in ("21", "X"):
        assert cli.main(["infer_many", "--chrom", c] + common) == 0
    monkeypatch.chdir(tmp_path / "genome")
    assert cli.main(["infer_genome", "--chroms", "all"] + common) == 0
    many, genome = _tree(str(tmp_path / "many" / "res")), _tree(str(tmp_path / "genome" / "res"))
    assert sorted(many) == sorted(genome)
    assert {os.path.dirname(k) for k in many} == {"chrom_21_0", "chrom_21_1", "chrom_21_2", "chrom_X_0", "chrom_X_1"}
    compared = 0
    for k in many:
        if os.path.basename(k).startswith("optimal_time_"):
            continue
        assert many[k] == genome[k], k
        compared += 1
    assert compared == 5 * (5 + 2 * (1 + 5 + 1))  # per batch: 5 input copies; per seed: flags, 5 arrays, log Z
    # the two chromosomes' models differ: chromosome X under chromosome 21's theta gives other files
    os.replace(tmp_path / "sg" / "theta_X.csv.gz", tmp_path / "theta_X.keep")
    with gzip.open(tmp_path / "sg" / "theta_21.csv.gz", "rb") as src, \
            gzip.open(tmp_path / "sg" / "theta_X.csv.gz", "wb") as dst:
        dst.write(src.read())
    monkeypatch.chdir(tmp_path / "swapped")
    assert cli.main(["infer_many", "--chrom", "X"] + common) == 0
    swapped = _tree(str(tmp_path / "swapped" / "res"))
    assert any(swapped[k] != genome[k] for k in swapped if k.endswith(".npz"))
    # a missing theta file: non-zero exit, nothing written
    os.remove(tmp_path / "sg" / "theta_X.csv.gz")
    monkeypatch.chdir(tmp_path / "none")
    assert cli.main(["infer_genome", "--chroms", "21,X"] + common) != 0
    assert os.listdir(tmp_path / "none") == []
