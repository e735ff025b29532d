"""Forward-only launches of the two-group engine (hyg_tg_filter_*), the part
that needs no device: the new symbols, the kernel plan of a forward-only launch
(the REC = false builds), its workspace, the argument checks, and the
`hygeia log_z` command over a fake of two_group.filter_chains_host.
"""
import ctypes as C
import itertools
import math
import os
import zlib

import numpy as np
import pytest

from hygeia_amd import _lib, cli, synthetic as syn, two_group
from tests import cli_trees

NEW = ("hyg_tg_filter_workspace_bytes", "hyg_tg_filter_workspace_bytes_multi", "hyg_tg_filter_chains",
       "hyg_tg_filter_chains_multi", "hyg_tg_filter_chains_host", "hyg_tg_filter_chains_host_multi",
       "hyg_tg_filter_kernel_name", "hyg_tg_filter_kernel_name_multi")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _model(K=3, M=4, B=5, k=0, max_total_reads=40, max_duration=151, **kw):
    mu, sg = syn.regime_params(K)
    rng = np.random.default_rng(100 + k)
    th = two_group.uniform_theta(K, 0.8)
    th = th + (rng.normal(0.0, 0.7, th.shape) if k else 0.0)
    return two_group.CaseControlModel(mu, sg, th, num_resampled_ancestors=M, num_samples_backward=B,
                                      max_total_reads=max_total_reads, max_duration=max_duration, **kw)


def _handles(models):
    return (C.c_void_p * len(models))(*[m.handle for m in models])


def _name(fn, *args):
    need = fn(*args, None, 0)
    assert need > 1, _lib.load().hyg_last_error()
    buf = C.create_string_buffer(need)
    assert fn(*args, buf, need) == need
    return buf.value.decode()


def test_new_symbols_exist(lib):
    for name in NEW:
        assert name in _lib.EXPORTS
        getattr(lib, name)
    assert callable(two_group.filter_chains_host) and hasattr(two_group, "DeviceFilter")
    assert "log_z" in cli.COMMANDS.split() and "log_z" in cli._SUBCOMMANDS


# (shape, forced forward width, chains) -> the eight template arguments, on a 256-CU device
PLAN = [
    ((6, 50, 25), 0, 582, "256,6,50,25,false,false"),    # the pipeline shape, more chains than CUs
    ((6, 50, 25), 0, 73, "512,6,50,25,false,false"),     # at most a chain per CU
    ((6, 50, 25), 768, 582, "768,6,50,25,false,false"),
    ((12, 50, 25), 0, 1164, "512,12,50,25,false,false"),
    ((12, 50, 25), 768, 5, "768,12,50,25,false,false"),
    ((13, 50, 25), 0, 5, "256,0,0,0,false,true"),        # generic GW at 256 whatever width is forced
    ((13, 50, 25), 64, 5, "256,0,0,0,false,true"),
    ((13, 50, 25), 512, 5000, "256,0,0,0,false,true"),
    ((13, 50, 25), 768, 5, "256,0,0,0,false,true"),
    ((12, 54, 25), 0, 5, "256,0,0,0,false,false"),       # fits at 256 only
    ((12, 54, 25), 512, 5, "256,0,0,0,false,false"),
    ((3, 4, 5), 64, 5, "64,0,0,0,false,false"),
    ((3, 4, 5), 128, 5, "128,0,0,0,false,false"),
    ((3, 4, 5), 256, 5, "256,0,0,0,false,false"),
    ((3, 4, 5), 512, 5, "512,0,0,0,false,false"),
    ((3, 4, 5), 768, 5, "768,0,0,0,false,false"),
    ((6, 50, 64), 0, 582, "256,0,0,0,false,false"),      # not the compiled shape (B)
]


@pytest.mark.parametrize("shape,force,n,args", PLAN)
def test_filter_kernel_name_pins_the_plan(lib, shape, force, n, args):
    models = [_model(*shape, k=k) for k in range(2)]
    try:
        assert lib.hyg_tg_set_device_cus(0, 256) == 0
        assert lib.hyg_tg_force_threads(force, 0) == 0
        one = _name(lib.hyg_tg_filter_kernel_name, models[0].handle, n)
        multi = _name(lib.hyg_tg_filter_kernel_name_multi, _handles(models), 2, n)
        assert one == "tg_forward_kernel<%s,false,false>" % args
        assert multi == "tg_forward_kernel<%s,true,false>" % args
        # planned as the forward of a full launch of that many chains: width and GW
        full = _name(lib.hyg_tg_kernel_name, models[0].handle, n, 0).rstrip(">").split("<")[1].split(",")
        assert (full[0], full[5]) == (args.split(",")[0], args.split(",")[5])
        for nm in (one, multi):
            assert len(nm.rstrip(">").split("<")[1].split(",")) == 8 and nm.endswith("false>")
        # the backward's forced width is none of its business
        assert lib.hyg_tg_force_threads(force, 768) == 0
        assert _name(lib.hyg_tg_filter_kernel_name, models[0].handle, n) == one
    finally:
        lib.hyg_tg_force_threads(0, 0)
        lib.hyg_tg_set_device_cus(0, 0)
        for m in models:
            m.close()


def test_filter_plan_follows_the_cu_count(lib):
    m = _model(6, 50, 25)
    try:
        # (256 is also what a host without a device plans for)
        for cus, n, width in ((256, 1, 512), (256, 256, 512), (256, 257, 256)):
            assert lib.hyg_tg_set_device_cus(0, cus) == 0
            assert _name(lib.hyg_tg_kernel_name, m.handle, n, 0).startswith("tg_forward_kernel<%d,6,50,25," % width)
            assert _name(lib.hyg_tg_filter_kernel_name, m.handle, n).startswith("tg_forward_kernel<%d,6,50,25," % width)
    finally:
        lib.hyg_tg_set_device_cus(0, 0)
        m.close()


def test_more_than_256_resampled_particles_is_unsupported(lib):
    models = [_model(3, 257, 5, k=k) for k in range(2)]
    try:
        assert lib.hyg_tg_filter_kernel_name(models[0].handle, 5, None, 0) == _lib.HYG_EUNSUPPORTED
        assert "exceeds 256" in lib.hyg_last_error().decode()
        assert lib.hyg_tg_filter_kernel_name_multi(_handles(models), 2, 5, None, 0) == _lib.HYG_EUNSUPPORTED
        assert lib.hyg_tg_kernel_name(models[0].handle, 5, 0, None, 0) == _lib.HYG_EUNSUPPORTED  # as the full launch
    finally:
        for m in models:
            m.close()


HEADER_PER_CHAIN = 56 + 4 + 8  # the descriptor, the default status and the log Z slot
MODEL_ENTRY = 56  # of the model table of a multi-model launch


def _header(n):
    return (HEADER_PER_CHAIN * n + 255) // 256 * 256


@pytest.mark.parametrize("shape,gw", [((6, 50, 25), False), ((13, 50, 25), True), ((12, 50, 25), False)])
def test_filter_workspace(lib, shape, gw):
    """No history: the size has no argument for the chains' lengths; it grows
    per chain by the descriptor and, for a global-weights shape only, by the
    forward scratch of 16 B x N_max rounded up to 256 B. (K = 12: the full
    launch's backward-only scratch is not in it.)"""
    K, M, B = shape
    models = [_model(K, M, B, k=k) for k in range(3)]
    try:
        m = models[0]
        assert m.global_weights == gw
        nmax = m.num_particles
        scratch = (16 * nmax + 255) // 256 * 256 if gw else 0
        for n in (0, 1, 3, 4, 7, 582, 1000):
            assert lib.hyg_tg_filter_workspace_bytes(m.handle, n) == _header(n) + n * scratch
            multi = lib.hyg_tg_filter_workspace_bytes_multi(_handles(models), 3, n)
            assert multi - n * scratch == (_header(n) + 3 * MODEL_ENTRY + 255) // 256 * 256
            assert two_group.DeviceFilter.workspace_bytes(m, [(0, 5, 0, 0, 0)] * n) == _header(n) + n * scratch
            assert two_group.DeviceFilter.workspace_bytes(models, [(0, 99, 0, 0, 0)] * n) == multi
        # against the full launch of 582 chains of 100 000 sites: the records are gone
        full = lib.hyg_tg_workspace_bytes(m.handle, 582, 58200000)
        assert full - lib.hyg_tg_filter_workspace_bytes(m.handle, 582) >= 58200000 * (32 + 16 * M)
        for force in (64, 512):
            assert lib.hyg_tg_force_threads(force, force) == 0
            assert lib.hyg_tg_filter_workspace_bytes(m.handle, 7) == _header(7) + 7 * scratch
        assert lib.hyg_tg_filter_workspace_bytes(None, 7) == 0
        assert lib.hyg_tg_filter_workspace_bytes(m.handle, -1) == 0
        assert lib.hyg_tg_filter_workspace_bytes_multi(_handles(models), 0, 7) == 0
        assert lib.hyg_tg_filter_workspace_bytes_multi(None, 3, 7) == 0
    finally:
        lib.hyg_tg_force_threads(0, 0)
        for mm in models:
            mm.close()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_argument_errors_are_einval(lib):
    models = [_model(k=0), _model(k=1), _model(k=2, M=5)]
    good = models[:2]
    try:
        chains = (_lib.TgChain * 3)()
        for i in range(3):
            chains[i].n_sites = 5
        lz = np.zeros(3)
        st = np.zeros(3, np.int32)
        z = np.zeros((5, 1), np.uint16)
        idx = (C.c_int32 * 3)(0, 1, 0)
        # incompatible models: every _multi entry, the field named
        for rc in (lib.hyg_tg_filter_kernel_name_multi(_handles(models), 3, 3, None, 0),
                   lib.hyg_tg_filter_chains_multi(_handles(models), 3, chains, idx, 3, None, None, 0, None, None, None,
                                                  None),
                   lib.hyg_tg_filter_chains_host_multi(_handles(models), 3, _p(z), _p(z), 1, _p(z), _p(z), 1, 5, chains,
                                                       idx, 3, _p(lz), None, _p(st))):
            assert rc == _lib.HYG_EINVAL
            assert "differ in num_resampled_ancestors:" in lib.hyg_last_error().decode()
        # a model index out of range, or none
        for bad in (2, -1):
            bidx = (C.c_int32 * 3)(0, 1, bad)
            assert lib.hyg_tg_filter_chains_multi(_handles(good), 2, chains, bidx, 3, None, None, 0, None, None, None,
                                                  None) == _lib.HYG_EINVAL
            assert "chain_model[2] = %d" % bad in lib.hyg_last_error().decode()
            assert lib.hyg_tg_filter_chains_host_multi(_handles(good), 2, _p(z), _p(z), 1, _p(z), _p(z), 1, 5, chains,
                                                       bidx, 3, _p(lz), None, _p(st)) == _lib.HYG_EINVAL
            assert "chain_model[2] = %d" % bad in lib.hyg_last_error().decode()
        assert lib.hyg_tg_filter_chains_multi(_handles(good), 2, chains, None, 3, None, None, 0, None, None, None,
                                              None) == _lib.HYG_EINVAL
        # null model, null arguments, negative length
        assert lib.hyg_tg_filter_chains(None, chains, 3, None, None, 0, None, None, None, None) == _lib.HYG_EINVAL
        assert lib.hyg_tg_filter_chains(good[0].handle, None, 3, None, None, 0, None, None, None,
                                        None) == _lib.HYG_EINVAL
        assert lib.hyg_tg_filter_chains_host(None, _p(z), _p(z), 1, _p(z), _p(z), 1, 5, chains, 3, _p(lz), None,
                                             _p(st)) == _lib.HYG_EINVAL
        assert lib.hyg_tg_filter_kernel_name(None, 3, None, 0) == _lib.HYG_EINVAL
        assert lib.hyg_tg_filter_kernel_name(good[0].handle, 3, None, -1) == _lib.HYG_EINVAL
        with pytest.raises(ValueError):
            two_group.filter_chains_host({"control": z, "case": z}, {"control": z, "case": z}, good[0], [])
        with pytest.raises(ValueError):  # longer than the model's max_duration
            z2 = np.zeros((200, 1), np.uint16)
            two_group.filter_chains_host({"control": z2, "case": z2}, {"control": z2, "case": z2}, good[0],
                                         [(0, 200, 0, 0, 0)])
        with pytest.raises(ValueError):
            two_group.filter_chains_host({"control": z, "case": z}, {"control": z, "case": z}, good, [(0, 5, 0, 0, 0)])
    finally:
        for m in models:
            m.close()


def test_compute_entries_refuse_without_device(lib):
    if lib.hyg_device_count() > 0:
        pytest.skip("host without a GPU only")
    models = [_model(k=0), _model(k=1)]
    try:
        chains = (_lib.TgChain * 2)()
        for i in range(2):
            chains[i].n_sites = 5
        lz, st, z = np.zeros(2), np.zeros(2, np.int32), np.zeros((5, 1), np.uint16)
        E = np.zeros((5, 6))
        idx = (C.c_int32 * 2)(0, 1)
        rcs = [lib.hyg_tg_filter_chains(models[0].handle, chains, 2, _p(E), _p(E), 0, _p(lz), None, None, None),
               lib.hyg_tg_filter_chains_multi(_handles(models), 2, chains, idx, 2, _p(E), _p(E), 0, _p(lz), None, None,
                                              None),
               lib.hyg_tg_filter_chains_host(models[0].handle, _p(z), _p(z), 1, _p(z), _p(z), 1, 5, chains, 2, _p(lz),
                                             None, _p(st)),
               lib.hyg_tg_filter_chains_host_multi(_handles(models), 2, _p(z), _p(z), 1, _p(z), _p(z), 1, 5, chains, idx,
                                                   2, _p(lz), None, _p(st))]
        assert rcs == [_lib.HYG_EDEVICE] * 4
        assert b"no CPU fallback" in lib.hyg_last_error()
        with pytest.raises(_lib.HygError) as e:
            two_group.filter_chains_host({"control": z, "case": z}, {"control": z, "case": z}, models,
                                         [(0, 5, 0, 1, 0), (0, 5, 0, 2, 0)], chain_model=[1, 0])
        assert e.value.code == _lib.HYG_EDEVICE
    finally:
        for m in models:
            m.close()


# ------------------------------------------------------------ hygeia log_z
class FakeFilter:
    """two_group.filter_chains_host without a device: a chain's log Z is a
    function of its own total-read rows, its seed, its chain id and its model's
    parameters. `calls` records every launch."""

    def __init__(self, fail_chain=None):
        self.calls, self.fail_chain = [], fail_chain

    def __call__(self, observations, n_total_reads, model, chains, final_weights=False, chain_model=None):
        models = list(model)
        assert chain_model is not None and len(chain_model) == len(chains) and not final_weights
        desc = [(m.params.num_resampled_ancestors, m.params.minimum_duration, m.params.omega_case,
                 m.params.merge_log_prob, m.params.split_prob, m.params.num_samples_backward,
                 tuple(m.params.theta[: m.params.theta_len]), m.max_total_reads, m.max_duration) for m in models]
        self.calls.append((desc, [tuple(int(x) for x in c) for c in chains], [int(k) for k in chain_model]))
        out = {"log_z": np.zeros(len(chains)), "status": np.zeros(len(chains), np.int32)}
        for i, (s0, T, seed, cid, _) in enumerate(chains):
            tc, tk = (np.asarray(n_total_reads[g][s0:s0 + T]).astype(np.int64) for g in ("control", "case"))
            crc = zlib.crc32(bytes(models[chain_model[i]].params))
            out["log_z"][i] = -(float(tc.sum() + 3 * tk.sum()) + 7 * seed + (cid & 0xFFFF) + (cid >> 32) % 997
                                + crc % 100003) / 7.0
        if self.fail_chain is not None:
            out["status"][self.fail_chain] = _lib.HYG_ENUMERIC
        return out


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("logz"))
    cli_trees.write_inputs(root)
    return root


GRID = ["--omega_case", "0.7,0.8", "--merge_log_prob", "-2.5", "--split_prob", "0.01,0.05", "--minimum_duration", "3,2"]


def _run(inputs, mp, name, extra, fake, data="data", sg="sg"):
    os.makedirs(os.path.join(inputs, name))
    mp.chdir(os.path.join(inputs, name))
    mp.setenv("HYGEIA_PARSE_CACHE", "0")
    mp.setattr(two_group, "filter_chains_host", fake)
    return cli.main(["log_z", "--chroms", "all", "--seeds", "0,5"] + cli_trees.COMMON +
                    ["--data_dir", f"../{data}", "--single_group_dir", f"../{sg}"] + extra)


def test_log_z_command(inputs, monkeypatch):
    fake = FakeFilter()
    assert _run(inputs, monkeypatch, "grid", GRID, fake) == 0
    settings = list(itertools.product((0.7, 0.8), (-2.5,), (0.01, 0.05)))
    tasks = [(c, b) for c, T in cli_trees.CHROMS for b in range(T // 1000 + 1)]
    # one launch per (M, u), in flag order
    assert len(fake.calls) == 4
    launches = [(M, u) for M in (12, 20) for u in (3, 2)]
    # the chains: task x seed x setting with infer's seeds and chain ids, over the chromosomes' sites one after another
    want_chains, want_idx, where = [], [], []
    site0 = 0
    for g, (chrom, T) in enumerate(cli_trees.CHROMS):
        for b in range(T // 1000 + 1):
            (lo, hi), _ = cli.segment_index(T, b, 1000, 50)
            for sd in (0, 5):
                for s in range(len(settings)):
                    want_chains.append((site0 + lo, hi - lo, sd, cli.chain_id(chrom, b), 0))
                    want_idx.append(g * len(settings) + s)
                    where.append((chrom, b, sd, s, hi - lo))
        site0 += T
    thetas = [tuple(cli.control_theta(cli.read_theta(os.path.join(inputs, "sg"), c), 6, c)) for c, _ in cli_trees.CHROMS]
    rows, summary = [], []
    for (M, u), (desc, chains, idx) in zip(launches, fake.calls):
        assert chains == want_chains and idx == want_idx
        assert len(desc) == 2 * len(settings)
        reads = {d[7] for d in desc}
        assert len(reads) == 1  # one common max_total_reads
        for g in range(2):
            for s, (om, mg, sp) in enumerate(settings):
                d = desc[g * len(settings) + s]
                assert d[:6] == (M, u, om, mg, sp, 7) and d[6] == thetas[g]
                assert d[8] == (1100, 1050)[g] + 1  # the chromosome's longest task (a buffer on both sides, one) + 1
    # the files, byte for byte, from the fake's numbers
    replay = FakeFilter()
    assert _run(inputs, monkeypatch, "grid2", GRID, replay) == 0
    for name in ("log_z.tsv", "log_z_summary.tsv"):
        with open(os.path.join(inputs, "grid", "res", name), "rb") as a, \
                open(os.path.join(inputs, "grid2", "res", name), "rb") as b:
            assert a.read() == b.read()
    assert sorted(os.listdir(os.path.join(inputs, "grid", "res"))) == ["log_z.tsv", "log_z_summary.tsv"]
    assert sorted(os.listdir(os.path.join(inputs, "grid"))) == ["res"]
    # the numbers of each launch again, with models built here from the recorded parameters
    lines = ["\t".join(("chrom", "batch", "seed", "num_resampled_particles", "minimum_duration", "omega_case",
                        "merge_log_prob", "split_prob", "n_sites", "log_z"))]
    slines = ["\t".join(("num_resampled_particles", "minimum_duration", "omega_case", "merge_log_prob", "split_prob",
                         "n_tasks", "n_seeds", "sum_log_mean_z"))]
    values = _replay_values(inputs, launches, settings, want_chains, want_idx, thetas, fake.calls)
    for (M, u), lz in zip(launches, values):
        for i, (chrom, b, sd, s, n) in enumerate(where):
            om, mg, sp = settings[s]
            lines.append("\t".join([chrom, str(b), str(sd), str(M), str(u), repr(om), repr(mg), repr(sp), str(n),
                                    repr(float(lz[i]))]))
        per = np.asarray(lz).reshape(len(tasks), 2, len(settings))
        for s, (om, mg, sp) in enumerate(settings):
            terms = []
            for t in range(len(tasks)):
                x = per[t, :, s]
                terms.append(float(x.max()) + math.log(float(np.exp(x - x.max()).sum())) - math.log(2))
            tot = math.fsum(terms)
            slines.append("\t".join([str(M), str(u), repr(om), repr(mg), repr(sp), str(len(tasks)), "2", repr(tot)]))
    with open(os.path.join(inputs, "grid", "res", "log_z.tsv")) as fh:
        assert fh.read() == "\n".join(lines) + "\n"
    with open(os.path.join(inputs, "grid", "res", "log_z_summary.tsv")) as fh:
        assert fh.read() == "\n".join(slines) + "\n"
    assert len(lines) == 1 + 4 * len(tasks) * 2 * len(settings) and len(slines) == 1 + 4 * len(settings)


def _replay_values(inputs, launches, settings, chains, idx, thetas, calls):
    """The fake's log Z of every chain of every launch, from models built here
    with the parameters the command's models were recorded with."""
    tot = {g: np.concatenate([np.loadtxt(os.path.join(inputs, "data", f"n_total_reads_{g}_{c}.txt.gz"), delimiter=",",
                                         ndmin=2) for c, _ in cli_trees.CHROMS]) for g in ("control", "case")}
    mu = np.array([float(x) for x in "0.95,0.05,0.80,0.20,0.50,0.50".split(",")], dtype=np.float32)
    sigma = np.array([float(x) for x in "0.05,0.05,0.1,0.1,0.1,0.2886751".split(",")], dtype=np.float32)
    out = []
    for (M, u), (desc, _, _) in zip(launches, calls):
        models = [two_group.CaseControlModel(mu, sigma, d[6], minimum_duration=d[1], omega_case=d[2],
                                             merge_log_prob=d[3], split_prob=d[4], num_resampled_ancestors=d[0],
                                             num_samples_backward=d[5], max_total_reads=d[7], max_duration=d[8])
                  for d in desc]
        try:
            out.append(FakeFilter()(None, tot, models, chains, chain_model=idx)["log_z"])
        finally:
            for m in models:
                m.close()
    return out


def test_log_z_defaults_are_one_setting(inputs, monkeypatch):
    fake = FakeFilter()
    assert _run(inputs, monkeypatch, "defaults", ["--batches", "0"], fake) == 0
    assert len(fake.calls) == 2  # the two --num_resampled_particles of the common flags
    desc, chains, idx = fake.calls[0]
    assert [d[1:5] for d in desc] == [(3, 0.8, math.log(0.1), 0.01)] * 2
    assert idx == [0, 0, 1, 1] and [c[2] for c in chains] == [0, 5, 0, 5]


@pytest.mark.parametrize("name,extra,kw,message", [
    ("twice", ["--chroms", "21,21"], {}, "--chroms names a chromosome twice"),
    ("bad", [], dict(data="data_bad"), "chromosome 21: methylated reads exceed total reads"),
    ("missing", ["--chroms", "21,X"], dict(sg="sg_missing"), "chromosome X: "),
    ("none", ["--chroms", ""], {}, "no chromosome to run"),
])
def test_log_z_input_errors(inputs, monkeypatch, capsys, name, extra, kw, message):
    fake = FakeFilter()
    assert _run(inputs, monkeypatch, "err_" + name, extra, fake, **kw) == 1
    err = capsys.readouterr().err
    assert err.startswith("hygeia log_z: ") and message in err
    assert fake.calls == [] and os.listdir(os.path.join(inputs, "err_" + name)) == []  # nothing launched or written


def test_log_z_failed_chain_names_its_row(inputs, monkeypatch):
    fake = FakeFilter(fail_chain=5)  # task 21/0, seed 5, second setting of four
    with pytest.raises(_lib.HygError) as e:
        _run(inputs, monkeypatch, "failed", GRID, fake)
    assert e.value.code == _lib.HYG_ENUMERIC
    msg = str(e.value)
    for part in ("chrom=21", "batch=0", "seed=5", "num_resampled_particles=12", "minimum_duration=3", "omega_case=0.7",
                 "merge_log_prob=-2.5", "split_prob=0.05"):
        assert part in msg, msg
    assert os.listdir(os.path.join(inputs, "failed")) == []
