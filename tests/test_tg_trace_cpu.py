"""Traced forward-only launches of the two-group engine (hyg_tg_trace_*), the
part that needs no device: the new symbols, the kernel plan of a traced launch
(the TRC builds), the argument checks, `hygeia filter_genome` and `hygeia log_z
--trimmed` over a fake of two_group.filter_chains_host, and the reference
helper of the GPU tests (tests/tg_trace_ref.py) against the exact enumeration
of the model.
"""
import ast
import ctypes as C
import itertools
import math
import os
import zlib

import numpy as np
import pytest
from scipy.special import logsumexp

from hygeia_amd import _lib, cli, evidence, two_group
from tests import cli_trees, tg_trace_ref
from tests.test_tg_exact import _problem
from tests.test_tg_filter_cpu import PLAN, FakeFilter, _handles, _model, _name, _p
from tests.tg_exact_model import phantom_regime

NEW = ("hyg_tg_trace_chains", "hyg_tg_trace_chains_multi", "hyg_tg_trace_chains_host", "hyg_tg_trace_chains_host_multi",
       "hyg_tg_trace_kernel_name", "hyg_tg_trace_kernel_name_multi")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_new_symbols_exist(lib):
    for name in NEW:
        assert name in _lib.EXPORTS
        getattr(lib, name)
    assert C.sizeof(_lib.TgTrace) == 24
    assert "filter_genome" in cli.COMMANDS.split() and "filter_genome" in cli._SUBCOMMANDS
    assert two_group.TRACES == (None, "log_z", "all")
    assert any(n == "trimmed" and k == "bool" and d is False for n, k, d, _ in evidence.LOGZ_FLAGS)


@pytest.mark.parametrize("shape,force,n,args", PLAN)
def test_trace_kernel_name_pins_the_plan(lib, shape, force, n, args):
    """The forward-only launch's row with a ninth argument, true; the
    forward-only names themselves are what they were."""
    models = [_model(*shape, k=k) for k in range(2)]
    try:
        assert lib.hyg_tg_set_device_cus(0, 256) == 0
        assert lib.hyg_tg_force_threads(force, 0) == 0
        assert _name(lib.hyg_tg_trace_kernel_name, models[0].handle, n) == "tg_forward_kernel<%s,false,false,true>" % args
        assert _name(lib.hyg_tg_trace_kernel_name_multi, _handles(models), 2, n) == \
            "tg_forward_kernel<%s,true,false,true>" % args
        assert _name(lib.hyg_tg_filter_kernel_name, models[0].handle, n) == "tg_forward_kernel<%s,false,false>" % args
        assert _name(lib.hyg_tg_filter_kernel_name_multi, _handles(models), 2, n) == \
            "tg_forward_kernel<%s,true,false>" % args
        full = _name(lib.hyg_tg_kernel_name, models[0].handle, n, 0)
        assert full == "tg_forward_kernel<%s>" % args  # (the full launch's: six arguments)
    finally:
        lib.hyg_tg_force_threads(0, 0)
        lib.hyg_tg_set_device_cus(0, 0)
        for m in models:
            m.close()


def test_trace_plan_follows_the_cu_count(lib):
    m = _model(6, 50, 25)
    try:
        # (256 is also what a host without a device plans for)
        for cus, n, width in ((256, 1, 512), (256, 256, 512), (256, 257, 256)):
            assert lib.hyg_tg_set_device_cus(0, cus) == 0
            assert _name(lib.hyg_tg_trace_kernel_name, m.handle, n) == \
                "tg_forward_kernel<%d,6,50,25,false,false,false,false,true>" % width
            assert _name(lib.hyg_tg_filter_kernel_name, m.handle, n) == \
                "tg_forward_kernel<%d,6,50,25,false,false,false,false>" % width
    finally:
        lib.hyg_tg_set_device_cus(0, 0)
        m.close()


def test_more_than_256_resampled_particles_is_unsupported(lib):
    models = [_model(3, 257, 5, k=k) for k in range(2)]
    try:
        assert lib.hyg_tg_trace_kernel_name(models[0].handle, 5, None, 0) == _lib.HYG_EUNSUPPORTED
        assert "exceeds 256" in lib.hyg_last_error().decode()
        assert lib.hyg_tg_trace_kernel_name_multi(_handles(models), 2, 5, None, 0) == _lib.HYG_EUNSUPPORTED
    finally:
        for m in models:
            m.close()


def _chains(n, T=5, out=None):
    chains = (_lib.TgChain * n)()
    for i in range(n):
        chains[i].n_sites = T
        chains[i].out_begin = i * T if out is None else out[i]
    return chains


def test_argument_errors_are_einval(lib):
    models = [_model(k=0), _model(k=1), _model(k=2, M=5)]
    good = models[:2]
    try:
        chains = _chains(3)
        lz, st, z = np.zeros(3), np.zeros(3, np.int32), np.zeros((5, 1), np.uint16)
        zt, sp, rp = np.zeros(15), np.zeros(15, np.float32), np.zeros((15, 6), np.float32)
        E = np.zeros((5, 6))
        idx = (C.c_int32 * 3)(0, 1, 0)
        big = 1 << 20
        tr = _lib.TgTrace(zt.ctypes.data, None, None)
        none = _lib.TgTrace(None, None, None)
        # no trace, or a trace without an array: that caller wants hyg_tg_filter_chains
        for t in (None, C.byref(none)):
            assert lib.hyg_tg_trace_chains(good[0].handle, chains, 3, _p(E), _p(E), big, t, _p(lz), None, None,
                                           None) == _lib.HYG_EINVAL
            assert "no trace array" in lib.hyg_last_error().decode()
            assert lib.hyg_tg_trace_chains_multi(_handles(good), 2, chains, idx, 3, _p(E), _p(E), big, t, _p(lz), None,
                                                 None, None) == _lib.HYG_EINVAL
            assert "no trace array" in lib.hyg_last_error().decode()
        for fn, head in ((lib.hyg_tg_trace_chains_host, (good[0].handle,)),
                         (lib.hyg_tg_trace_chains_host_multi, (_handles(good), 2))):
            tail = (idx,) if len(head) == 2 else ()
            args = head + (_p(z), _p(z), 1, _p(z), _p(z), 1, 5, chains) + tail
            assert fn(*args, 3, 15, None, None, None, _p(lz), None, _p(st)) == _lib.HYG_EINVAL
            assert "no trace array" in lib.hyg_last_error().decode()
            # out_begin + T beyond out_rows, a negative out_begin: before anything runs
            assert fn(*args, 3, 14, _p(zt), _p(sp), _p(rp), _p(lz), None, _p(st)) == _lib.HYG_EINVAL
            assert "chain outside the output rows" in lib.hyg_last_error().decode()
            neg = head + (_p(z), _p(z), 1, _p(z), _p(z), 1, 5, _chains(3, out=[0, -1, 5])) + tail
            assert fn(*neg, 3, 15, _p(zt), None, None, _p(lz), None, _p(st)) == _lib.HYG_EINVAL
            assert "chain outside the output rows" in lib.hyg_last_error().decode()
        # a workspace one byte short of hyg_tg_filter_workspace_bytes[_multi]
        need = lib.hyg_tg_filter_workspace_bytes(good[0].handle, 3)
        assert lib.hyg_tg_trace_chains(good[0].handle, chains, 3, _p(E), _p(E), need - 1, C.byref(tr), _p(lz), None,
                                       None, None) == _lib.HYG_EINVAL
        assert "workspace too small" in lib.hyg_last_error().decode()
        need = lib.hyg_tg_filter_workspace_bytes_multi(_handles(good), 2, 3)
        assert lib.hyg_tg_trace_chains_multi(_handles(good), 2, chains, idx, 3, _p(E), _p(E), need - 1, C.byref(tr),
                                             _p(lz), None, None, None) == _lib.HYG_EINVAL
        assert "workspace too small" in lib.hyg_last_error().decode()
        # incompatible models, a model index out of range, null model, negative length: as the filter entries
        assert lib.hyg_tg_trace_kernel_name_multi(_handles(models), 3, 3, None, 0) == _lib.HYG_EINVAL
        assert "differ in num_resampled_ancestors:" in lib.hyg_last_error().decode()
        assert lib.hyg_tg_trace_chains_multi(_handles(models), 3, chains, idx, 3, _p(E), _p(E), big, C.byref(tr), _p(lz),
                                             None, None, None) == _lib.HYG_EINVAL
        bidx = (C.c_int32 * 3)(0, 1, 2)
        assert lib.hyg_tg_trace_chains_multi(_handles(good), 2, chains, bidx, 3, _p(E), _p(E), big, C.byref(tr), _p(lz),
                                             None, None, None) == _lib.HYG_EINVAL
        assert "chain_model[2] = 2" in lib.hyg_last_error().decode()
        assert lib.hyg_tg_trace_chains(None, chains, 3, _p(E), _p(E), big, C.byref(tr), _p(lz), None, None,
                                       None) == _lib.HYG_EINVAL
        assert lib.hyg_tg_trace_kernel_name(None, 3, None, 0) == _lib.HYG_EINVAL
        assert lib.hyg_tg_trace_kernel_name(good[0].handle, 3, None, -1) == _lib.HYG_EINVAL
        # the Python layer
        obs = ({"control": z, "case": z}, {"control": z, "case": z})
        with pytest.raises(ValueError):
            two_group.filter_chains_host(*obs, good[0], [(0, 5, 0, 0, 0)], trace="everything", n_out_rows=5)
        with pytest.raises(ValueError):
            two_group.filter_chains_host(*obs, good[0], [(0, 5, 0, 0, 0)], trace="log_z")  # no n_out_rows
        with pytest.raises(ValueError):
            two_group.filter_chains_host(*obs, good[0], [(0, 5, 0, 0, 0)], n_out_rows=5)  # rows without a trace
        with pytest.raises(ValueError):  # overlapping rows
            two_group.filter_chains_host(*obs, good[0], [(0, 5, 0, 0, 0), (0, 5, 1, 0, 4)], trace="all", n_out_rows=10)
        with pytest.raises(ValueError):  # rows past the end
            two_group.filter_chains_host(*obs, good[0], [(0, 5, 0, 0, 1)], trace="all", n_out_rows=5)
    finally:
        for m in models:
            m.close()


def test_compute_entries_refuse_without_device(lib):
    if lib.hyg_device_count() > 0:
        pytest.skip("host without a GPU only")
    models = [_model(k=0), _model(k=1)]
    try:
        chains = _chains(2)
        lz, st, z = np.zeros(2), np.zeros(2, np.int32), np.zeros((5, 1), np.uint16)
        zt = np.zeros(10)
        E = np.zeros((5, 6))
        idx = (C.c_int32 * 2)(0, 1)
        tr = _lib.TgTrace(zt.ctypes.data, None, None)
        rcs = [lib.hyg_tg_trace_chains(models[0].handle, chains, 2, _p(E), _p(E), 1 << 20, C.byref(tr), _p(lz), None,
                                       None, None),
               lib.hyg_tg_trace_chains_multi(_handles(models), 2, chains, idx, 2, _p(E), _p(E), 1 << 20, C.byref(tr),
                                             _p(lz), None, None, None),
               lib.hyg_tg_trace_chains_host(models[0].handle, _p(z), _p(z), 1, _p(z), _p(z), 1, 5, chains, 2, 10,
                                            _p(zt), None, None, _p(lz), None, _p(st)),
               lib.hyg_tg_trace_chains_host_multi(_handles(models), 2, _p(z), _p(z), 1, _p(z), _p(z), 1, 5, chains, idx,
                                                  2, 10, _p(zt), None, None, _p(lz), None, _p(st))]
        assert rcs == [_lib.HYG_EDEVICE] * 4
        assert b"no CPU fallback" in lib.hyg_last_error()
        with pytest.raises(_lib.HygError) as e:
            two_group.filter_chains_host({"control": z, "case": z}, {"control": z, "case": z}, models,
                                         [(0, 5, 0, 1, 0), (0, 5, 0, 2, 5)], chain_model=[1, 0], trace="all",
                                         n_out_rows=10)
        assert e.value.code == _lib.HYG_EDEVICE
    finally:
        for m in models:
            m.close()


# ------------------------------------------------- the commands over a fake
def _site_term(tc, tk):
    tc, tk = (np.asarray(a).reshape(len(a), -1).astype(np.int64) for a in (tc, tk))
    return -(tc.sum(1) + 3 * tk.sum(1) + 1) / 8.0  # (dyadic: the sums below are exact)


class FakeTrace:
    """two_group.filter_chains_host with its trace keywords, without a device:
    a chain's log Z_t is an offset (its seed, its chain id, its model) plus the
    running sum of a per-site term of its own total-read rows; its
    probabilities are functions of the same. `calls` records (trace, n_out_rows,
    n_chains, chains, chain_model, models' descriptions)."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def offset(seed, cid, model):
        return -((7 * seed + (cid & 0xFFFF) + (cid >> 32) % 997 + zlib.crc32(bytes(model.params)) % 1009) / 4.0)

    def __call__(self, observations, n_total_reads, model, chains, final_weights=False, chain_model=None, trace=None,
                 n_out_rows=None):
        models = list(model)
        assert chain_model is not None and not final_weights
        self.calls.append((trace, n_out_rows, len(chains), [tuple(int(x) for x in c) for c in chains],
                           [int(k) for k in chain_model],
                           [(m.params.num_resampled_ancestors, m.params.num_samples_backward, m.max_duration)
                            for m in models]))
        n, K = len(chains), models[0].n_regimes
        out = {"log_z": np.zeros(n), "status": np.zeros(n, np.int32)}
        if trace is not None:
            out["log_z_t"] = np.full(int(n_out_rows), np.nan)
            if trace == "all":
                out["split_probs"] = np.full(int(n_out_rows), np.nan, np.float32)
                out["regime_probs"] = np.full((int(n_out_rows), 2 * K), np.nan, np.float32)
        for i, (s0, T, seed, cid, o0) in enumerate(chains):
            term = _site_term(n_total_reads["control"][s0:s0 + T], n_total_reads["case"][s0:s0 + T])
            L = self.offset(seed, cid, models[chain_model[i]]) + np.cumsum(term)
            out["log_z"][i] = L[-1]
            if trace is not None:
                out["log_z_t"][o0:o0 + T] = L
            if trace == "all":
                out["split_probs"][o0:o0 + T] = ((-term * 8) % 97 / 97.0).astype(np.float32)
                out["regime_probs"][o0:o0 + T] = (out["split_probs"][o0:o0 + T, None] +
                                                  np.arange(2 * K, dtype=np.float32)[None, :])
        return out


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """cli_trees' two chromosomes (2400 and 1300 sites) and one of 2000 sites,
    a multiple of --segment_size 1000: its last task's return range is empty."""
    root = str(tmp_path_factory.mktemp("trace"))
    cli_trees.write_inputs(root)
    cli_trees._write_chrom(root, "5", 2000, 2)
    return root


LENGTHS = dict(cli_trees.CHROMS, **{"5": 2000})
ORDER = ["5", "21", "X"]  # --chroms all: numbered chromosomes in numeric order, then by name


def _run(inputs, mp, name, argv, fake):
    os.makedirs(os.path.join(inputs, name))
    mp.chdir(os.path.join(inputs, name))
    mp.setenv("HYGEIA_PARSE_CACHE", "0")
    mp.setattr(two_group, "filter_chains_host", fake)
    return cli.main(argv + ["--chroms", "all", "--seeds", "0,5"] + cli_trees.COMMON +
                    ["--data_dir", "../data", "--single_group_dir", "../sg"])


def _totals(inputs, chrom):
    return [np.loadtxt(os.path.join(inputs, "data", f"n_total_reads_{g}_{chrom}.txt.gz"), delimiter=",", ndmin=2)
            for g in ("control", "case")]


def test_filter_genome_command(inputs, monkeypatch):
    fake = FakeTrace()
    assert _run(inputs, monkeypatch, "fg", ["filter_genome"], fake) == 0
    tasks = [(c, b) for c in ORDER for b in range(LENGTHS[c] // 1000 + 1)]
    assert [c[:3] for c in fake.calls] == [("all", sum(hi - lo for c, b in tasks for (lo, hi), _ in
                                                         [cli.segment_index(LENGTHS[c], b, 1000, 50)]) * 2, 2 * len(tasks))] * 2
    assert [c[5][0][:2] for c in fake.calls] == [(12, 7), (20, 7)]  # one launch per --num_resampled_particles
    # chains: task x seed over the chromosomes' sites one after another, rows one after another
    want, site0, out = [], 0, 0
    for g, chrom in enumerate(ORDER):
        for b in range(LENGTHS[chrom] // 1000 + 1):
            (lo, hi), _ = cli.segment_index(LENGTHS[chrom], b, 1000, 50)
            for sd in (0, 5):
                want.append((site0 + lo, hi - lo, sd, cli.chain_id(chrom, b), out))
                out += hi - lo
        site0 += LENGTHS[chrom]
    assert fake.calls[0][3] == want and fake.calls[0][4] == [ORDER.index(c) for c, b in tasks for _ in (0, 5)]
    res = os.path.join(inputs, "fg", "res")
    assert sorted(os.listdir(res)) == sorted(f"chrom_{c}_{b}" for c, b in tasks)
    for chrom, b in tasks:
        d = os.path.join(res, f"chrom_{chrom}_{b}")
        names = ["flags%d.txt" % sd for sd in (0, 5)] + ["log_normalizing_constants_optimal_%d.txt" % sd for sd in (0, 5)]
        names += ["filter_%s_%d_%d.npz" % (k, N, sd) for k in ("split_probs", "regime_probs", "log_z")
                  for N in (12 * 48, 20 * 48) for sd in (0, 5)]
        assert sorted(os.listdir(d)) == sorted(names)
        (lo, hi), _ = cli.segment_index(LENGTHS[chrom], b, 1000, 50)
        tc, tk = (a[lo:hi] for a in _totals(inputs, chrom))
        term = _site_term(tc, tk)
        for sd in (0, 5):
            with open(os.path.join(d, f"flags{sd}.txt")) as fh:
                flags = fh.read().split("\n")
            assert f"--chrom={chrom}" in flags and f"--batch={b}" in flags and f"--seed={sd}" in flags
            with open(os.path.join(d, f"log_normalizing_constants_optimal_{sd}.txt")) as fh:
                lz = ast.literal_eval(fh.read())
            assert sorted(lz) == [12 * 48, 20 * 48]
            for N in (12 * 48, 20 * 48):
                got = {}
                for k in ("split_probs", "regime_probs", "log_z"):
                    with np.load(os.path.join(d, f"filter_{k}_{N}_{sd}.npz")) as zf:
                        assert zf.files == ["arr_0"]
                        got[k] = zf["arr_0"]
                # every row of the task, buffers included
                assert got["split_probs"].shape == (hi - lo,) and got["split_probs"].dtype == np.float32
                assert got["regime_probs"].shape == (hi - lo, 12) and got["regime_probs"].dtype == np.float32
                assert got["log_z"].shape == (hi - lo,) and got["log_z"].dtype == np.float64
                np.testing.assert_array_equal(got["split_probs"], ((-term * 8) % 97 / 97.0).astype(np.float32))
                np.testing.assert_array_equal(np.diff(got["log_z"]), np.diff(got["log_z"][0] - term[0] + np.cumsum(term)))
                assert lz[N] == got["log_z"][-1]
    # the two launches differ by their models alone
    a = np.load(os.path.join(res, "chrom_21_1", "filter_log_z_576_5.npz"))["arr_0"]
    b = np.load(os.path.join(res, "chrom_21_1", "filter_log_z_960_5.npz"))["arr_0"]
    assert a[0] != b[0]


def test_log_z_trimmed(inputs, monkeypatch):
    grid = ["--omega_case", "0.7,0.8", "--split_prob", "0.01,0.05", "--minimum_duration", "3,2"]
    plain = FakeTrace()
    assert _run(inputs, monkeypatch, "plain", ["log_z"] + grid, plain) == 0
    # without the flag: the launches of before, no trace keyword in use
    assert len(plain.calls) == 4 and all(c[0] is None and c[1] is None for c in plain.calls)
    assert all(ch[4] == 0 for c in plain.calls for ch in c[3])
    assert sorted(os.listdir(os.path.join(inputs, "plain", "res"))) == ["log_z.tsv", "log_z_summary.tsv"]
    # ... through the very call the command made before: a fake without the keywords
    old = FakeFilter()
    assert _run(inputs, monkeypatch, "old", ["log_z"] + grid, old) == 0 and len(old.calls) == 4
    fake = FakeTrace()
    assert _run(inputs, monkeypatch, "trimmed", ["log_z", "--trimmed"] + grid, fake) == 0
    assert sorted(os.listdir(os.path.join(inputs, "trimmed", "res"))) == [
        "log_z.tsv", "log_z_summary.tsv", "log_z_trimmed.tsv", "log_z_trimmed_summary.tsv"]
    for name in ("log_z.tsv", "log_z_summary.tsv"):
        with open(os.path.join(inputs, "plain", "res", name), "rb") as a, \
                open(os.path.join(inputs, "trimmed", "res", name), "rb") as b:
            assert a.read() == b.read()
    settings = list(itertools.product((0.7, 0.8), (math.log(0.1),), (0.01, 0.05)))
    tasks = [(c, b) for c in ORDER for b in range(LENGTHS[c] // 1000 + 1)]
    n_rows = sum(hi - lo for c, b in tasks for (lo, hi), _ in [cli.segment_index(LENGTHS[c], b, 1000, 50)])
    assert [c[:3] for c in fake.calls] == [("log_z", n_rows * 2 * 4, len(tasks) * 2 * 4)] * 4
    # the same chains as without the flag, their rows one after another
    for c, q in zip(fake.calls, plain.calls):
        assert [ch[:4] for ch in c[3]] == [ch[:4] for ch in q[3]] and c[4] == q[4]
        assert [ch[4] for ch in c[3]] == list(np.cumsum([0] + [ch[1] for ch in c[3]][:-1]))
    # the trimmed ranges tile each chromosome; the chromosome of 2000 sites ends on an empty one
    ranges = {}
    for chrom, b in tasks:
        (lo, hi), (r0, r1) = cli.segment_index(LENGTHS[chrom], b, 1000, 50)
        ranges[(chrom, b)] = (lo, hi, r0, max(r0, r1))
    for chrom in ORDER:
        own = [ranges[(c, b)] for c, b in tasks if c == chrom]
        assert sum(r1 - r0 for _, _, r0, r1 in own) == LENGTHS[chrom]
        assert [lo + r0 for lo, _, r0, _ in own[1:]] == [lo + r1 for lo, _, _, r1 in own[:-1]]  # each starts where the last ended
    assert ranges[("5", 2)][2:] == (50, 50)
    with open(os.path.join(inputs, "trimmed", "res", "log_z_trimmed.tsv")) as fh:
        head, *rows = [line.rstrip("\n").split("\t") for line in fh]
    assert head == ["chrom", "batch", "seed", "num_resampled_particles", "minimum_duration", "omega_case",
                    "merge_log_prob", "split_prob", "n_trimmed_sites", "log_z_increment"]
    assert len(rows) == 4 * len(tasks) * 2 * 4
    inc = {}
    launches = [(M, u) for M in (12, 20) for u in (3, 2)]
    it = iter(rows)
    for M, u in launches:
        for chrom, b in tasks:
            lo, hi, r0, r1 = ranges[(chrom, b)]
            tc, tk = (a[lo:hi] for a in _totals(inputs, chrom))
            term = _site_term(tc, tk)
            for sd in (0, 5):
                for s, (om, mg, sp) in enumerate(settings):
                    row = next(it)
                    assert row[:9] == [chrom, str(b), str(sd), str(M), str(u), repr(om), repr(mg), repr(sp), str(r1 - r0)]
                    # L[r1 - 1] - L[r0 - 1], or L[r1 - 1] itself from the chain's first row; 0 on an empty range
                    if r1 == r0:
                        want = 0.0
                    elif r0 > 0:
                        want = float(term[r0:r1].sum())
                    else:
                        assert float(row[9]) != float(term[:r1].sum())  # (the chain's offset is in it)
                        want = None
                    if want is not None:
                        assert float(row[9]) == want, (chrom, b, sd, s)
                    inc[(M, u, chrom, b, sd, s)] = float(row[9])
    assert inc[(12, 3, "5", 2, 0, 0)] == 0.0
    with open(os.path.join(inputs, "trimmed", "res", "log_z_trimmed_summary.tsv")) as fh:
        head, *srows = [line.rstrip("\n").split("\t") for line in fh]
    assert head == ["num_resampled_particles", "minimum_duration", "omega_case", "merge_log_prob", "split_prob",
                    "n_tasks", "n_seeds", "n_trimmed_sites", "sum_log_mean_z_increment"]
    assert len(srows) == 4 * len(settings)
    it = iter(srows)
    for M, u in launches:
        for s, (om, mg, sp) in enumerate(settings):
            row = next(it)
            assert row[:8] == [str(M), str(u), repr(om), repr(mg), repr(sp), str(len(tasks)), "2",
                               str(sum(LENGTHS.values()))]
            want = math.fsum(evidence.log_mean_exp(np.array([inc[(M, u, c, b, sd, s)] for sd in (0, 5)]))
                             for c, b in tasks)
            assert float(row[8]) == want


# ------------------------------------- the reference helper, independently
@pytest.mark.parametrize("K,dseed", [(2, 31), (3, 32)])
def test_reference_rows_against_the_exact_filter(oracle, K, dseed):
    """In the keep-all regime the particle set is every path, so the helper's
    rows are the exact filter: log Z_t = logsumexp(alpha_t) to 1e-12, the
    marginals of alpha_t to 1e-6 (they are f32)."""
    T, u, M = 8, 2, {2: 256, 3: 4096}[K]  # above the largest finite particle count (136, 3442)
    p, ex, E, E_ex = _problem(oracle, K, T, dseed, M=M, B=4, u=u)
    seen = set()
    for seed in range(4):
        cid = 70 + seed
        full = oracle.chain(p, E, seed, cid, want_modes=True)
        assert full["status"] == 0
        assert np.all(full["modes"][1:] // 65536 == 0), "M too small for the keep-all regime"
        r_ph = phantom_regime(oracle, seed, cid, K)
        seen.add(r_ph)
        _, alphas, _, _ = ex.forward_backward(E_ex, r_ph)
        ref = tg_trace_ref.rows(p, E, range(T), seed, cid)
        assert ref["rows"].tolist() == list(range(T))
        assert ref["log_z_t"].dtype == np.float64 and ref["split_probs"].dtype == np.float32
        assert ref["regime_probs"].shape == (T, 2 * K) and ref["regime_probs"].dtype == np.float32
        assert ref["log_z_t"][T - 1] == full["log_z"]
        for t in range(T):
            lz = logsumexp(list(alphas[t].values()))
            assert abs(ref["log_z_t"][t] - lz) < 1e-12 * max(1.0, abs(lz)), (t, ref["log_z_t"][t], lz)
            split, regime = 0.0, np.zeros(2 * K)
            for (m, _, rc, _, rk), a in alphas[t].items():
                w = math.exp(a - lz)
                split += w if m == 0 else 0.0
                regime[rc] += w
                regime[K + rk] += w
            assert abs(float(ref["split_probs"][t]) - split) < 1e-6, (t, ref["split_probs"][t], split)
            np.testing.assert_allclose(ref["regime_probs"][t], regime, rtol=0, atol=1e-6)
    assert len(seen) >= 2


def test_row_set():
    modes = np.array([3, 0, 0, 1, 1, 1, 1, 1, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1])
    assert tg_trace_ref.row_set(modes) == [0, 1, 2, 3, 4, 5, 8, 9, 10, 15, 17]
    assert tg_trace_ref.row_set(modes, every=True) == list(range(18))
