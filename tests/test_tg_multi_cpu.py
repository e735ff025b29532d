"""Multi-model launches of the two-group engine, the part that needs no device:
which models may share a launch (hyg_tg_models_compatible), the workspace
bound, the kernel plan of a multi-model launch against the single-model plan
of the same shape and chain count, and the refusal of a bad per-chain model
index before anything is enqueued.
"""
import ctypes as C

import numpy as np
import pytest

from hygeia_amd import _lib, synthetic as syn, two_group


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _theta(K, k):
    """A theta that differs from model to model (k = 0: the uniform one)."""
    rng = np.random.default_rng(100 + k)
    th = two_group.uniform_theta(K, 0.8)
    return th + (rng.normal(0.0, 0.7, th.shape) if k else 0.0)


def _model(K=3, M=4, B=5, k=0, mu=None, sigma=None, max_total_reads=40, max_duration=151, **kw):
    m0, s0 = syn.regime_params(K)
    return two_group.CaseControlModel(m0 if mu is None else mu, s0 if sigma is None else sigma, _theta(K, k),
                                      num_resampled_ancestors=M, num_samples_backward=B,
                                      max_total_reads=max_total_reads, max_duration=max_duration, **kw)


def _handles(models):
    return (C.c_void_p * len(models))(*[m.handle for m in models])


def _close(models):
    for m in models:
        m.close()


def test_models_that_differ_in_theta_and_durations_are_compatible(lib):
    models = [_model(k=0), _model(k=1, omega_case=0.7, split_prob=0.02, max_duration=1000),
              _model(k=2, max_duration=300, merge_log_prob=np.log(0.2), kappa_control=3.0, kappa_case=2.5)]
    try:
        assert lib.hyg_tg_models_compatible(_handles(models), 3) == _lib.HYG_OK
        assert lib.hyg_tg_models_compatible(_handles(models[:1]), 1) == _lib.HYG_OK
    finally:
        _close(models)


def _other_mu(entry):
    mu, _ = syn.regime_params(3)
    mu = list(mu)
    mu[entry] = float(np.nextafter(mu[entry], 1.0))  # one bit of one entry
    return mu


@pytest.mark.parametrize("field,kw", [
    ("n_regimes", dict(K=4)),
    ("num_resampled_ancestors", dict(M=5)),
    ("num_samples_backward", dict(B=6)),
    ("minimum_duration", dict(minimum_duration=2)),
    ("max_total_reads", dict(max_total_reads=41)),
    ("mu", dict(mu=_other_mu(1))),
])
def test_incompatible_models_are_refused_with_the_field_named(lib, field, kw):
    models = [_model(), _model(k=1), _model(k=2, **kw)]
    try:
        assert lib.hyg_tg_models_compatible(_handles(models), 3) == _lib.HYG_EINVAL
        msg = lib.hyg_last_error().decode()
        assert msg.startswith("models 0 and 2 differ in %s:" % field), msg
        assert lib.hyg_tg_models_compatible(_handles(models), 2) == _lib.HYG_OK  # the first two agree
        # every entry point that takes the models refuses them the same way
        assert lib.hyg_tg_kernel_name_multi(_handles(models), 3, 10, 0, None, 0) == _lib.HYG_EINVAL
        assert "differ in %s:" % field in lib.hyg_last_error().decode()
        chain = (_lib.TgChain * 1)()
        chain[0].n_sites = 5
        idx = (C.c_int32 * 1)(0)
        out = _lib.TgOutputs()
        assert lib.hyg_tg_run_chains_multi(_handles(models), 3, chain, idx, 1, None, None, 0, C.byref(out),
                                           None) == _lib.HYG_EINVAL
        assert "differ in %s:" % field in lib.hyg_last_error().decode()
    finally:
        _close(models)


def test_no_models_or_a_null_entry_is_refused(lib):
    m = _model()
    try:
        assert lib.hyg_tg_models_compatible(_handles([m]), 0) == _lib.HYG_EINVAL
        assert lib.hyg_tg_models_compatible(None, 1) == _lib.HYG_EINVAL
        h = (C.c_void_p * 2)(m.handle, None)
        assert lib.hyg_tg_models_compatible(h, 2) == _lib.HYG_EINVAL
        assert "null model 1" in lib.hyg_last_error().decode()
    finally:
        m.close()


@pytest.mark.parametrize("shape", [(3, 4, 5), (6, 50, 25), (12, 50, 25), (13, 50, 25)])
def test_workspace_bound(lib, shape):
    K, M, B = shape
    models = [_model(K, M, B, k=k) for k in range(3)]
    try:
        h = _handles(models)
        single = lib.hyg_tg_workspace_bytes(models[0].handle, 7, 1050)
        sizes = []
        for force in ((0, 0), (64, 64), (256, 256), (512, 768)):
            assert lib.hyg_tg_force_threads(*force) == 0
            assert lib.hyg_tg_workspace_bytes(models[0].handle, 7, 1050) == single
            sizes.append(lib.hyg_tg_workspace_bytes_multi(h, 3, 7, 1050))
        assert len(set(sizes)) == 1  # no forced width moves it
        assert single <= sizes[0] <= single + 256 * 3  # the table: a few hundred bytes
        assert lib.hyg_tg_workspace_bytes_multi(h, 1, 7, 1050) >= single
        assert lib.hyg_tg_workspace_bytes_multi(h, 0, 7, 1050) == 0
        assert lib.hyg_tg_workspace_bytes_multi(None, 3, 7, 1050) == 0
    finally:
        lib.hyg_tg_force_threads(0, 0)
        _close(models)


def _name(fn, *args):
    need = fn(*args, None, 0)
    assert need > 1, _lib.load().hyg_last_error()
    buf = C.create_string_buffer(need)
    assert fn(*args, buf, need) == need
    return buf.value.decode()


# the shapes with builds of their own, a generic one, GW ones (K = 13; M = 200), one that fits at 256 only
SHAPES = [(3, 4, 5), (6, 50, 25), (12, 50, 25), (6, 50, 64), (13, 50, 25), (6, 200, 5), (12, 54, 25)]
# rows the multi-model ladder holds as compiled-shape builds: (direction, width, K, GW)
MM_SHAPE_ROWS = {("tg_forward_kernel", nt, K, "false") for nt in (256, 512, 768) for K in (6, 12)
                 if (nt, K) != (256, 12)} | \
                {("tg_backward_kernel", nt, K, "false") for nt in (256, 512, 768) for K in (6, 12)
                 if (nt, K) != (256, 12)} | {("tg_backward_kernel", 256, 12, "true")}


@pytest.mark.parametrize("shape", SHAPES)
def test_multi_plan_is_the_single_plan_of_the_same_launch(lib, shape):
    """Width and GW flag of hyg_tg_kernel_name_multi equal hyg_tg_kernel_name's
    over chain counts around the CU count of a (pretended) 4-CU device and
    forced widths; the name carries the seventh argument, no phase timers, and
    the compiled shape wherever the multi-model ladder has that build."""
    K, M, B = shape
    models = [_model(K, M, B, k=k) for k in range(2)]
    dev = 0
    try:
        h = _handles(models)
        assert lib.hyg_tg_set_device_cus(dev, 4) == 0
        for force in ((0, 0), (64, 128), (256, 256), (512, 768), (768, 512)):
            assert lib.hyg_tg_force_threads(*force) == 0
            for n in (1, 3, 4, 5, 9, 100000):
                for backward in (0, 1):
                    one = _name(lib.hyg_tg_kernel_name, models[0].handle, n, backward)
                    multi = _name(lib.hyg_tg_kernel_name_multi, h, 2, n, backward)
                    kern, a = one.rstrip(">").split("<")
                    kern_m, b = multi.rstrip(">").split("<")
                    a, b = a.split(","), b.split(",")
                    assert kern_m == kern and len(a) == 6 and len(b) == 7
                    assert b[0] == a[0] and b[5] == a[5], (force, n, one, multi)  # width, GW
                    assert b[4] == "false" and b[6] == "true"
                    if (kern, int(a[0]), int(a[1]), a[5]) in MM_SHAPE_ROWS:
                        assert b[1:4] == a[1:4], (one, multi)
                    else:
                        assert b[1:4] == ["0", "0", "0"], (one, multi)
    finally:
        lib.hyg_tg_force_threads(0, 0)
        lib.hyg_tg_set_device_cus(dev, 0)
        _close(models)


def test_required_multi_rows_exist(lib):
    """The compiled-shape builds the issue asks for are reached."""
    dev = 0
    want = {(6, 50, 25): {(0, 0, 1): ("512,6,50,25", "768,6,50,25"), (0, 0, 100000): ("256,6,50,25", "256,6,50,25"),
                          (768, 512, 1): ("768,6,50,25", "512,6,50,25")},
            (12, 50, 25): {(0, 0, 1): ("512,12,50,25", "768,12,50,25"),
                           (0, 0, 100000): ("512,12,50,25", "256,12,50,25"),
                           (768, 512, 1): ("768,12,50,25", "512,12,50,25")}}
    try:
        assert lib.hyg_tg_set_device_cus(dev, 4) == 0
        for shape, cases in want.items():
            models = [_model(*shape, k=k) for k in range(2)]
            try:
                for (ff, fb, n), (f, b) in cases.items():
                    assert lib.hyg_tg_force_threads(ff, fb) == 0
                    fwd = _name(lib.hyg_tg_kernel_name_multi, _handles(models), 2, n, 0)
                    bwd = _name(lib.hyg_tg_kernel_name_multi, _handles(models), 2, n, 1)
                    assert fwd == "tg_forward_kernel<%s,false,false,true>" % f
                    gw = "true" if b == "256,12,50,25" else "false"
                    assert bwd == "tg_backward_kernel<%s,false,%s,true>" % (b, gw)
            finally:
                _close(models)
    finally:
        lib.hyg_tg_force_threads(0, 0)
        lib.hyg_tg_set_device_cus(dev, 0)


def test_bad_chain_model_index_is_einval(lib):
    models = [_model(k=k) for k in range(2)]
    try:
        chains = (_lib.TgChain * 3)()
        for i in range(3):
            chains[i].n_sites, chains[i].out_begin = 5, 5 * i
        out = _lib.TgOutputs()
        for bad in (2, -1):
            idx = (C.c_int32 * 3)(0, 1, bad)
            rc = lib.hyg_tg_run_chains_multi(_handles(models), 2, chains, idx, 3, None, None, 0, C.byref(out), None)
            assert rc == _lib.HYG_EINVAL
            assert "chain_model[2] = %d" % bad in lib.hyg_last_error().decode()
            z = np.zeros((5, 1), np.uint16)
            o = {k: np.zeros(64, np.float64) for k in "abcdefg"}
            p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
            rc = lib.hyg_tg_run_chains_host_multi(_handles(models), 2, p(z), p(z), 1, p(z), p(z), 1, 5, chains, idx, 3,
                                                  15, p(o["a"]), p(o["b"]), p(o["c"]), p(o["d"]), p(o["e"]),
                                                  p(o["f"]), None, p(o["g"]))
            assert rc == _lib.HYG_EINVAL
            assert "chain_model[2] = %d" % bad in lib.hyg_last_error().decode()
        assert lib.hyg_tg_run_chains_multi(_handles(models), 2, chains, None, 3, None, None, 0, C.byref(out),
                                           None) == _lib.HYG_EINVAL
        with pytest.raises(ValueError):
            two_group._models_of(models, [0, 1, 2], 3)
        with pytest.raises(ValueError):
            two_group._models_of(models, None, 3)
    finally:
        _close(models)
