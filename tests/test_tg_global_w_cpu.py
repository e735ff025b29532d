"""Host-side selection of the global-weights path (no device needed).

A two-group shape keeps its particle arrays in global memory exactly when the
forward's LDS layout at 256 threads exceeds the 160 KiB of a CU
(hyg_tg_global_weights); every shape that fits keeps its layouts and its
workspace size.
"""
import pytest

from hygeia_amd import _lib

LDS_CU = 160 * 1024


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _model(K, M, B=25):
    from hygeia_amd import synthetic as syn
    from hygeia_amd import two_group

    mu, sg = syn.regime_params(K)
    return two_group.CaseControlModel(mu, sg, two_group.uniform_theta(K, 0.8), num_resampled_ancestors=M,
                                      num_samples_backward=B, max_total_reads=300, max_duration=1000)


@pytest.mark.parametrize("K,M,gw", [(6, 50, 0), (12, 50, 0), (13, 50, 1), (6, 200, 1), (16, 256, 1)])
def test_global_weights_diagnostic(lib, K, M, gw):
    m = _model(K, M)
    assert lib.hyg_tg_global_weights(m.handle) == gw
    assert m.global_weights == bool(gw)
    assert lib.hyg_tg_global_weights(None) == 0


def test_boundary_at_m_50(lib):
    """C5 (K = 12, 145 KiB of particle arrays and state) is the last M = 50 shape in LDS."""
    assert lib.hyg_tg_global_weights(_model(12, 50).handle) == 0
    assert lib.hyg_tg_global_weights(_model(13, 50).handle) == 1


@pytest.mark.parametrize("K,M", [(13, 50), (6, 200), (16, 256)])
def test_new_shapes_lds_and_workspace(lib, K, M):
    m = _model(K, M)
    nmax = m.num_particles
    assert nmax == M * (2 * K + K * K)
    for backward in (0, 1):
        assert 0 < lib.hyg_tg_lds_bytes(m.handle, 256, backward) <= LDS_CU
        assert lib.hyg_tg_lds_bytes(m.handle, 512, backward) == 0  # the shape has one width
        assert lib.hyg_tg_lds_bytes(m.handle, 768, backward) == 0
    # one width, whatever the launch size
    assert lib.hyg_tg_threads_per_chain(m.handle, 1) == 256
    assert lib.hyg_tg_threads_per_chain(m.handle, 10000) == 256
    # a per-chain scratch of the weights and the keys
    one, two = (lib.hyg_tg_workspace_bytes(m.handle, n, 1000) for n in (1, 2))
    assert two - one >= 16 * nmax
    assert (two - one) % 256 == 0


def test_forced_width_does_not_move_large_shapes(lib):
    m, m6 = _model(13, 50), _model(6, 50)
    try:
        assert lib.hyg_tg_force_threads(512, 768) == 0
        assert lib.hyg_tg_threads_per_chain(m.handle, 1) == 256
        assert lib.hyg_tg_threads_per_chain(m6.handle, 1) == 512  # (a shape in LDS follows the override)
        assert lib.hyg_tg_force_threads(128, 64) == 0
        assert lib.hyg_tg_threads_per_chain(m.handle, 1) == 256
    finally:
        lib.hyg_tg_force_threads(0, 0)


# Recorded from the parent commit 7d431b9 (hyg_tg_lds_bytes at 256 / 512 / 768,
# forward then backward; hyg_tg_workspace_bytes(m, n, 1000) for n = 1, 2).
EXISTING = {
    (6, 50): dict(fwd=(53648, 54256, 54736), bwd=(37888, 42240, 46592), ws=(832512, 832512)),
    (12, 50): dict(fwd=(152048, 152656, 153136), bwd=(30560, 92640, 96992), ws=(899840, 967168)),
}


@pytest.mark.parametrize("K,M", sorted(EXISTING))
def test_existing_shapes_unchanged(lib, K, M):
    m = _model(K, M)
    want = EXISTING[(K, M)]
    assert tuple(lib.hyg_tg_lds_bytes(m.handle, nt, 0) for nt in (256, 512, 768)) == want["fwd"]
    assert tuple(lib.hyg_tg_lds_bytes(m.handle, nt, 1) for nt in (256, 512, 768)) == want["bwd"]
    assert tuple(lib.hyg_tg_workspace_bytes(m.handle, n, 1000) for n in (1, 2)) == want["ws"]


def _small_model(K, M, B):
    from hygeia_amd import synthetic as syn
    from hygeia_amd import two_group

    mu, sg = syn.regime_params(K)
    return two_group.CaseControlModel(mu, sg, two_group.uniform_theta(K, 0.8), num_resampled_ancestors=M,
                                      num_samples_backward=B, max_total_reads=4, max_duration=8)


@pytest.mark.parametrize("K", range(2, 17))
def test_every_shape_has_a_width_that_fits(lib, K):
    """Every shape the model accepts with M <= 256 is launched at a width whose
    LDS layout exists and fits a CU, forward and backward, for few and many
    chains, automatic or forced: shapes just under the global-weights limit
    (K = 12, M = 54: 163 392 B at 256 threads, 164 000 B at 512) take 256
    threads, as does a forced width with fewer threads than M."""
    n = 0
    for B in (25, 64):
        for M in range(1, 257):
            try:
                m = _small_model(K, M, B)
            except (ValueError, _lib.HygError):
                continue  # not a shape the model accepts
            n += 1
            try:
                for force in ((0, 0), (512, 768), (768, 512), (64, 128)):
                    assert lib.hyg_tg_force_threads(*force) == 0
                    for chains in (1, 100000):
                        nt = lib.hyg_tg_threads_per_chain(m.handle, chains)
                        assert nt in (64, 128, 256, 512, 768) and nt >= M, (K, M, B, force, chains, nt)
                        assert 0 < lib.hyg_tg_lds_bytes(m.handle, nt, 0) <= LDS_CU, (K, M, B, force, chains, nt)
                        nb = lib.hyg_tg_backward_threads_per_chain(m.handle, chains)
                        assert nb in (64, 128, 256, 512, 768) and nb >= M, (K, M, B, force, chains, nb)
                        assert 0 < lib.hyg_tg_lds_bytes(m.handle, nb, 1) <= LDS_CU, (K, M, B, force, chains, nb)
            finally:
                lib.hyg_tg_force_threads(0, 0)
                m.close()
    assert n >= 256  # the scan saw shapes


def test_shape_just_under_the_limit_runs_at_256(lib):
    m = _model(12, 54)
    assert lib.hyg_tg_global_weights(m.handle) == 0
    assert lib.hyg_tg_lds_bytes(m.handle, 256, 0) == 163392 and lib.hyg_tg_lds_bytes(m.handle, 512, 0) == 164000
    assert lib.hyg_tg_threads_per_chain(m.handle, 1) == 256
    assert lib.hyg_tg_threads_per_chain(m.handle, 100000) == 256
    assert lib.hyg_tg_backward_threads_per_chain(m.handle, 1) == 768  # the backward's W alone fits at any width
    one, two = (lib.hyg_tg_workspace_bytes(m.handle, n, 1000) for n in (1, 2))
    assert two == one  # no scratch: the arrays are in LDS
