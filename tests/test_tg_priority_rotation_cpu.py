"""Rotating wave priorities of the 256-thread forward kernels: the table (no device needed).

With every chain at one priority a SIMD prefers the oldest wave, so the chains of
a CU advance at fixed, unequal rates for a whole launch. The kernels therefore give
each wave a base priority from its wave slot in the SIMD and the epoch of the
device's constant clock (hyg_tg_set_priority_rotation). hyg_tg_priority_base looks
a (clock value, slot) pair up in the table the kernels use. What makes the rotation
fair is checked here on that table: in every epoch the slots 0, 1, 2 hold three
different priorities; over one period every pair of slots leads half of the time
(two chains on a CU) and every slot holds each rank a third of the time (three).
"""
import itertools

import pytest

from hygeia_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _orders(lib, n_epochs, at=0):
    ep = lib.hyg_tg_priority_epoch_ticks()
    return [tuple(lib.hyg_tg_priority_base(e * ep + at, s) for s in range(3)) for e in range(n_epochs)]


def test_epoch_is_short_against_a_chain_and_long_against_a_step(lib):
    """One order lasts 0.1 to 1 ms of 10 ns ticks: tens of forward steps (about
    13 us each), thousands of periods in a 100 000-step chain."""
    ep = lib.hyg_tg_priority_epoch_ticks()
    assert 10_000 <= ep <= 100_000 and ep & (ep - 1) == 0


def test_every_epoch_orders_the_three_slots(lib):
    for o in _orders(lib, 12):
        assert sorted(o) == [0, 1, 2], o


def test_one_period_holds_the_six_orders(lib):
    o = _orders(lib, 12)
    assert set(o[:6]) == set(itertools.permutations(range(3)))
    assert o[6:] == o[:6]


def test_pairs_and_triples_share_alike(lib):
    o = _orders(lib, 6)
    for a, b in itertools.combinations(range(3), 2):  # two chains on a CU, in any two slots
        assert sum(1 for e in o if e[a] > e[b]) == 3, (a, b, o)
    for s in range(3):  # three chains: every rank a third of the time
        assert sorted(e[s] for e in o) == [0, 0, 1, 1, 2, 2], (s, o)


def test_constant_within_an_epoch_and_slots_wrap(lib):
    ep = lib.hyg_tg_priority_epoch_ticks()
    assert _orders(lib, 6, at=0) == _orders(lib, 6, at=ep - 1)
    big = (1 << 63) + 12345  # the clock is 64 bits wide
    for s in range(3):
        assert lib.hyg_tg_priority_base(big, s) == lib.hyg_tg_priority_base(big, s + 3) \
            == lib.hyg_tg_priority_base(big, s + 6)
    assert lib.hyg_tg_priority_base(0, -1) == -1


def test_switch_leaves_the_plan_alone(lib):
    """The switch is a launch parameter of the same kernels: widths and kernel
    names do not depend on it."""
    import ctypes as C

    from hygeia_amd import synthetic, two_group

    K, M, B = 6, 50, 25
    mu, sg = synthetic.regime_params(K)
    model = two_group.CaseControlModel(mu, sg, two_group.uniform_theta(K, 0.8), num_resampled_ancestors=M,
                                       num_samples_backward=B, max_total_reads=200, max_duration=1000)

    def names():
        out = []
        for n in (1, 256, 582, 768):
            for backward in (0, 1):
                need = lib.hyg_tg_kernel_name(model.handle, n, backward, None, 0)
                buf = C.create_string_buffer(need)
                assert lib.hyg_tg_kernel_name(model.handle, n, backward, buf, need) == need
                out.append((buf.value.decode(), int(lib.hyg_tg_threads_per_chain(model.handle, n))))
        return out

    try:
        assert lib.hyg_tg_set_priority_rotation(0) == 0
        off = names()
        assert lib.hyg_tg_set_priority_rotation(1) == 0
        assert names() == off
    finally:
        lib.hyg_tg_set_priority_rotation(1)
