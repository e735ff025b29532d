"""The switch of the forward's fine list walk (hyg_tg_set_fine_list_walk): no device needed.

The 256-thread forward kernels walk a wave's candidate list per 64 entries
unless the process switches that off (the A/B of one binary, and
tests/test_gpu_tg_list_tiers.py, which runs every case both ways). The default
is on; the setter takes any non-zero value as on and never fails.
"""
import pytest

from hygeia_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_on_by_default(lib):
    assert lib.hyg_tg_fine_list_walk() == 1


def test_setter_and_getter(lib):
    try:
        assert lib.hyg_tg_set_fine_list_walk(0) == 0 and lib.hyg_tg_fine_list_walk() == 0
        assert lib.hyg_tg_set_fine_list_walk(7) == 0 and lib.hyg_tg_fine_list_walk() == 1
        assert lib.hyg_tg_set_fine_list_walk(0) == 0 and lib.hyg_tg_set_fine_list_walk(1) == 0
        assert lib.hyg_tg_fine_list_walk() == 1
    finally:
        lib.hyg_tg_set_fine_list_walk(1)
