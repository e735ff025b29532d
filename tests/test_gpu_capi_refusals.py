"""What the chain-launch and kernel-name entries of the C ABI refuse on the
device, case by case against the commit before capi.cpp's host launch layer was
folded into shared helpers (tests/golden/capi_refusals_parent.json, section
device): the refusals behind an entry's device check -- a workspace one byte
short, a null output buffer, psi_capacity, the estimation settings -- and
n_chains == 0 returning HYG_OK. No case reaches a kernel launch.
"""
import pytest

from tests import test_capi_refusals_cpu as cpu

pytestmark = pytest.mark.gpu


def test_refusals_on_the_device_equal_the_parents():
    bad = cpu.differences("device", True)
    assert not bad, "\n".join(bad)
