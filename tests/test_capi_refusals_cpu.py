"""What the chain-launch and kernel-name entries of the C ABI refuse on a host
without a device, case by case against the commit before capi.cpp's host launch
layer was folded into shared helpers (tests/golden/capi_refusals_parent.json,
section no_device, recorded by tests/golden/make_capi_refusals.py): the return
code and the whole message of every case, so which refusals an entry makes
before its device check, and in which order, stay what they were.
"""
import importlib.util
import json
import os

import pytest

from hygeia_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def load_generator():
    spec = importlib.util.spec_from_file_location("make_capi_refusals", os.path.join(GOLDEN, "make_capi_refusals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def differences(section: str, device: bool):
    """The cases whose (code, message) differ from the parent's, as text."""
    with open(os.path.join(GOLDEN, "capi_refusals_parent.json")) as f:
        want = json.load(f)[section]
    got = load_generator().run(_lib.load(), device)
    assert sorted(got) == sorted(want), set(got) ^ set(want)
    assert len(want) > 700
    return [f"{name}: parent {want[name]}, now {got[name]}" for name in want if got[name] != want[name]]


def test_refusals_without_a_device_equal_the_parents():
    if _lib.load().hyg_device_count() > 0:
        pytest.skip("the no_device section is what a host without a GPU answers")
    bad = differences("no_device", False)
    assert not bad, "\n".join(bad)
