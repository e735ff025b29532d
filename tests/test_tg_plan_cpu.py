"""The two-group launcher's kernel plan (no device needed): which width, LDS
layout and kernel instantiation a launch gets.

The selection is pinned against the commit before the launcher was rewritten
around one plan per launch: tests/golden/tg_plan_parent.json holds what that
commit's library reported over a scan of shapes, forced widths and launch sizes
(tests/golden/make_tg_plan.py), and NAMES below what its instantiation ladder
returned (printed by a throwaway fprintf in that commit's fwd_kernel /
bwd_kernel, which had no entry point for it).
"""
import ctypes as C
import importlib.util
import json
import os
import re

import pytest

from hygeia_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _load_generator():
    spec = importlib.util.spec_from_file_location("make_tg_plan", os.path.join(GOLDEN, "make_tg_plan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _load_generator()


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def kernel_name(lib, model, n_chains, backward):
    need = lib.hyg_tg_kernel_name(model.handle, n_chains, backward, None, 0)
    assert need > 1, lib.hyg_last_error()
    buf = C.create_string_buffer(need)
    assert lib.hyg_tg_kernel_name(model.handle, n_chains, backward, buf, need) == need
    return buf.value.decode()


@pytest.fixture(scope="module")
def listed_kernels():
    """The instantiations of the built library (the committed resource notes)."""
    with open(os.path.join(ROOT, "profiles", "gw_resource_notes_after.txt")) as f:
        names = [line.split()[0] for line in f.read().splitlines()[1:] if line.strip()]
    assert len(names) == 37
    return set(names)


def test_selection_equals_parent_and_names_are_consistent(lib, listed_kernels):
    """One pass over the scan: the rows equal the parent's, and every case's
    kernel names are built instantiations of the reported width whose forward
    GW flag is hyg_tg_global_weights."""
    with open(os.path.join(GOLDEN, "tg_plan_parent.json")) as f:
        want = json.load(f)
    assert want["columns"] == gen.COLUMNS
    rows = []
    for m, row in gen.scan(lib):
        rows.append(row)
        f = row.split()
        n, ntf, ntb, gw = int(f[5]), int(f[7]), int(f[8]), int(f[-2])
        fwd, bwd = kernel_name(lib, m, n, 0), kernel_name(lib, m, n, 1)
        assert fwd in listed_kernels and bwd in listed_kernels, (row, fwd, bwd)
        assert fwd.startswith("tg_forward_kernel<%d," % ntf), (row, fwd)
        assert bwd.startswith("tg_backward_kernel<%d," % ntb), (row, bwd)
        assert fwd.endswith(",true>" if gw else ",false>"), (row, fwd)
    shapes = {tuple(r.split()[:3]) for r in rows}
    assert len(shapes) >= 300  # the scan saw shapes
    assert len(shapes) == want["shapes"] and len(rows) == want["n_rows"]
    kept = [r for r in rows if int(r.split()[0]) in gen.ROWS_KEPT]
    assert len(kept) == len(want["rows"])
    for got, exp in zip(kept, want["rows"]):
        assert got == exp, gen.COLUMNS
    assert gen.digest(rows) == want["sha256"]


def F(args):
    return "tg_forward_kernel<%s>" % args


def B(args):
    return "tg_backward_kernel<%s>" % args


GW = (F("256,0,0,0,false,true"), B("256,0,0,0,false,true"))
# (K, M, B) -> per (forced widths, n_chains): forward, backward
NAMES = {
    (6, 50, 25): {  # C3
        ((0, 0), 1): (F("512,6,50,25,false,false"), B("768,6,50,25,false,false")),
        ((0, 0), 100000): (F("256,6,50,25,false,false"), B("256,6,50,25,false,false")),
        ((512, 768), 1): (F("512,6,50,25,false,false"), B("768,6,50,25,false,false")),
        ((512, 768), 100000): (F("512,6,50,25,false,false"), B("768,6,50,25,false,false")),
    },
    (12, 50, 25): {  # C5
        ((0, 0), 1): (F("512,12,50,25,false,false"), B("768,12,50,25,false,false")),
        ((0, 0), 100000): (F("512,12,50,25,false,false"), B("256,12,50,25,false,true")),
        ((512, 768), 1): (F("512,12,50,25,false,false"), B("768,12,50,25,false,false")),
        ((512, 768), 100000): (F("512,12,50,25,false,false"), B("768,12,50,25,false,false")),
    },
    (6, 50, 64): {  # the C3 sizes, another B: the generic builds
        ((0, 0), 1): (F("512,0,0,0,false,false"), B("768,0,0,0,false,false")),
        ((0, 0), 100000): (F("256,0,0,0,false,false"), B("256,0,0,0,false,false")),
        ((512, 768), 1): (F("512,0,0,0,false,false"), B("768,0,0,0,false,false")),
        ((512, 768), 100000): (F("512,0,0,0,false,false"), B("768,0,0,0,false,false")),
    },
    # particle arrays past LDS: the one width 256, forced or not
    (13, 50, 25): {(f, n): GW for f in ((0, 0), (512, 768)) for n in (1, 100000)},
    (6, 200, 25): {(f, n): GW for f in ((0, 0), (512, 768)) for n in (1, 100000)},
    (16, 256, 25): {(f, n): GW for f in ((0, 0), (512, 768)) for n in (1, 100000)},
    (12, 65, 25): {(f, n): GW for f in ((0, 0), (512, 768)) for n in (1, 100000)},  # M > 64
    # fits at 256 threads only (forward); the backward's layout fits at any width
    (12, 54, 25): {(f, n): (F("256,0,0,0,false,false"), B("768,0,0,0,false,false"))
                   for f in ((0, 0), (512, 768)) for n in (1, 100000)},
}


@pytest.mark.parametrize("shape", sorted(NAMES))
def test_kernel_names_equal_parent(lib, shape):
    m = gen.small_model(*shape)
    try:
        for (force, n), want in sorted(NAMES[shape].items()):
            assert lib.hyg_tg_force_threads(*force) == 0
            assert (kernel_name(lib, m, n, 0), kernel_name(lib, m, n, 1)) == want, (shape, force, n)
    finally:
        lib.hyg_tg_force_threads(0, 0)
        m.close()


def test_kernel_name_buffer_convention(lib):
    m = gen.small_model(6, 50, 25)
    try:
        full = kernel_name(lib, m, 100000, 1)
        assert re.fullmatch(r"tg_backward_kernel<\d+,\d+,\d+,\d+,(true|false),(true|false)>", full)
        buf = C.create_string_buffer(b"x" * 16, 16)
        assert lib.hyg_tg_kernel_name(m.handle, 100000, 1, buf, 8) == len(full) + 1  # truncated, NUL included
        assert buf.raw[:8] == full[:7].encode() + b"\0" and buf.raw[8:] == b"x" * 8
        assert lib.hyg_tg_kernel_name(None, 1, 0, None, 0) == _lib.HYG_EINVAL
        assert lib.hyg_tg_kernel_name(m.handle, 1, 0, None, -1) == _lib.HYG_EINVAL
    finally:
        m.close()


def test_more_than_256_ancestors_has_no_plan(lib):
    """M = 257: the model is built, and no width runs it (one resampled
    ancestor per thread of at most 256 threads where the shape is past LDS)."""
    m = gen.small_model(6, 257, 25)
    try:
        for backward in (0, 1):
            assert lib.hyg_tg_kernel_name(m.handle, 1, backward, None, 0) == _lib.HYG_EUNSUPPORTED
            assert lib.hyg_last_error().decode() == ("num_resampled_particles M = 257 exceeds 256 (one resampled "
                                                     "ancestor per thread of a 256-thread workgroup)")
    finally:
        m.close()
