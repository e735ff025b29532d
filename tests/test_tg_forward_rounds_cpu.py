"""The schedule of a forward cut into two rounds (hyg_tg_forward_schedule,
hyg_tg_set_forward_rounds), as data; no device needed.

A launch of n chains on C CUs leaves the first n % C CUs one chain more than
the others for its whole length. Round 1 runs every chain to a cut of its own,
round 2 resumes every chain from its last record in another block order, in
which the chains of round 1's heavier CUs sit on lighter ones. The tests pin
that on the flagship job's 582 chains and on small faked devices, and that
every launch the schedule has no business with is left as one launch.
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from hygeia_amd import _lib, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("make_tg_plan", os.path.join(ROOT, "tests", "golden", "make_tg_plan.py"))
gen = importlib.util.module_from_spec(spec)
spec.loader.exec_module(gen)

CUS = [256]  # the CU count the schedule is asked for (the settings fixture)
RESIDENT = 3  # forward workgroups a CU holds at 256 threads (<= 168 VGPRs)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def c3(lib):
    m = gen.small_model(6, 50, 25)
    yield m
    m.close()


@pytest.fixture
def settings(lib):
    """Sets the CU count the schedule is asked for, the rounds mode and the
    forced forward width for one test; restores the defaults afterwards. The
    kernel is planned for the current device (256 CUs on a host without one,
    which hyg_tg_set_device_cus does not change there), so the small pretended
    devices force the width a launch of more chains than CUs has, 256."""
    def apply(cus, mode, width=None):
        CUS[0] = cus
        assert lib.hyg_tg_set_device_cus(0, 256) == 0
        assert lib.hyg_tg_set_forward_rounds(mode) == 0
        assert lib.hyg_tg_force_threads((256 if cus < 256 else 0) if width is None else width, 0) == 0

    yield apply
    lib.hyg_tg_set_device_cus(0, 0)
    lib.hyg_tg_set_forward_rounds(1)
    lib.hyg_tg_force_threads(0, 0)


def schedule(lib, model, lengths, forward_only=0, resident=RESIDENT, multi=0):
    n = len(lengths)
    T = np.ascontiguousarray(lengths, dtype=np.int32)
    blocks = np.zeros(2, np.int32)
    order, begin, end = (np.zeros((2, n), np.int32) for _ in range(3))
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rounds = lib.hyg_tg_forward_schedule(model.handle, p(T), n, multi, forward_only, CUS[0], resident, 2, p(blocks),
                                         p(order), p(begin), p(end))
    assert rounds in (1, 2), lib.hyg_last_error()
    return rounds, blocks, order, begin, end


def c3_lengths():
    """The flagship job's chains in launch order: every segment under two seeds, longest first."""
    segs = synthetic.segment_chains(synthetic.chromosome_sizes(28_000_000))
    return sorted([s[3] for s in segs] * 2, reverse=True)


def check_split(lengths, cus, sched, all_heavy_move=True):
    rounds, blocks, order, begin, end = sched
    n = len(lengths)
    T = np.asarray(lengths)
    assert rounds == 2 and blocks[0] == n
    # round 1: every chain in launch order, from step 1
    assert (order[0] == np.arange(n)).all() and (begin[0] == 1).all()
    cut = end[0]
    live = np.flatnonzero(cut < T)
    # the ranges tile [1, T) in order; a cut is 64 q + 1 with a step left behind it
    assert ((cut == T) | ((cut % 64 == 1) & (cut >= 65) & (cut < T))).all()
    assert (begin[1][live] == cut[live]).all() and (end[1][live] == T[live]).all()
    done = np.setdiff1d(np.arange(n), live)
    assert (begin[1][done] == end[1][done]).all()  # a finished chain runs nothing more
    # no chain that could be cut is left whole
    assert (cut[T >= 66] < T[T >= 66]).all() and (cut[T < 66] == T[T < 66]).all()
    # round 2's order: a permutation of the chains still running; finished ones are absent
    n2 = int(blocks[1])
    assert n2 == len(live) and sorted(order[1][:n2]) == list(live) and (order[1][n2:] == -1).all()
    # the chains of round 1's heavier CUs sit on lighter ones
    k, e = n // cus, n % cus
    k2, e2 = n2 // cus, n2 % cus
    heavy1 = [i for i in live if k >= 1 and i % cus < e]
    pos = {int(c): p for p, c in enumerate(order[1][:n2])}
    heavy2 = lambda p: k2 >= 1 and p % cus < e2  # noqa: E731
    light_blocks = sum(1 for p in range(n2) if not heavy2(p))
    moved = sum(1 for i in heavy1 if not heavy2(pos[int(i)]))
    if all_heavy_move:
        assert moved == len(heavy1)
    else:  # more heavy chains than light blocks: every light block holds one
        assert len(heavy1) > light_blocks and moved == light_blocks
    # the heavy blocks hold the light chains with the least left to do
    light1 = [i for i in live if i not in set(heavy1)]
    in_heavy = [int(c) for p, c in enumerate(order[1][:n2]) if heavy2(p) and c in set(light1)]
    stay = [i for i in light1 if i not in set(in_heavy)]
    if in_heavy and stay:
        assert max(T[i] - cut[i] for i in in_heavy) <= min(T[i] - cut[i] for i in stay)
    return cut


def test_c3_job_is_cut_in_two(lib, c3, settings):
    """582 chains on 256 CUs: 70 CUs hold three chains, 186 two. The 210 chains
    of the three-chain CUs all sit on two-chain CUs in round 2, and the rounds
    are balanced: a heavy chain does 60 % of its steps in round 1, a
    light one a little more, by the step rates of the two loads in each round."""
    settings(256, 1)
    T = c3_lengths()
    assert len(T) == 582 and T[0] == 110000
    cut = check_split(T, 256, schedule(lib, c3, T))
    T = np.asarray(T)
    heavy = np.arange(582) % 256 < 70
    assert heavy.sum() == 210
    # measured us per step of the slowest chain (profiles/r09_census_rounds.txt): a three- and a two-chain CU in
    # round 1 (a, b), a two- and a three-chain CU in round 2 (c, d); both rounds end together at
    # a fh = b fl and c (1 - fh) = d (1 - fl)
    a, b, c, d = 15.60, 14.44, 14.03, 15.98
    fh = (d - c) * b / (a * d - b * c)
    fl = fh * a / b
    assert abs(fh - 0.603) < 0.001 and abs(fl - 0.6515) < 0.001
    assert (np.abs(cut[heavy] - fh * T[heavy]) <= 33).all() and (np.abs(cut[~heavy] - fl * T[~heavy]) <= 33).all()
    # under those rates each round's two kinds of CU end within a block of steps of each other
    assert abs((cut[heavy] * a).max() - (cut[~heavy] * b).max()) <= 64 * a
    assert abs(((T - cut)[heavy] * c).max() - ((T - cut)[~heavy] * d).max()) <= 64 * d
    # the multi-model launch of the same chains is cut alike
    assert schedule(lib, c3, list(T), multi=1)[0] == 2


@pytest.mark.parametrize("n,cus,lengths", [
    (5, 4, [700, 650, 300, 66, 200]),
    (10, 4, [700, 640, 600, 510, 450, 400, 64, 300, 250, 200]),  # one chain below the earliest cut
    (10, 4, [700, 640, 600, 510, 450, 400, 65, 300, 130, 190]),
])
def test_forced_rounds_on_small_devices(lib, c3, settings, n, cus, lengths):
    settings(cus, 2)
    assert len(lengths) == n
    check_split(lengths, cus, schedule(lib, c3, lengths))
    settings(cus, 1)  # automatic: too short for a relaunch to pay
    assert schedule(lib, c3, lengths)[0] == 1


def test_forced_rounds_with_more_heavy_chains_than_light_blocks(lib, c3, settings):
    """10 chains on 4 CUs, all cut: six sit on the three-chain CUs and round 2
    has four blocks on two-chain CUs, so four move and two cannot (the automatic
    mode does not cut such a launch: the heavy set must fit the light blocks)."""
    settings(4, 2)
    lengths = [700, 640, 600, 510, 450, 400, 350, 300, 250, 200]
    check_split(lengths, 4, schedule(lib, c3, lengths), all_heavy_move=False)
    settings(4, 1)
    assert schedule(lib, c3, [100000 + x for x in lengths])[0] == 1


def test_smallest_and_last_legal_cuts(lib, c3, settings):
    settings(4, 2)
    lengths = [700, 640, 190, 510, 450, 400, 64, 300, 100, 600]
    _, _, _, _, end = schedule(lib, c3, lengths)
    cut = dict(zip(lengths, end[0]))
    assert cut[64] == 64  # finishes in round 1
    assert cut[100] == 65  # the smallest legal cut
    assert cut[190] == 129 == (190 - 2) // 64 * 64 + 1  # the last legal one below T


def one_launch(sched, n):
    rounds, blocks, order, begin, end = sched
    return (rounds == 1 and blocks[0] == n and blocks[1] == 0 and (order[0] == np.arange(n)).all()
            and (order[1] == -1).all() and (begin[0] == 1).all() and (begin[1] == end[1]).all())


def test_launches_that_are_not_cut(lib, c3, settings):
    long = 110000
    settings(256, 1)
    assert schedule(lib, c3, [long] * 582)[0] == 2  # (the control: this one is)
    for n in (768, 512, 73, 256):  # full CUs, one chain per CU or fewer
        T = [long] * n
        assert one_launch(schedule(lib, c3, T), n), n
        s = schedule(lib, c3, T)
        assert (s[4][0] == long).all()
    assert one_launch(schedule(lib, c3, [long] * 291), 291)  # one or two per CU: the rate at one was never measured
    assert one_launch(schedule(lib, c3, [long] * 700), 700)  # 188 CUs of three: 564 chains for 136 blocks
    assert one_launch(schedule(lib, c3, [4000] * 582), 582)  # below the length threshold
    assert one_launch(schedule(lib, c3, [long] * 582, forward_only=1), 582)  # a forward-only launch
    assert one_launch(schedule(lib, c3, [long] * 582, resident=2), 582)  # no CU holds three
    for width in (512, 768):  # a forced width other than 256
        settings(256, 1, width)
        assert one_launch(schedule(lib, c3, [long] * 582), 582)
        settings(256, 2, width)
        assert one_launch(schedule(lib, c3, [long] * 582), 582)
    settings(256, 1)
    gw = gen.small_model(6, 200, 25)  # particle arrays in global memory
    try:
        assert lib.hyg_tg_global_weights(gw.handle) == 1
        assert one_launch(schedule(lib, gw, [long] * 582), 582)
        settings(256, 2)
        assert one_launch(schedule(lib, gw, [long] * 582), 582)
    finally:
        gw.close()


def test_600_chains_fit_and_are_cut(lib, c3, settings):
    settings(256, 1)
    T = [110000] * 600
    check_split(T, 256, schedule(lib, c3, T))


def test_mode_zero_is_one_launch(lib, c3, settings):
    for cus, lengths in ((256, c3_lengths()), (4, [700, 650, 300, 66, 200]), (4, [300] * 10)):
        settings(cus, 0)
        assert one_launch(schedule(lib, c3, lengths), len(lengths))


def test_mode_range_and_arguments(lib, c3):
    try:
        assert [lib.hyg_tg_set_forward_rounds(m) for m in (0, 1, 2)] == [0, 0, 0]
        assert lib.hyg_tg_set_forward_rounds(3) == _lib.HYG_EINVAL and lib.hyg_tg_set_forward_rounds(-1) == _lib.HYG_EINVAL
    finally:
        lib.hyg_tg_set_forward_rounds(1)
    T = np.array([100, 0], np.int32)
    a = np.zeros(4, np.int32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.hyg_tg_forward_schedule(c3.handle, p(T), 2, 0, 0, 256, 3, 2, p(a), p(a), p(a), p(a)) == _lib.HYG_EINVAL
    assert lib.hyg_tg_forward_schedule(c3.handle, p(T), 1, 0, 0, 256, 3, 1, p(a), p(a), p(a), p(a)) == _lib.HYG_EINVAL
    assert lib.hyg_tg_forward_schedule(None, p(T), 1, 0, 0, 256, 3, 2, p(a), p(a), p(a), p(a)) == _lib.HYG_EINVAL


def kernel_name(lib, model, n, backward):
    buf = C.create_string_buffer(96)
    assert lib.hyg_tg_kernel_name(model.handle, n, backward, buf, 96) > 1
    return buf.value.decode()


def test_plan_rows_are_unchanged(lib, c3, settings):
    """The launch's own kernels are what they were, whatever the rounds mode."""
    for mode in (0, 1, 2):
        settings(256, mode)
        assert kernel_name(lib, c3, 582, 0) == "tg_forward_kernel<256,6,50,25,false,false>"
        assert kernel_name(lib, c3, 582, 1) == "tg_backward_kernel<256,6,50,25,false,false>"
        assert kernel_name(lib, c3, 73, 0) == "tg_forward_kernel<512,6,50,25,false,false>"
        assert kernel_name(lib, c3, 73, 1) == "tg_backward_kernel<768,6,50,25,false,false>"
