"""The stream plan of a device (ocrs_amd/csrc/stream_plan.hpp, option "stream_budget") through its host-only hook
ocrs_stream_plan_selftest: which light lane a call is dealt, and the accounting behind it.  No GPU."""
import ctypes as C

import pytest

from ocrs_amd import _lib

ACQUIRE, RELEASE, SET_BUDGET, LOAD, BUDGET, LIGHT = range(6)


@pytest.fixture(scope="module")
def lib():
    from ocrs_amd import build
    build.build()
    return _lib.lib()


def drive(lib, budget, ops):
    flat = (C.c_int32 * (2 * len(ops)))(*[v for op in ops for v in op])
    out = (C.c_int32 * max(1, len(ops)))()
    _lib.check(lib.ocrs_stream_plan_selftest(C.c_int(budget), flat, C.c_size_t(len(ops)), out))
    return list(out[:len(ops)])


def test_a_call_gets_the_least_loaded_light_lane_and_ties_go_round_robin(lib):
    # budget 5: lanes 0, 1, 2.  Empty plan: every lane ties, dealt in turn; then the next round the same way
    assert drive(lib, 5, [(LIGHT, 0)] + [(ACQUIRE, -1)] * 7) == [3, 0, 1, 2, 0, 1, 2, 0]
    # least loaded wins over the turn: lane 1 ends a call, the next call goes there although the turn is lane 0's
    got = drive(lib, 5, [(ACQUIRE, -1)] * 3 + [(RELEASE, 1), (ACQUIRE, -1), (LOAD, 0), (LOAD, 1), (LOAD, 2)])
    assert got == [0, 1, 2, 2, 1, 1, 1, 1]
    # ... and a tie after that starts behind the lane dealt last (lane 1): lane 2, then 0
    got = drive(lib, 5, [(ACQUIRE, -1)] * 3 + [(RELEASE, 1), (ACQUIRE, -1), (ACQUIRE, -1), (ACQUIRE, -1)])
    assert got[-2:] == [2, 0]
    # two lanes ending calls: the emptier one first, whichever the turn
    got = drive(lib, 5, [(ACQUIRE, -1)] * 6 + [(RELEASE, 2), (RELEASE, 2), (RELEASE, 0), (ACQUIRE, -1), (ACQUIRE, -1), (ACQUIRE, -1)])
    assert got[-3:] == [2, 0, 2]


def test_a_second_lease_of_one_call_avoids_the_lane_the_call_is_on(lib):
    # (the long/short split of a recognition request: the long lines go to another lane than the call's own)
    assert drive(lib, 4, [(ACQUIRE, -1), (ACQUIRE, 0), (ACQUIRE, -1), (ACQUIRE, 1)]) == [0, 1, 0, 0]
    # the other lane is taken even when it is the fuller one
    assert drive(lib, 4, [(ACQUIRE, -1), (ACQUIRE, -1), (ACQUIRE, -1), (RELEASE, 0), (RELEASE, 0), (ACQUIRE, 0), (LOAD, 1)])[-2:] == [1, 2]
    # one light lane: nothing to avoid it with
    assert drive(lib, 3, [(ACQUIRE, -1), (ACQUIRE, 0)]) == [0, 0]


@pytest.mark.parametrize("order", [(0, 1, 2, 0, 1), (1, 0, 1, 2, 0), (2, 1, 0, 1, 0), (0, 0, 1, 1, 2)])
def test_release_order_does_not_matter(lib, order):
    ops = [(ACQUIRE, -1)] * 5 + [(RELEASE, lane) for lane in order] + [(LOAD, 0), (LOAD, 1), (LOAD, 2)] + [(ACQUIRE, -1)] * 3
    got = drive(lib, 5, ops)
    assert got[:5] == [0, 1, 2, 0, 1]
    assert got[5:10] == [4, 3, 2, 1, 0]          # calls still in flight after each end
    assert got[10:13] == [0, 0, 0]               # every lane back to empty
    assert sorted(got[13:]) == [0, 1, 2]         # and the empty plan deals every lane once again


def test_budget_three_has_one_light_lane_and_budget_zero_is_private(lib):
    assert drive(lib, 3, [(LIGHT, 0), (ACQUIRE, -1), (ACQUIRE, -1), (ACQUIRE, -1), (LOAD, 0)]) == [1, 0, 0, 0, 3]
    assert drive(lib, 0, [(BUDGET, 0), (LIGHT, 0), (ACQUIRE, -1), (ACQUIRE, -1), (RELEASE, -1), (RELEASE, -1)]) == [0, 0, -1, -1, 1, 0]
    assert drive(lib, 16, [(LIGHT, 0)]) == [14]
    for bad in (1, 2, 17, -1):
        flat, out = (C.c_int32 * 2)(), (C.c_int32 * 1)()
        assert lib.ocrs_stream_plan_selftest(C.c_int(bad), flat, C.c_size_t(0), out) != 0


def test_a_budget_change_with_a_lease_outstanding_is_refused(lib):
    got = drive(lib, 4, [(ACQUIRE, -1), (SET_BUDGET, 8), (BUDGET, 0), (SET_BUDGET, 4), (RELEASE, 0), (SET_BUDGET, 8), (BUDGET, 0), (LIGHT, 0),
                         (SET_BUDGET, 2), (SET_BUDGET, 17), (SET_BUDGET, 0), (ACQUIRE, -1), (SET_BUDGET, 4), (RELEASE, -1), (SET_BUDGET, 4), (BUDGET, 0)])
    #            refused  still 4  no change: fine  idle: taken up           never valid   private   a private call counts too
    assert got == [0, 0, 4, 1, 0, 1, 8, 6, 0, 0, 1, -1, 0, 0, 1, 4]


def test_the_option_takes_zero_and_three_to_sixteen_for_the_process_only(lib):
    assert "stream_budget" in _lib.option_names()
    try:
        for ok in (0, 3, 4, 8, 16):
            assert lib.ocrs_set_option(b"stream_budget", C.c_long(ok)) == 0
        for bad in (1, 2, 17, -4):
            assert lib.ocrs_set_option(b"stream_budget", C.c_long(bad)) == 1
            assert b"out of range" in lib.ocrs_last_error()
    finally:
        assert lib.ocrs_set_option(b"stream_budget", C.c_long(4)) == 0
