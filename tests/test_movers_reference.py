"""The path arithmetic of the movers on the CPU: sgp_path_prepare against the float64 restatement (tests/mover_reference.py), sgp_path_advance bit for bit
against the float32 restatement, and properties of the restatement itself.  No device."""
import ctypes as C

import numpy as np
import pytest

import mover_reference as mr
import mover_scenes as ms
from substrata_amd import abi, build

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(build.build())
    abi.bind(lib, "sgp_")
    return lib


def waypoint_array(waypoints):
    a = np.zeros(len(waypoints), dtype=abi.path_waypoint_dtype)
    for k, (pos, typ, pause, speed) in enumerate(waypoints):
        a[k]["pos"] = pos; a[k]["type"] = typ; a[k]["pause_time"] = pause; a[k]["speed"] = speed
    return a


def lib_prepare(lib, waypoints):
    a = waypoint_array(waypoints)
    out = np.zeros(max(len(a), 1), dtype=abi.path_segment_dtype)
    total = C.c_double(-1.0)
    r = lib.sgp_path_prepare(a.ctypes.data if len(a) else out.ctypes.data, len(a), out.ctypes.data, C.byref(total))
    return (out[:len(a)], total.value) if r == abi.OK else None


@pytest.fixture(scope="module")
def prepared(lib):
    return {name: lib_prepare(lib, wps) for name, wps in ms.PATHS.items()}


def ulp32(x):
    return float(np.spacing(F32(abs(x))))


@pytest.mark.parametrize("name", sorted(ms.PATHS))
def test_prepare_against_float64(prepared, name):
    got = prepared[name]
    r32, r64 = mr.prepare(ms.PATHS[name], F32), mr.prepare(ms.PATHS[name], F64)
    assert got is not None and r32 is not None and r64 is not None
    segs, total = got
    worst = 0.0
    for k, (s32, s64) in enumerate(zip(r32[0], r64[0])):
        assert int(segs[k]["type"]) == s64.type and tuple(segs[k]["pos"]) == tuple(F32(x) for x in s64.pos)
        assert segs[k]["pause_time"] == F32(s64.pause_time) and segs[k]["speed"] == F32(s64.speed)
        for f in mr.DERIVED:
            ref = float(getattr(s64, f))
            err, own = abs(float(segs[k][f]) - ref), abs(float(getattr(s32, f)) - ref)
            assert err <= 4.0 * own + ulp32(ref), (name, k, f, err, own)
            worst = max(worst, err / max(abs(ref), 1.0e-30))
        for c in range(3):      # a unit vector (or zero): an ulp of its length
            ref = float(s64.exit_dir[c])
            err, own = abs(float(segs[k]["exit_segment_unit_dir"][c]) - ref), abs(float(s32.exit_dir[c]) - ref)
            assert err <= 4.0 * own + ulp32(1.0), (name, k, c, err, own)
    # the traversal time: double sums of fp32 quotients
    assert abs(total - r64[1]) <= 4.0 * abs(r32[1] - r64[1]) + ulp32(r64[1]), (name, total, r32[1], r64[1])
    print("%s: worst relative error of a derived value %.3e, total time %.9f (float64 %.9f)" % (name, worst, total, r64[1]))


@pytest.mark.parametrize("name", sorted(ms.REFUSED))
def test_refusals_are_equal(lib, name):
    assert lib_prepare(lib, ms.REFUSED[name]) is None, name
    assert b"sgp_path_prepare" in lib.sgp_last_error()
    assert mr.prepare(ms.REFUSED[name], F64) is None and mr.prepare(ms.REFUSED[name], F32) is None


def test_the_loop_has_every_kind_of_curve(prepared):
    """What the table promises: arcs with zero and non-zero entry and exit straights, and the angle < 1e-6 branch."""
    segs = prepared["loop"][0]
    curves = [s for s in segs if s["type"] == mr.CURVE_IN]
    exit_len = [float(s["segment_len"]) - float(s["just_curve_len"]) - float(s["entry_segment_len"]) for s in curves]
    assert any(s["entry_segment_len"] == 0 for s in curves) and any(abs(s["entry_segment_len"] - 2.0) < 1e-4 for s in curves)
    assert any(abs(e) < 1e-5 for e in exit_len) and any(abs(e - 2.0) < 1e-4 for e in exit_len)
    assert all(abs(s["curve_angle"] - np.pi / 2) < 1e-5 and abs(s["curve_r"] - 4.0) < 1e-4 for s in curves)
    eq = prepared["straight_curve"][0][1]
    assert eq["curve_angle"] == 0 and eq["curve_r"] == 1000.0 and eq["just_curve_len"] == 0 and eq["entry_segment_len"] == eq["segment_len"] == 5.0


@pytest.mark.parametrize("name", sorted(ms.PATHS))
def test_advance_is_bit_equal(lib, prepared, name):
    """After every one of 200 updates at three values of dt: index, dist, time and status equal to the float32 restatement fed the library's segments."""
    arr = np.ascontiguousarray(prepared[name][0])
    segs = mr.segs_from_array(arr, F32)
    seen = set()
    for dt in ms.DTS:
        p = abi.PathProgress(0, 0.0, 0.0)
        state = (0, F32(0), F32(0))
        for u in range(200):
            st = C.c_uint32(0)
            assert lib.sgp_path_advance(arr.ctypes.data, len(arr), C.byref(p), C.c_float(dt), C.byref(st)) == abi.OK
            before = state
            idx, dist, time, status = mr.advance(segs, state, F32(dt))
            state = (idx, dist, time)
            assert p.waypoint_index == idx and st.value == status, (name, dt, u)
            assert F32(p.dist_along_segment).tobytes() == dist.tobytes() and F32(p.time_along_segment).tobytes() == time.tobytes(), (name, dt, u, p.dist_along_segment, dist)
            ends = (idx - before[0]) % len(segs)
            if status & mr.ST_OVERRUN:
                seen.add("overrun")
                assert dist == 0 and time == 0
            elif ends > 1:
                seen.add("several_ends")
            if segs[idx].type == mr.STATION and time < segs[idx].pause_time and idx == before[0] and before[2] > 0:
                seen.add("paused")
    if name == "ring":
        assert {"overrun", "several_ends"} <= seen
    if name == "loop":
        assert "paused" in seen      # the pause of 0.5 s is longer than several frames
    # dt == 0 and a negative dt change nothing
    p = abi.PathProgress(1, 0.25, 0.125)
    st = C.c_uint32(0)
    for dt in (0.0, -1.0):
        assert lib.sgp_path_advance(arr.ctypes.data, len(arr), C.byref(p), C.c_float(dt), C.byref(st)) == abi.OK
        assert (p.waypoint_index, p.dist_along_segment, p.time_along_segment, st.value) == (1, 0.25, 0.125, 0)
    assert lib.sgp_path_advance(arr.ctypes.data, len(arr), C.byref(p), C.c_float(float("nan")), C.byref(st)) == abi.ERR_INVALID
    p.waypoint_index = len(arr)
    assert lib.sgp_path_advance(arr.ctypes.data, len(arr), C.byref(p), C.c_float(0.1), C.byref(st)) == abi.ERR_INVALID


@pytest.mark.parametrize("name", sorted(ms.PATHS))
def test_a_loop_walked_for_its_total_time_returns_to_its_start(name):
    segs, total = mr.prepare(ms.PATHS[name], F64)
    total = sum(float(s.segment_len / s.speed) + (float(s.pause_time) if s.type == mr.STATION else 0.0) for s in segs)
    start = mr.eval_state(segs, 0, F64(0))[0]
    idx, dist, time, status = mr.advance(segs, (0, F64(0), F64(0)), F64(total), max_ends=10 ** 6)
    pos = mr.eval_state(segs, idx, dist)[0]
    extent = max(float(mr.v_dist(s.pos, segs[0].pos)) for s in segs)
    assert status == 0 and float(mr.v_dist(pos, start)) <= 64 * len(segs) * np.finfo(F64).eps * max(extent, 1.0), (idx, dist)


def test_a_follower_sits_follow_dist_behind_on_a_straight():
    segs, _ = mr.prepare(ms.PATHS["loop"], F32)
    # the leader 6 m along the straight from (14, 4) to (14, 12); then 1 m past (8, 16), the follower back on the exit straight of the curve before it
    for idx, dist, follow in ((2, F32(6.0), 2.5), (4, F32(1.0), 1.5)):
        lead = mr.eval_state(segs, idx, dist)[0]
        pos, d, fi, fd, status = mr.eval_backwards(segs, idx, dist, F32(follow))
        assert status == 0 and abs(float(mr.v_dist(lead, pos)) - follow) < 1e-5
        assert abs(float(mr.v_len(d)) - 1.0) < 1e-6
    # more segment starts than the cap: the entry of the segment reached, flagged
    ring, _ = mr.prepare(ms.PATHS["ring"], F32)
    pos, d, fi, fd, status = mr.eval_backwards(ring, 10, F32(0.01), F32(5.0))
    assert status == mr.ST_OVERRUN and fi == (10 - 64) % 100 and fd == 0 and pos == ring[fi].pos
