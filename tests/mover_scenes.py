"""The seeded table of paths, tracks and mover mixes the mover tests share -- a helper, not a test.

Waypoints are (pos, type, pause_time, speed) with fp32-representable values where it matters (the restatement rounds them to fp32 first, as the ABI does)."""
import math

import numpy as np

from mover_reference import CURVE_IN, CURVE_OUT, STATION, EASE_LINEAR, EASE_SMOOTHSTEP, ORIENT_ALONG_PATH

DTS = (1.0 / 60.0, 0.1, 0.37)      # a frame; several ends of the short segments; past the cap on "ring"


def _loop():
    """A rounded rectangle: a station with a pause of 0.5 s (30 frames), four arcs -- entry and exit straights of zero length, an exit straight of 2, an
    entry straight of 2 --, curve-outs between them."""
    return [((0, 0, 0), STATION, 0.5, 4.0), ((10, 0, 0), CURVE_IN, 0.0, 3.0), ((14, 4, 0), CURVE_OUT, 0.0, 5.0), ((14, 12, 0), CURVE_IN, 0.0, 3.0),
            ((8, 16, 0), CURVE_OUT, 0.0, 6.0), ((2, 16, 0), CURVE_IN, 0.0, 2.5), ((-4, 12, 0), CURVE_OUT, 0.0, 5.0), ((-4, 4, 0), CURVE_IN, 0.0, 3.5)]


def _straight_curve():
    """A CurveIn whose entry and exit directions are equal (the angle < 1e-6 branch), a station off the plane, a sloped return."""
    return [((0, 0, 1), CURVE_OUT, 0.0, 2.0), ((5, 0, 1), CURVE_IN, 0.0, 2.0), ((10, 0, 1), CURVE_OUT, 0.0, 3.0), ((15, 0, 1), STATION, 0.25, 4.0),
            ((15, 6, 3), CURVE_OUT, 0.0, 7.0), ((0, 6, 1), STATION, 0.0, 5.0)]


def _ring(n=100, r=1.0, speed=50.0):
    """Short segments: a frame passes 13 ends, 0.1 s passes the cap of 64."""
    return [((r * math.cos(2 * math.pi * k / n), r * math.sin(2 * math.pi * k / n), 2.0), CURVE_OUT if k % 3 else STATION, 0.0, speed) for k in range(n)]


def _random(seed, n):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-20.0, 20.0, size=(n, 3)).astype(np.float32)
    return [(tuple(float(x) for x in pts[k]), STATION if rng.integers(3) == 0 else CURVE_OUT, float(np.float32(rng.uniform(0.0, 0.2))), float(np.float32(rng.uniform(1.0, 30.0))))
            for k in range(n)]


PATHS = {"loop": _loop(), "straight_curve": _straight_curve(), "ring": _ring(), "ring_fast": _ring(speed=400.0), "two": [((0, 0, 0), STATION, 0.1, 1.0), ((0, 0, 3), STATION, 0.3, 2.0)],
         "random7": _random(7, 7), "random128": _random(128, 128)}

REFUSED = {"one": _loop()[:1], "empty": [], "too_many": _random(129, 129),
           "zero_segment": [((0, 0, 0), CURVE_OUT, 0.0, 1.0), ((0, 0, 0), CURVE_OUT, 0.0, 1.0), ((1, 0, 0), CURVE_OUT, 0.0, 1.0)],
           "nan_pos": [((0, float("nan"), 0), CURVE_OUT, 0.0, 1.0), ((1, 0, 0), CURVE_OUT, 0.0, 1.0)],
           "inf_pos": [((0, float("inf"), 0), CURVE_OUT, 0.0, 1.0), ((1, 0, 0), CURVE_OUT, 0.0, 1.0)],
           "zero_speed": [((0, 0, 0), CURVE_OUT, 0.0, 0.0), ((1, 0, 0), CURVE_OUT, 0.0, 1.0)],
           "negative_speed": [((0, 0, 0), CURVE_OUT, 0.0, -1.0), ((1, 0, 0), CURVE_OUT, 0.0, 1.0)],
           "inf_speed": [((0, 0, 0), CURVE_OUT, 0.0, float("inf")), ((1, 0, 0), CURVE_OUT, 0.0, 1.0)],
           "negative_pause": [((0, 0, 0), STATION, -0.5, 1.0), ((1, 0, 0), CURVE_OUT, 0.0, 1.0)],
           "nan_pause": [((0, 0, 0), STATION, float("nan"), 1.0), ((1, 0, 0), CURVE_OUT, 0.0, 1.0)],
           "unknown_type": [((0, 0, 0), 3, 0.0, 1.0), ((1, 0, 0), CURVE_OUT, 0.0, 1.0)],
           # a curve whose entry line and exit ray are antiparallel: 1 - dot^2 = 0, the intersection is not finite
           "antiparallel_curve": [((0, 0, 0), CURVE_IN, 0.0, 1.0), ((4, 0, 0), CURVE_OUT, 0.0, 1.0), ((1, 0, 0), CURVE_OUT, 0.0, 1.0), ((-4, 0, 0), CURVE_OUT, 0.0, 1.0)]}


def _rz(deg, sign=1.0):
    a = math.radians(deg)
    return (0.0, 0.0, sign * math.sin(0.5 * a), sign * math.cos(0.5 * a))


# (start, target, duration, easing, cur_elapsed)
POS_TRACKS = [((0, 0, 1), (0, 0, 4), 0.5, EASE_LINEAR, 0.0), ((1, 2, 3), (-2, 5, 3.5), 0.4, EASE_SMOOTHSTEP, 0.05),
              ((0, 0, 0), (1, 1, 1), 0.3, EASE_LINEAR, 0.9),      # cur_elapsed > duration: the target at once, then inactive
              ((3, 0, 0), (3, 0, 2), 0.0, EASE_SMOOTHSTEP, 0.0)]  # duration clamped to 1e-4
ROT_TRACKS = [(_rz(0), _rz(120, -1.0), 0.5, EASE_LINEAR, 0.0),     # dot < 0: the target is negated first
              (_rz(10), _rz(10.5), 0.3, EASE_SMOOTHSTEP, 0.0),     # nearly parallel: the normalised lerp
              ((0.0, 0.0, 0.0, 1.0), (math.sin(0.7), 0.0, 0.0, math.cos(0.7)), 0.45, EASE_SMOOTHSTEP, 0.1),
              (_rz(0), _rz(90), 0.2, EASE_LINEAR, 0.5)]            # cur_elapsed > duration


def mix(n):
    """n mover specs.  Path movers: ("path", path name, initial_time, leader index in this list or None, follow_dist, flags, base_rot);
    move-to movers: ("moveto", position track index or None, rotation track index or None, hold_pos, hold_rot).  Leaders come before their followers."""
    cycle = [("path", "loop", 0.0, None, 0.0, ORIENT_ALONG_PATH, _rz(0)),
             ("path", "loop", 0.0, 0, 1.5, ORIENT_ALONG_PATH, _rz(0)),            # crosses one segment start now and then
             ("path", "loop", 0.0, 0, 9.0, 0, _rz(30)),                           # several
             ("moveto", 0, 0, (0, 0, 1), _rz(0)),
             ("path", "ring", 0.013, None, 0.0, ORIENT_ALONG_PATH, _rz(45)),
             ("path", "ring", 0.0, 4, 0.3, 0, _rz(0)),                            # several starts of the short segments
             ("path", "ring", 0.0, 4, 5.0, ORIENT_ALONG_PATH, _rz(0)),            # more than 64: the cap
             ("moveto", 1, None, (1, 2, 3), _rz(20)),
             ("path", "straight_curve", 3.3, None, 0.0, ORIENT_ALONG_PATH, (math.sin(0.2), 0.0, 0.0, math.cos(0.2))),
             ("path", "straight_curve", 0.0, 8, 0.0, 0, _rz(0)),                  # follow_dist 0: on the leader
             ("moveto", None, 1, (5, 5, 5), _rz(10)),
             ("moveto", 2, 3, (0, 0, 0), _rz(0)),
             ("path", "random7", 1.0e4 + 0.37, None, 0.0, ORIENT_ALONG_PATH, _rz(0)),
             ("path", "two", -0.3, None, 0.0, ORIENT_ALONG_PATH, _rz(0)),         # a negative time: the non-negative remainder
             ("moveto", 3, 2, (3, 0, 0), _rz(0)),
             ("path", "random128", 77.0, None, 0.0, 0, _rz(0)),
             ("path", "ring_fast", 0.0, None, 0.0, ORIENT_ALONG_PATH, _rz(0))]       # a frame hits the cap of 64 segment ends
    out = []
    for k in range(n):
        s = cycle[k % len(cycle)]
        base = k - k % len(cycle)
        if s[0] == "path":
            t0 = s[2] + 5.3 * (k // len(cycle))      # (spread over the loop's 17 s: station, arcs, entry and exit straights)
            leader = None if s[3] is None else base + s[3]
            s = ("path", s[1], t0, leader, s[4], s[5], s[6])
        out.append(s)
    return out
