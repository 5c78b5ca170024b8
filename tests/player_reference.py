"""PlayerPhysics::update's velocity rule (gui_client/PlayerPhysics.cpp:256-342) and what follows its ExtendedUpdate (:450-461), restated in numpy float32 from
the reference's text, one scalar operation at a time, independently of substrata_amd/csrc/sgp_player_rule.h.  float64 appears only in the jump window
(time_since_jump_pressed is a double there, JUMP_PERIOD the float 0.1f promoted).

glare-core's Vec3f is absent; the forms taken for it are the ones docs/CONTRACT.md 4n lists as UNVERIFIED: length = sqrt((x*x + y*y) + z*z), normalise = v / length,
setLength(l) = v * (l / length), myMin(a, b) = a if a < b else b, myClamp(x, lo, hi) = max(lo, min(x, hi)), removeComponentInDir(v, d) = v - d * dot(v, d)."""
import numpy as np

F = np.float32
DRIVE_ON, DRIVE_FLY, DRIVE_GRAVITY, DRIVE_FREE_CAMERA, DRIVE_SMOOTH_STAIRS = 1, 2, 4, 8, 16
JUMP_PERIOD = F(0.1)


def vec(x, y, z):
    return [F(x), F(y), F(z)]


def add(a, b):
    return [a[0] + b[0], a[1] + b[1], a[2] + b[2]]


def sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def mul(a, s):
    return [a[0] * s, a[1] * s, a[2] * s]


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def length(a):
    return np.sqrt(dot(a, a))


def my_min(a, b):
    return a if a < b else b


def my_max(a, b):
    return a if a > b else b


def my_clamp(x, lo, hi):
    return my_max(lo, my_min(x, hi))


def submerged_fraction(water_enabled, water_z, feet_z, eye_height):
    if not water_enabled:
        return F(0)
    return my_clamp((water_z - feet_z) / eye_height, F(0), F(1))


def jump_due(cur_time, last_jump_time):
    return bool((np.float64(cur_time) - np.float64(last_jump_time)) < np.float64(JUMP_PERIOD))


def update(vel, move, move_up, flags, supported, ground_vel, ground_normal, feet_z, water_enabled, water_z, dt, due, jump_speed, max_air_speed, eye_height, campos_z_delta):
    """Returns dict(vel, move, on_ground, jumped, allow_sliding, fraction_submerged, campos_z_delta).  All floats np.float32, vectors lists of three."""
    with np.errstate(all="ignore"):
        fly, gravity = bool(flags & DRIVE_FLY), bool(flags & DRIVE_GRAVITY)
        wet = submerged_fraction(water_enabled, water_z, feet_z, eye_height)
        # processMoveUp: move_desired_vel += Vec3f(0,0,1) * (factor * move_speed * run factor), where it is honoured
        if fly or (flags & DRIVE_FREE_CAMERA) or wet > F(0.3):
            move = add(move, mul(vec(0, 0, 1), move_up))
        allow_sliding = bool(move[0] != 0 or move[1] != 0 or move[2] != 0)
        v = list(vel)
        if not fly:
            par = list(move)
            if wet < F(0.3):
                par[2] = F(0)
            if supported and (v[2] - ground_vel[2]) < F(0.1):
                v = add(par, ground_vel)
            else:
                if length(par) > max_air_speed:
                    par = mul(par, max_air_speed / length(par))
                v = add(v, mul(par, dt))
            if gravity:
                v = add(v, mul(vec(0, 0, -9.81), dt))
                v = add(v, mul([F(0), F(0), F(9.81) * F(1.1) * wet], dt))
                v = mul(v, F(1) - my_min(F(0.2), F(2.0) * wet * dt))
            if v[2] < F(-100):
                v[2] = F(-100)
        else:
            speed = length(v)
            if length(move) < F(1.0e-4):
                desired = vec(0, 0, 0)
            else:
                l = length(move)
                desired = mul([move[0] / l, move[1] / l, move[2] / l], speed)
            accel = add(mul(move, F(3)), mul(sub(desired, v), F(2)))
            v = add(v, mul(accel, dt))
        c = campos_z_delta - F(20) * dt * campos_z_delta
        if abs(c) < F(1.0e-5):
            c = F(0)
        on_ground = bool(supported and (vel[2] - ground_vel[2]) < F(0.1))
        jumped = False
        if due and supported:
            on_ground = False
            if fly:
                v = add(v, [F(0), F(0), jump_speed])
            else:
                v = add(add(sub(move, mul(ground_normal, dot(move, ground_normal))), ground_vel), [F(0), F(0), jump_speed])
            jumped = True
        return dict(vel=v, move=move, on_ground=on_ground, jumped=jumped, allow_sliding=allow_sliding, fraction_submerged=wet, campos_z_delta=c)


def camera(pos, vel, supported, ground_vel, dz, eye_height, campos_z_delta):
    with np.errstate(all="ignore"):
        c = my_clamp(campos_z_delta + dz, F(-0.3), F(0.3))
        rel = sub(vel, ground_vel) if supported else list(vel)
        rel[2] = F(0)
        return dict(campos_z_delta=c, last_xy=rel, cam_pos=[pos[0], pos[1], pos[2] + eye_height - c])
