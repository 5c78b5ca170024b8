"""The two host exports of the audio sources' batch (sgp_audibility_pair_ray, sgp_audibility_ramp_step: sgp_audibility_math.h compiled for the host, the code
the device runs) against the numpy restatement of docs/CONTRACT.md 4m (tests/audibility_reference.py): 10 000 seeded cases each, equal to the bit, the exact
boundary cases, and both outcomes of every branch well represented.  No device."""
import ctypes as C

import numpy as np
import pytest

from substrata_amd import abi, build
import audibility_reference as ar

F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(build.build())
    abi.bind(lib, "sgp_")
    return lib


def f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def host_pair_ray(lib, ps, pl, volume, before):
    inr, tr, dist, trace, d = C.c_uint32(7), C.c_uint32(7), C.c_float(-1.0), C.c_float(-1.0), (C.c_float * 3)(9, 9, 9)
    assert lib.sgp_audibility_pair_ray(f3(ps), f3(pl), float(volume), int(before), C.byref(inr), C.byref(tr), C.byref(dist), d, C.byref(trace)) == abi.OK
    return bool(inr.value), bool(tr.value), F32(dist.value), np.array(list(d), F32), F32(trace.value)


def restated_pair_ray(ps, pl, volume, before):
    dx, dy, dz, d2, maxd, max2 = ar.geometry(ps, pl, volume)
    now = ar.range_step(np.asarray(before, bool), d2, max2)
    tr, dist = ar.traced(now, d2, maxd)
    dirs, trace = ar.pair_ray(dx, dy, dz, dist)
    dist = np.where(tr, dist, F32(0)); dirs = np.where(tr[..., None], dirs, F32(0)); trace = np.where(tr, trace, F32(0))
    return now, tr, dist.astype(F32), dirs.astype(F32), trace.astype(F32), d2, max2, maxd


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def check_pairs(lib, ps, pl, volume, before):
    now, tr, dist, dirs, trace, d2, max2, maxd = restated_pair_ray(ps, pl, volume, before)
    for i in range(len(ps)):
        h = host_pair_ray(lib, ps[i], pl[i], volume[i], before[i])
        assert h[0] == now[i] and h[1] == tr[i], i
        assert bits(h[2]) == bits(dist[i]) and np.array_equal(bits(h[3]), bits(dirs[i])) and bits(h[4]) == bits(trace[i]), i
    return now, tr, dist, dirs, trace, d2, max2, maxd


def test_pair_rays_equal_the_restatement_on_seeded_cases(lib):
    rng = np.random.default_rng(31)
    n = 10000
    pl = rng.uniform(-300, 300, (n, 3)).astype(F32)
    volume = rng.uniform(0.0, 2.5, n).astype(F32)
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    frac = rng.uniform(0.0, 1.4, n)
    frac[::7] = rng.uniform(0.0, 0.02, n)[::7]                                 # close by: dist in [0, 1] for most volumes
    ps = (pl + u * (60.0 * volume * frac)[:, None]).astype(F32)
    ps[::53] = pl[::53]                                                        # on top of the listener: dist == 0
    # exactly on the boundary (d2 == max2 and dist == maxd: in range, not traced): along an axis from a listener at the origin
    edge = np.flatnonzero(np.arange(n) % 11 == 0)
    pl[edge] = 0; ps[edge] = 0
    ps[edge, edge % 3] = F32(60.0) * volume[edge]
    before = rng.integers(0, 2, n).astype(bool)
    now, tr, dist, dirs, trace, d2, max2, maxd = check_pairs(lib, ps, pl, volume, before)
    assert (d2[edge] == max2[edge]).all() and now[edge].all() and not tr[edge].any()
    # both outcomes of every branch, well represented
    leaves, enters = before & ~now, ~before & now
    assert leaves.sum() > 500 and enters.sum() > 1500 and (before & now).sum() > 1500 and (~before & ~now).sum() > 500
    assert tr.sum() > 3000 and (now & ~tr).sum() >= 50 and (~now).sum() > 1000      # in range and not traced: volume 0, or dist rounding onto maxd
    assert (tr & (dist == 0)).sum() >= 100 and (tr & (dist > 0)).sum() > 3000
    assert (tr & (trace == 0)).sum() > 300 and (tr & (trace == 60)).sum() > 300 and (tr & (trace > 0) & (trace < 60)).sum() > 1500
    d = dirs[tr & (dist > 0)]
    assert np.max(np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0)) < 1e-6


def test_pair_rays_on_the_exact_boundaries(lib):
    """dist exactly maxd and its two float neighbours, d2 exactly max2, dist == 0, dist in [0, 1], dist > 61: along one axis from a listener at the origin, where
    dx is the coordinate itself and sqrt(x * x) is x again."""
    volumes = np.array([0.25, 0.5, 1.0, 1.5, 2.0, 0.7, 1.1, 0.013], F32)
    for v in volumes:
        maxd = F32(60.0) * v
        below, above = np.nextafter(maxd, F32(0)), np.nextafter(maxd, F32(np.inf))
        for axis in range(3):
            def at(x):
                p = np.zeros(3, F32); p[axis] = x
                return p
            zero = np.zeros(3, F32)
            for before in (False, True):
                # exactly on the boundary: d2 == max2 -- enters, does not leave -- and dist == maxd: not traced
                inr, tr, dist, d, trace = host_pair_ray(lib, at(maxd), zero, v, before)
                assert inr and not tr and dist == 0 and trace == 0
                # one float inside: in range, traced
                inr, tr, dist, d, trace = host_pair_ray(lib, at(below), zero, v, before)
                assert inr and tr and dist == below and d[axis] == 1 and trace == min(max(below - F32(1), F32(0)), F32(60))
                # one float outside: never enters, leaves
                inr, tr, dist, d, trace = host_pair_ray(lib, at(above), zero, v, before)
                assert not inr and not tr
            ps = np.stack([at(maxd), at(below), at(above), at(-below)])
            check_pairs(lib, ps, np.zeros((4, 3), F32), np.full(4, v, F32), np.array([False, True, True, False]))
    # dist == 0: direction (1, 0, 0), nothing traced beyond the listener
    p = np.array([3.5, -2.0, 7.25], F32)
    inr, tr, dist, d, trace = host_pair_ray(lib, p, p, 1.0, False)
    assert inr and tr and dist == 0 and tuple(d) == (1, 0, 0) and trace == 0
    # dist in [0, 1]: trace length 0; dist > 61: trace length 60
    for x in (0.001, 0.5, 1.0):
        inr, tr, dist, d, trace = host_pair_ray(lib, (x, 0, 0), (0, 0, 0), 1.0, False)
        assert tr and dist == F32(x) and trace == 0
    for x, want in ((1.5, 0.5), (61.0, 60.0), (61.5, 60.0), (100.0, 60.0)):
        inr, tr, dist, d, trace = host_pair_ray(lib, (0, x, 0), (0, 0, 0), 2.0, True)
        assert tr and trace == F32(want)
    assert lib.sgp_audibility_pair_ray(None, f3(p), 1.0, 0, None, None, None, None, None) == abi.ERR_INVALID


def host_ramp(lib, r, mute, cur_time, transition):
    changed = C.c_uint32(7)
    assert lib.sgp_audibility_ramp_step(C.byref(r), 1 if mute else 0, float(cur_time), float(transition), C.byref(changed)) == abi.OK
    return bool(changed.value)


def test_ramps_equal_the_restatement_over_seeded_sequences(lib):
    """50 sequences of 200 updates at irregular times, the mute decision flipping at seeded moments -- also in mid-ramp --, some with a transition shorter
    than 1e-4, cur_time going backwards once in each: all five variables after every update."""
    rng = np.random.default_rng(32)
    n_seq, n_upd = 50, 200
    transition = np.where(np.arange(n_seq) % 5 == 4, rng.uniform(1e-6, 9e-5, n_seq), np.where(np.arange(n_seq) % 5 == 3, rng.uniform(0.05, 0.3, n_seq), 1.0))
    model = ar.fresh_ramp((n_seq,))
    host = [abi.AudibilityRamp(-2.0, -1.0, 1.0, 1.0, 1.0, 0) for _ in range(n_seq)]
    t = rng.uniform(0.0, 1000.0, n_seq)
    mute = np.zeros(n_seq, bool)
    back_at = rng.integers(20, n_upd - 20, n_seq)
    counts = {k: 0 for k in ("muting_started", "unmuting_started", "ramping", "settled", "changed", "unchanged", "mid_ramp_flip", "tiny_span", "backwards")}
    for upd in range(n_upd):
        dt = rng.choice([0.004, 0.016, 0.033, 0.1, 0.4], n_seq) * rng.uniform(0.5, 1.5, n_seq)
        back = back_at == upd
        t = np.where(back, t - rng.uniform(0.1, 0.6, n_seq), t + dt)
        flip = rng.random(n_seq) < 0.06
        mute = mute ^ flip
        before = {k: v.copy() for k, v in model.items()}
        changed, what = ar.ramp_step(model, mute, t, transition)
        for i in range(n_seq):
            assert host_ramp(lib, host[i], mute[i], t[i], transition[i]) == changed[i], (upd, i)
            h = host[i]
            assert (h.mute_change_start_time, h.mute_change_end_time) == (model["start"][i], model["end"][i]), (upd, i)
            assert np.array_equal(bits([h.mute_volume_factor, h.mute_vol_fac_start, h.mute_vol_fac_end]),
                                  bits([model["factor"][i], model["fac_start"][i], model["fac_end"][i]])), (upd, i)
        started = what["muting_started"] | what["unmuting_started"]
        counts["muting_started"] += int(what["muting_started"].sum()); counts["unmuting_started"] += int(what["unmuting_started"].sum())
        counts["ramping"] += int(what["ramping"].sum()); counts["settled"] += int((~what["ramping"]).sum())
        counts["changed"] += int(changed.sum()); counts["unchanged"] += int((~changed).sum())
        counts["mid_ramp_flip"] += int((started & (before["factor"] != before["fac_end"])).sum())
        counts["tiny_span"] += int(((t < model["end"]) & ((model["end"] - model["start"]) <= 1.0e-4)).sum())
        counts["backwards"] += int(back.sum())
    print(counts)
    assert counts["muting_started"] >= 100 and counts["unmuting_started"] >= 100 and counts["mid_ramp_flip"] >= 30
    assert counts["ramping"] >= 1000 and counts["settled"] >= 3000 and counts["changed"] >= 1000 and counts["unchanged"] >= 3000
    assert counts["tiny_span"] >= 5 and counts["backwards"] == n_seq
    assert lib.sgp_audibility_ramp_step(None, 0, 0.0, 1.0, None) == abi.ERR_INVALID
