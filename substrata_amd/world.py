"""Thin numpy/ctypes driver over the C ABI (include/sgp.h).

`CWorld` is ABI plumbing only: it owns no physics.  The product binds it to substrata_amd/libsgp.so (HIP, gfx950);
the test suite binds the same class to its CPU checker library (a different symbol prefix) so that parity tests
drive both sides through identical calls.
"""
import ctypes as C
import numpy as np
from . import abi


class SgpError(RuntimeError):
    pass


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _f3(v):
    return np.ascontiguousarray(v, dtype=np.float32).reshape(3)


def _f4(v):
    return np.ascontiguousarray(v, dtype=np.float32).reshape(4)


class _Owned:
    """A handle of the C ABI that belongs to a world and is destroyed by sgp_<_stem>_destroy: close() is idempotent, and runs when the object goes."""
    _stem = None

    def __init__(self, world, handle):
        self._w, self._h = world, handle

    def close(self):
        if self._h:
            self._w._fn(self._stem + "_destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Batch(_Owned):
    """A device-resident batch of one world: sgp_<_stem>_create with the capacities, update(); states() where the batch has a _state_dtype."""
    _state_dtype = None

    def __init__(self, world, *capacities):
        super().__init__(world, C.c_void_p())
        world._check(world._fn(self._stem + "_create")(world._h, *[int(c) for c in capacities], C.byref(self._h)), self._stem + "_create")
        self.capacity = int(capacities[0])
        self._update = world._fn(self._stem + "_update")

    def update(self, dt=1.0 / 60.0):
        self._w._check(self._update(self._h, float(dt)), self._stem + "_update")

    def states(self, first=0, n=None):
        n = self.capacity - first if n is None else int(n)
        out = np.zeros(n, dtype=self._state_dtype)
        self._w._check(self._w._fn(self._stem + "_get_states")(self._h, int(first), n, out.ctypes.data), self._stem + "_get_states")
        return out

    def checkpoint(self, cp=None):
        """Captures the batch's state; cp: a BatchCheckpoint of this batch to overwrite in place (its buffers are re-used).  Enqueues and returns."""
        if cp is None:
            h = C.c_void_p()
            self._w._check(self._w._fn(self._stem + "_checkpoint")(self._h, C.byref(h)), self._stem + "_checkpoint")
            return BatchCheckpoint(self._w, h)
        if not cp._h:
            raise SgpError("checkpoint: the BatchCheckpoint to overwrite has been closed")
        self._w._check(self._w._fn(self._stem + "_checkpoint")(self._h, C.byref(cp._h)), self._stem + "_checkpoint")
        return cp

    def rollback(self, cp):
        """The batch becomes what it was when cp was captured; pair it with CWorld.rollback to the checkpoint of the same moment."""
        if not cp._h:
            raise SgpError("rollback: the BatchCheckpoint has been closed")
        self._w._check(self._w._fn(self._stem + "_rollback")(self._h, cp._h), self._stem + "_rollback")


class BatchCheckpoint(_Owned):
    """A captured state of one batch (sgp_batch_checkpoint): owns device and host memory, belongs to the batch that made it."""
    _stem = "batch_checkpoint"

    def info(self):
        i = abi.BatchCheckpointInfo()
        self._w._check(self._w._fn("batch_checkpoint_get_info")(self._h, C.byref(i)), "batch_checkpoint_get_info")
        return i.as_dict()


class Checkpoint(_Owned):
    """A captured world state (sgp_checkpoint): owns device and host memory, belongs to the world that made it."""
    _stem = "checkpoint"

    def info(self):
        i = abi.CheckpointInfo()
        self._w._check(self._w._fn("checkpoint_get_info")(self._h, C.byref(i)), "checkpoint_get_info")
        return i.as_dict()

    def to_bytes(self):
        """The pointer-free blob CWorld.restore loads into a fresh world with the same description."""
        n = C.c_uint64(0)
        self._w._check(self._w._fn("checkpoint_write")(self._h, None, 0, C.byref(n)), "checkpoint_write")
        buf = np.empty(n.value, dtype=np.uint8)
        self._w._check(self._w._fn("checkpoint_write")(self._h, buf.ctypes.data, buf.nbytes, C.byref(n)), "checkpoint_write")
        return buf.tobytes()


class Characters(_Batch):
    """A batch of virtual characters of one world (sgp_characters): numpy in, numpy out.  update() enqueues and returns; states() waits."""
    _stem, _state_dtype = "characters", abi.character_state_dtype

    def __init__(self, world, capacity):
        super().__init__(world, capacity)

    def default_desc(self):
        d = abi.CharacterDesc()
        self._w._fn("default_character_desc")(C.byref(d))
        return d

    def add(self, desc, pos):
        i = C.c_uint32(0)
        self._w._check(self._w._fn("character_add")(self._h, C.byref(desc), _fp(_f3(pos)), C.byref(i)), "character_add")
        return int(i.value)

    def remove(self, i):
        self._w._check(self._w._fn("character_remove")(self._h, int(i)), "character_remove")

    def set_pose(self, ids, pos):
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(len(ids), 3)
        self._w._check(self._w._fn("characters_set_pose")(self._h, ids.ctypes.data, pos.ctypes.data, len(ids)), "characters_set_pose")

    def set_shape(self, i, radius, half_height, offset=(0.0, 0.0, 0.0)):
        self._w._check(self._w._fn("characters_set_shape")(self._h, int(i), float(radius), float(half_height), _fp(_f3(offset))), "characters_set_shape")

    def set_inputs(self, first, inputs):
        """inputs: array of abi.character_input_dtype (velocity, ignore_id, flags) for characters first, first + 1, ..."""
        inputs = np.ascontiguousarray(inputs, dtype=abi.character_input_dtype).reshape(-1)
        self._w._check(self._w._fn("characters_set_inputs")(self._h, int(first), len(inputs), inputs.ctypes.data), "characters_set_inputs")

    def drain_contacts(self, cap=4096):
        out = np.zeros(cap, dtype=abi.character_contact_dtype)
        n = C.c_uint32(0)
        self._w._check(self._w._fn("characters_drain_contacts")(self._h, out.ctypes.data, cap, C.byref(n)), "characters_drain_contacts")
        return out[:min(n.value, cap)].copy()

    # driven characters: PlayerPhysics::update's rule on the device
    def default_drive(self):
        d = abi.CharacterDrive()
        self._w._fn("default_character_drive")(C.byref(d))
        return d

    def set_drive(self, first, drives):
        """drives: array of abi.character_drive_dtype for characters first, first + 1, ...; in force until set again"""
        drives = np.ascontiguousarray(drives, dtype=abi.character_drive_dtype).reshape(-1)
        self._w._check(self._w._fn("characters_set_drive")(self._h, int(first), len(drives), drives.ctypes.data), "characters_set_drive")

    def jump(self, ids, cur_time):
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        self._w._check(self._w._fn("characters_jump")(self._h, ids.ctypes.data, len(ids), float(cur_time)), "characters_jump")

    def update_at(self, dt, cur_time):
        self._w._check(self._w._fn("characters_update_at")(self._h, float(dt), float(cur_time)), "characters_update_at")

    def drive_states(self, first=0, n=None):
        n = self.capacity - first if n is None else int(n)
        out = np.zeros(n, dtype=abi.character_drive_state_dtype)
        self._w._check(self._w._fn("characters_get_drive_states")(self._h, int(first), n, out.ctypes.data), "characters_get_drive_states")
        return out


class Movers(_Batch):
    """A batch of path and move-to controllers of one world (sgp_movers): update() enqueues and returns; states() waits."""
    _stem, _state_dtype = "movers", abi.mover_state_dtype

    def __init__(self, world, capacity, path_capacity):
        super().__init__(world, capacity, path_capacity)

    def add_path(self, waypoints):
        """waypoints: array of abi.path_waypoint_dtype (pos, type, pause_time, speed); returns the path id."""
        wp = np.ascontiguousarray(waypoints, dtype=abi.path_waypoint_dtype).reshape(-1)
        p = C.c_uint32(0)
        self._w._check(self._w._fn("movers_path_add")(self._h, wp.ctypes.data, len(wp), C.byref(p)), "movers_path_add")
        return int(p.value)

    def remove_path(self, path):
        self._w._check(self._w._fn("movers_path_remove")(self._h, int(path)), "movers_path_remove")

    def path_segments(self, path):
        out = np.zeros(abi.MOVER_MAX_WAYPOINTS, dtype=abi.path_segment_dtype)
        n = C.c_uint32(0)
        self._w._check(self._w._fn("movers_path_get")(self._h, int(path), out.ctypes.data, len(out), C.byref(n)), "movers_path_get")
        return out[:n.value].copy()

    def add_path_mover(self, body, path, initial_time=0.0, leader=None, follow_dist=0.0, base_rot=(0.0, 0.0, 0.0, 1.0), orient_along_path=False, tag=0):
        d = abi.MoverDesc(kind=abi.MOVER_PATH, body=int(body), flags=abi.MOVER_ORIENT_ALONG_PATH if orient_along_path else 0, path=int(path),
                          initial_time=float(initial_time), tag=int(tag), leader=abi.INVALID_ID if leader is None else int(leader), follow_dist=float(follow_dist))
        d.base_rot[:] = [float(x) for x in base_rot]
        d.hold_rot[3] = 1.0
        return self.add(d)

    def add_moveto_mover(self, body, hold_pos, hold_rot=(0.0, 0.0, 0.0, 1.0), tag=0):
        d = abi.MoverDesc(kind=abi.MOVER_MOVETO, body=int(body), leader=abi.INVALID_ID, tag=int(tag))
        d.base_rot[3] = 1.0
        d.hold_pos[:] = [float(x) for x in hold_pos]
        d.hold_rot[:] = [float(x) for x in hold_rot]
        return self.add(d)

    def add(self, desc):
        i = C.c_uint32(0)
        self._w._check(self._w._fn("mover_add")(self._h, C.byref(desc), C.byref(i)), "mover_add")
        return int(i.value)

    def remove(self, i):
        self._w._check(self._w._fn("mover_remove")(self._h, int(i)), "mover_remove")

    def set_position_track(self, i, start, target, duration, easing=abi.MOVER_EASE_LINEAR, cur_elapsed=0.0):
        a, b = (C.c_float * 3)(*[float(x) for x in start]), (C.c_float * 3)(*[float(x) for x in target])
        self._w._check(self._w._fn("movers_set_position_track")(self._h, int(i), a, b, float(duration), int(easing), float(cur_elapsed)), "movers_set_position_track")

    def set_rotation_track(self, i, start, target, duration, easing=abi.MOVER_EASE_LINEAR, cur_elapsed=0.0):
        a, b = (C.c_float * 4)(*[float(x) for x in start]), (C.c_float * 4)(*[float(x) for x in target])
        self._w._check(self._w._fn("movers_set_rotation_track")(self._h, int(i), a, b, float(duration), int(easing), float(cur_elapsed)), "movers_set_rotation_track")


class Proximity(_Batch):
    """A batch of proximity and zone watchers of one world (sgp_proximity): numpy in, numpy out.  update() enqueues and returns; states(), observers() and
    drain_events() wait."""
    _stem, _state_dtype = "proximity", abi.proximity_state_dtype

    def __init__(self, world, object_capacity, zone_capacity=16, event_capacity=4096):
        super().__init__(world, object_capacity, zone_capacity, event_capacity)
        self.event_capacity = int(event_capacity)

    def update(self):
        self._w._check(self._update(self._h), "proximity_update")

    def add(self, bodies, radius=20.0, flags=abi.PROX_WANT_NEAR | abi.PROX_WANT_ZONE, tags=None):
        """One call for all of `bodies`; radius, flags and tags are scalars or one value per body.  Returns the ids (uint32)."""
        bodies = np.ascontiguousarray(bodies, dtype=np.uint32).reshape(-1)
        d = np.zeros(len(bodies), dtype=abi.proximity_object_dtype)
        d["body"], d["radius"], d["flags"] = bodies, radius, flags
        d["tag"] = 0 if tags is None else tags
        ids = np.zeros(len(bodies), dtype=np.uint32)
        self._w._check(self._w._fn("proximity_add")(self._h, d.ctypes.data, len(d), ids.ctypes.data), "proximity_add")
        return ids

    def remove(self, i):
        self._w._check(self._w._fn("proximity_remove")(self._h, int(i)), "proximity_remove")

    def set_flags(self, i, flags):
        self._w._check(self._w._fn("proximity_set_flags")(self._h, int(i), int(flags)), "proximity_set_flags")

    def set_observer(self, k, pos=None, body=None, offset=(0.0, 0.0, 0.0)):
        """Observer k at `pos`, or riding `body` at the world-space `offset`."""
        o = abi.ProximityObserver(source=abi.PROX_OBS_POINT if body is None else abi.PROX_OBS_BODY, body=0 if body is None else int(body))
        o.pos[:] = [float(x) for x in ((0.0, 0.0, 0.0) if pos is None else pos)]
        o.offset[:] = [float(x) for x in offset]
        self._w._check(self._w._fn("proximity_set_observer")(self._h, int(k), C.byref(o)), "proximity_set_observer")

    def set_points(self, first, xyz):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        self._w._check(self._w._fn("proximity_set_points")(self._h, int(first), len(xyz), xyz.ctypes.data), "proximity_set_points")

    def remove_observer(self, k):
        self._w._check(self._w._fn("proximity_remove_observer")(self._h, int(k)), "proximity_remove_observer")

    def add_zone(self, mn, mx, key):
        z = C.c_uint32(0)
        self._w._check(self._w._fn("proximity_zone_add")(self._h, _fp(_f3(mn)), _fp(_f3(mx)), int(key), C.byref(z)), "proximity_zone_add")
        return int(z.value)

    def remove_zone(self, zone):
        self._w._check(self._w._fn("proximity_zone_remove")(self._h, int(zone)), "proximity_zone_remove")

    def observers(self, first=0, n=abi.PROX_MAX_OBSERVERS):
        out = np.zeros(int(n), dtype=abi.proximity_observer_state_dtype)
        self._w._check(self._w._fn("proximity_get_observers")(self._h, int(first), int(n), out.ctypes.data), "proximity_get_observers")
        return out

    def drain_events(self, cap=None):
        """(events since the last drain as abi.proximity_event_dtype, in their order; how many more did not fit event_capacity)"""
        cap = self.event_capacity if cap is None else int(cap)
        out = np.zeros(max(cap, 1), dtype=abi.proximity_event_dtype)
        n, dropped = C.c_uint32(0), C.c_uint32(0)
        self._w._check(self._w._fn("proximity_drain_events")(self._h, out.ctypes.data, cap, C.byref(n), C.byref(dropped)), "proximity_drain_events")
        return out[:min(n.value, cap)].copy(), int(dropped.value)


class Audibility(_Batch):
    """A batch of audio sources and listeners of one world (sgp_audibility): numpy in, numpy out.  update(cur_time) enqueues and returns; states(),
    pair_states(), listeners() and drain_events() wait."""
    _stem, _state_dtype = "audibility", abi.audibility_state_dtype

    def __init__(self, world, source_capacity, listener_capacity=1, event_capacity=4096):
        super().__init__(world, source_capacity, listener_capacity, event_capacity)
        self.listener_capacity, self.event_capacity = int(listener_capacity), int(event_capacity)
        self._prox = None

    def update(self, cur_time):
        self._w._check(self._update(self._h, float(cur_time)), "audibility_update")

    def add(self, descs):
        """descs: array of abi.audibility_source_dtype.  Returns the ids (uint32)."""
        d = np.ascontiguousarray(descs, dtype=abi.audibility_source_dtype).reshape(-1)
        ids = np.zeros(len(d), dtype=np.uint32)
        self._w._check(self._w._fn("audibility_add")(self._h, d.ctypes.data, len(d), ids.ctypes.data), "audibility_add")
        return ids

    def add_points(self, pos, volume=1.0, zone_key=abi.INVALID_ID, flags=abi.AUD_WANT_RANGE | abi.AUD_WANT_OCCLUSION | abi.AUD_WANT_VOLUME, tags=None):
        pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
        d = np.zeros(len(pos), dtype=abi.audibility_source_dtype)
        d["kind"], d["pos"], d["volume"], d["zone_key"], d["flags"] = abi.AUD_SRC_POINT, pos, volume, zone_key, flags
        d["tag"] = 0 if tags is None else tags
        return self.add(d)

    def add_bodies(self, bodies, volume=1.0, zone_key=abi.INVALID_ID, flags=abi.AUD_WANT_RANGE | abi.AUD_WANT_OCCLUSION | abi.AUD_WANT_VOLUME, tags=None):
        bodies = np.ascontiguousarray(bodies, dtype=np.uint32).reshape(-1)
        d = np.zeros(len(bodies), dtype=abi.audibility_source_dtype)
        d["kind"], d["body"], d["volume"], d["zone_key"], d["flags"] = abi.AUD_SRC_BODY, bodies, volume, zone_key, flags
        d["tag"] = 0 if tags is None else tags
        return self.add(d)

    def remove(self, i):
        self._w._check(self._w._fn("audibility_remove")(self._h, int(i)), "audibility_remove")

    def set_points(self, first, xyz):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        self._w._check(self._w._fn("audibility_set_points")(self._h, int(first), len(xyz), xyz.ctypes.data), "audibility_set_points")

    def set_volume(self, i, volume):
        self._w._check(self._w._fn("audibility_set_volume")(self._h, int(i), float(volume)), "audibility_set_volume")

    def set_flags(self, i, flags):
        self._w._check(self._w._fn("audibility_set_flags")(self._h, int(i), int(flags)), "audibility_set_flags")

    def set_listener(self, k, pos=None, body=None, offset=(0.0, 0.0, 0.0), ignore_body=abi.INVALID_ID, zone_key=abi.INVALID_ID, mute_outside=False):
        """Listener k at `pos`, or riding `body` at the world-space `offset`."""
        o = abi.AudibilityListener(source=abi.AUD_LST_POINT if body is None else abi.AUD_LST_BODY, body=0 if body is None else int(body),
                                   ignore_body=int(ignore_body), zone_key=int(zone_key), mute_outside=1 if mute_outside else 0)
        o.pos[:] = [float(x) for x in ((0.0, 0.0, 0.0) if pos is None else pos)]
        o.offset[:] = [float(x) for x in offset]
        self._w._check(self._w._fn("audibility_set_listener")(self._h, int(k), C.byref(o)), "audibility_set_listener")

    def remove_listener(self, k):
        self._w._check(self._w._fn("audibility_remove_listener")(self._h, int(k)), "audibility_remove_listener")

    def set_listener_points(self, first, xyz):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        self._w._check(self._w._fn("audibility_set_listener_points")(self._h, int(first), len(xyz), xyz.ctypes.data), "audibility_set_listener_points")

    def set_listener_zone(self, k, zone_key, mute_outside):
        self._w._check(self._w._fn("audibility_set_listener_zone")(self._h, int(k), int(zone_key), 1 if mute_outside else 0), "audibility_set_listener_zone")

    def set_transition(self, seconds):
        self._w._check(self._w._fn("audibility_set_transition")(self._h, float(seconds)), "audibility_set_transition")

    def attach_proximity(self, proximity=None):
        """Listener k takes its zone key from observer k of `proximity` on the device; None detaches."""
        self._w._check(self._w._fn("audibility_attach_proximity")(self._h, proximity._h if proximity is not None else None), "audibility_attach_proximity")
        self._prox = proximity

    def set_muting_keys(self, keys):
        keys = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1)
        self._w._check(self._w._fn("audibility_set_muting_keys")(self._h, keys.ctypes.data, len(keys)), "audibility_set_muting_keys")

    def pair_states(self, first=0, n=None):
        """abi.audibility_pair_state_dtype, shape (n, listener_capacity)."""
        n = self.capacity - first if n is None else int(n)
        out = np.zeros((n, self.listener_capacity), dtype=abi.audibility_pair_state_dtype)
        self._w._check(self._w._fn("audibility_get_pair_states")(self._h, int(first), n, out.ctypes.data), "audibility_get_pair_states")
        return out

    def listeners(self, first=0, n=None):
        n = self.listener_capacity - first if n is None else int(n)
        out = np.zeros(n, dtype=abi.audibility_listener_state_dtype)
        self._w._check(self._w._fn("audibility_get_listeners")(self._h, int(first), n, out.ctypes.data), "audibility_get_listeners")
        return out

    def drain_events(self, cap=None):
        """(events since the last drain as abi.audibility_event_dtype, in their order; how many more did not fit event_capacity)"""
        cap = self.event_capacity if cap is None else int(cap)
        out = np.zeros(max(cap, 1), dtype=abi.audibility_event_dtype)
        n, dropped = C.c_uint32(0), C.c_uint32(0)
        self._w._check(self._w._fn("audibility_drain_events")(self._h, out.ctypes.data, cap, C.byref(n), C.byref(dropped)), "audibility_drain_events")
        return out[:min(n.value, cap)].copy(), int(dropped.value)


class Crafts(_Batch):
    """A batch of hover cars and boats of one world (sgp_crafts): update() enqueues and returns; states() waits."""
    _stem, _state_dtype = "crafts", abi.craft_state_dtype

    def __init__(self, world, capacity):
        super().__init__(world, capacity)

    def default_desc(self, kind, body=None):
        d = abi.CraftDesc()
        self._w._fn("default_craft_desc")(int(kind), C.byref(d))
        if body is not None:
            d.body = int(body)
        return d

    def add(self, desc):
        i = C.c_uint32(0)
        self._w._check(self._w._fn("craft_add")(self._h, C.byref(desc), C.byref(i)), "craft_add")
        return int(i.value)

    def remove(self, i):
        self._w._check(self._w._fn("craft_remove")(self._h, int(i)), "craft_remove")

    def set_inputs(self, first, inputs):
        """inputs: array of abi.craft_input_dtype (forward, right, up, hand_brake, flags) for crafts first, first + 1, ..."""
        inputs = np.ascontiguousarray(inputs, dtype=abi.craft_input_dtype).reshape(-1)
        self._w._check(self._w._fn("crafts_set_inputs")(self._h, int(first), len(inputs), inputs.ctypes.data), "crafts_set_inputs")

    def start_righting(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        self._w._check(self._w._fn("crafts_start_righting")(self._h, ids.ctypes.data, len(ids)), "crafts_start_righting")

    def attach(self, particles=None):
        """The Particles batch of the same world that receives what the crafts raise (None: detach; emissions are then only counted)."""
        self._w._check(self._w._fn("crafts_attach_particles")(self._h, particles._h if particles is not None else None), "crafts_attach_particles")
        self._particles = particles      # (kept alive while attached)


class Particles(_Batch):
    """A batch of point particles of one world (sgp_particles): numpy in, numpy out.  add(), update() and clear() enqueue and return; read() and
    drain_events() wait.  (No states(): read() returns the live particles.)"""
    _stem = "particles"

    def __init__(self, world, capacity, event_capacity=4096):
        super().__init__(world, capacity, event_capacity)
        self.event_capacity = int(event_capacity)

    def defaults(self, n=1):
        """n records of abi.particle_dtype filled by sgp_default_particle (the defaults of the reference's Particle())."""
        d = abi.Particle()
        self._w._fn("default_particle")(C.byref(d))
        out = np.zeros(int(n), dtype=abi.particle_dtype)
        out[:] = np.frombuffer(bytes(d), dtype=abi.particle_dtype)[0]
        return out

    def add(self, particles):
        particles = np.ascontiguousarray(particles, dtype=abi.particle_dtype).reshape(-1)
        self._w._check(self._w._fn("particles_add")(self._h, particles.ctypes.data, len(particles)), "particles_add")

    def clear(self):
        self._w._check(self._w._fn("particles_clear")(self._h), "particles_clear")

    def read(self, cap=None):
        """The live particles in slot order (abi.particle_state_dtype)."""
        cap = self.capacity if cap is None else int(cap)
        out = np.zeros(cap, dtype=abi.particle_state_dtype)
        n = C.c_uint32(0)
        self._w._check(self._w._fn("particles_read")(self._h, out.ctypes.data, cap, C.byref(n)), "particles_read")
        return out[:min(n.value, cap)].copy()

    def drain_events(self, cap=None):
        """(events since the last drain as abi.particle_event_dtype, how many more did not fit event_capacity)"""
        cap = self.event_capacity if cap is None else int(cap)
        out = np.zeros(max(cap, 1), dtype=abi.particle_event_dtype)
        n, dropped = C.c_uint32(0), C.c_uint32(0)
        self._w._check(self._w._fn("particles_drain_events")(self._h, out.ctypes.data, cap, C.byref(n), C.byref(dropped)), "particles_drain_events")
        return out[:min(n.value, cap)].copy(), int(dropped.value)


class CWorld:
    def __init__(self, lib, prefix, max_bodies=65536, gravity=(0.0, 0.0, -9.81), device=0, settings=None,
                 max_body_pairs=0, max_manifolds=0, large_body_radius=0.0):
        self._lib, self._p = lib, prefix
        self._h = C.c_void_p()
        d = abi.WorldDesc()
        self._fn("default_world_desc")(C.byref(d))
        d.max_bodies = int(max_bodies)
        d.max_body_pairs = int(max_body_pairs)
        d.max_manifolds = int(max_manifolds)
        d.device = int(device)
        d.gravity[:] = gravity
        if large_body_radius:
            d.large_body_radius = float(large_body_radius)
        if settings:
            for k, v in settings.items():
                setattr(d.settings, k, v)
        self.desc = d
        self._check(self._fn("world_create")(C.byref(d), C.byref(self._h)), "world_create")
        self.max_bodies = int(max_bodies)

    # -- plumbing -------------------------------------------------------------------------------------------
    def _fn(self, name):
        return getattr(self._lib, self._p + name)

    def _check(self, rc, what):
        if rc != abi.OK:
            msg = ""
            fn = getattr(self._lib, self._p + "last_error", None)
            if fn is not None:
                m = fn()
                msg = m.decode() if m else ""
            raise SgpError(f"{self._p}{what} failed: rc={rc} {msg}")

    def close(self):
        if self._h:
            self._fn("world_destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- bodies ---------------------------------------------------------------------------------------------
    def default_body_desc(self):
        d = abi.BodyDesc()
        self._fn("default_body_desc")(C.byref(d))
        return d

    def add(self, desc):
        out = C.c_uint32(abi.INVALID_ID)
        rc = self._fn("body_add")(self._h, C.byref(desc), C.byref(out))
        if rc == abi.ERR_REJECTED:
            return abi.INVALID_ID
        self._check(rc, "body_add")
        return out.value

    def add_batch(self, descs):
        """descs: numpy structured array of abi.body_desc_dtype. Returns ids (uint32; INVALID_ID where rejected)."""
        descs = np.ascontiguousarray(descs, dtype=abi.body_desc_dtype)
        ids = np.empty(len(descs), dtype=np.uint32)
        self._check(self._fn("body_add_batch")(self._h, descs.ctypes.data, len(descs), ids.ctypes.data), "body_add_batch")
        return ids

    def add_compound(self, base_desc, children):
        """StaticCompoundShapeSettings::AddShape x n + Create on a static body (MeshBuilding.cpp:396-407).  base_desc: one record of
        abi.body_desc_dtype (pose, layer, material, userdata); children: array of abi.compound_child_dtype.  Returns the compound's id."""
        base = np.ascontiguousarray(base_desc, dtype=abi.body_desc_dtype).reshape(-1)[:1].copy()
        ch = np.ascontiguousarray(children, dtype=abi.compound_child_dtype)
        out = C.c_uint32(abi.INVALID_ID)
        self._check(self._fn("body_add_compound")(self._h, C.cast(base.ctypes.data, C.POINTER(abi.BodyDesc)), ch.ctypes.data, len(ch), C.byref(out)),
                    "body_add_compound")
        return out.value

    def compound_size(self, i):
        n = C.c_uint32(0)
        self._check(self._fn("body_compound_size")(self._h, int(i), C.byref(n)), "body_compound_size")
        return n.value

    def remove(self, i):
        self._check(self._fn("body_remove")(self._h, int(i)), "body_remove")

    def activate(self, i):
        self._check(self._fn("body_activate")(self._h, int(i)), "body_activate")

    def get_volume(self, i):
        v = C.c_float(0.0)
        self._check(self._fn("body_get_volume")(self._h, int(i), C.byref(v)), "body_get_volume")
        return v.value

    def set_layer(self, i, layer):
        self._check(self._fn("body_set_layer")(self._h, int(i), int(layer)), "body_set_layer")

    def set_pose_vel(self, i, pos, rot, lin_vel=(0, 0, 0), ang_vel=(0, 0, 0)):
        self._check(self._fn("body_set_pose_vel")(self._h, int(i), _fp(_f3(pos)), _fp(_f4(rot)), _fp(_f3(lin_vel)),
                                                  _fp(_f3(ang_vel))), "body_set_pose_vel")

    def set_pose_vel_batch(self, ids, recs):
        """Insert many physics snapshots at once (recs: structured array of abi.pose_vel_dtype)."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        recs = np.ascontiguousarray(recs, dtype=abi.pose_vel_dtype)
        fn = getattr(self._lib, self._p + "body_set_pose_vel_batch", None)
        if fn is None:      # the CPU checker has no batched entry point
            for i, r in zip(ids, recs):
                self.set_pose_vel(int(i), r["pos"], r["rot"], r["lin_vel"], r["ang_vel"])
            return
        self._check(fn(self._h, ids.ctypes.data, recs.ctypes.data, len(ids)), "body_set_pose_vel_batch")

    def set_pose_shape(self, i, pos, rot, shape):
        self._check(self._fn("body_set_pose_shape")(self._h, int(i), _fp(_f3(pos)), _fp(_f4(rot)), _fp(_f4(shape))),
                    "body_set_pose_shape")

    def set_pos(self, i, pos):
        self._check(self._fn("body_set_pos")(self._h, int(i), _fp(_f3(pos))), "body_set_pos")

    def set_vel(self, i, lin_vel, ang_vel):
        self._check(self._fn("body_set_vel")(self._h, int(i), _fp(_f3(lin_vel)), _fp(_f3(ang_vel))), "body_set_vel")

    def move_kinematic(self, i, pos, rot, dt):
        self._check(self._fn("body_move_kinematic")(self._h, int(i), _fp(_f3(pos)), _fp(_f4(rot)), float(dt)),
                    "body_move_kinematic")

    def add_force(self, i, f):
        self._check(self._fn("body_add_force")(self._h, int(i), _fp(_f3(f))), "body_add_force")

    def add_force_at(self, i, f, p):
        self._check(self._fn("body_add_force_at")(self._h, int(i), _fp(_f3(f)), _fp(_f3(p))), "body_add_force_at")

    def add_torque(self, i, t):
        self._check(self._fn("body_add_torque")(self._h, int(i), _fp(_f3(t))), "body_add_torque")

    def get_state(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        out = np.zeros(len(ids), dtype=abi.body_state_dtype)
        self._check(self._fn("body_get_state")(self._h, ids.ctypes.data, len(ids), out.ctypes.data), "body_get_state")
        return out

    def read_states(self, first=0, n=None):
        n = self.max_bodies - first if n is None else n
        out = np.zeros(n, dtype=abi.body_state_dtype)
        self._check(self._fn("world_read_states")(self._h, int(first), int(n), out.ctypes.data), "world_read_states")
        return out

    def read_active(self, cap=None, out=None):
        """States of the active bodies (the application's per-frame read-back).  `out`: a reusable caller-owned record array."""
        if out is not None:
            cap = len(out)
        else:
            cap = self.max_bodies if cap is None else cap
            out = np.zeros(cap, dtype=abi.body_state_dtype)
        n = C.c_uint32(0)
        self._check(self._fn("world_read_active")(self._h, out.ctypes.data, int(cap), C.byref(n)), "world_read_active")
        return out[:min(n.value, cap)]

    def read_active_view(self):
        """States of the active bodies as a read-only view of the library's pinned host buffer (no copy into a caller buffer);
        valid until the next read-back call on this world."""
        ptr = C.c_void_p(0)
        n = C.c_uint32(0)
        self._check(self._fn("world_read_active_view")(self._h, C.byref(ptr), C.byref(n)), "world_read_active_view")
        if n.value == 0:
            return np.zeros(0, dtype=abi.body_state_dtype)
        buf = (C.c_char * (n.value * abi.body_state_dtype.itemsize)).from_address(ptr.value)
        a = np.frombuffer(buf, dtype=abi.body_state_dtype, count=n.value)
        a.flags.writeable = False
        return a

    def read_active_poses_view(self):
        """Id, position and rotation of the active bodies (32-byte records) as a read-only view of the library's pinned host buffer;
        valid until the next read-back call on this world."""
        ptr = C.c_void_p(0)
        n = C.c_uint32(0)
        self._check(self._fn("world_read_active_poses_view")(self._h, C.byref(ptr), C.byref(n)), "world_read_active_poses_view")
        if n.value == 0:
            return np.zeros(0, dtype=abi.body_pose_dtype)
        buf = (C.c_char * (n.value * abi.body_pose_dtype.itemsize)).from_address(ptr.value)
        a = np.frombuffer(buf, dtype=abi.body_pose_dtype, count=n.value)
        a.flags.writeable = False
        return a

    # -- world ----------------------------------------------------------------------------------------------
    def set_water(self, enabled, z):
        self._check(self._fn("world_set_water")(self._h, int(bool(enabled)), float(z)), "world_set_water")

    def set_contact_events(self, enabled):
        self._check(self._fn("world_set_contact_events")(self._h, int(bool(enabled))), "world_set_contact_events")

    # -- checkpoints ----------------------------------------------------------------------------------------
    def checkpoint(self, cp=None):
        """Captures the world's state; cp: a Checkpoint of this world to overwrite in place (its buffers are re-used)."""
        if cp is None:
            h = C.c_void_p()
            self._check(self._fn("world_checkpoint")(self._h, C.byref(h)), "world_checkpoint")
            return Checkpoint(self, h)
        if not cp._h:
            raise SgpError("checkpoint: the Checkpoint to overwrite has been closed")
        self._check(self._fn("world_checkpoint")(self._h, C.byref(cp._h)), "world_checkpoint")      # (the library writes the handle it used back)
        return cp

    def rollback(self, cp):
        if not cp._h:
            raise SgpError("rollback: the Checkpoint has been closed")
        self._check(self._fn("world_rollback")(self._h, cp._h), "world_rollback")

    def restore(self, blob):
        """Loads a Checkpoint.to_bytes() blob into this world, which must be fresh and have the blob's description."""
        buf = np.frombuffer(bytes(blob), dtype=np.uint8)
        self._check(self._fn("world_restore")(self._h, buf.ctypes.data, buf.nbytes), "world_restore")

    def step(self, dt=1.0 / 60.0):
        self._check(self._fn("world_step")(self._h, float(dt)), "world_step")

    def step_n(self, dt, n):
        self._check(self._fn("world_step_n")(self._h, float(dt), int(n)), "world_step_n")

    def step_profiled(self, dt=1.0 / 60.0):
        p = abi.StepProfile()
        self._check(self._fn("world_step_profiled")(self._h, float(dt), C.byref(p)), "world_step_profiled")
        return p

    def stats(self):
        s = abi.StepStats()
        self._check(self._fn("world_stats")(self._h, C.byref(s)), "world_stats")
        return s

    def launch_counts(self):
        """(graph replays, eager steps, idle steps) so far -- product library only."""
        g, e, i = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self._check(self._fn("world_launch_counts")(self._h, C.byref(g), C.byref(e), C.byref(i)), "world_launch_counts")
        return g.value, e.value, i.value

    def num_bodies(self):
        n = C.c_uint32(0)
        self._check(self._fn("world_num_bodies")(self._h, C.byref(n)), "world_num_bodies")
        return n.value

    def event_counts(self):
        """Events waiting per kind (index = abi.EVENT_*), nothing drained -- product library only."""
        c = (C.c_uint32 * 5)()
        self._check(self._fn("world_event_counts")(self._h, c), "world_event_counts")
        return list(c)

    def drain_events(self, kind, cap=1 << 16):
        dt = abi.body_event_dtype if kind <= abi.EVENT_ENTERED_WATER else abi.contact_event_dtype
        n = C.c_uint32(0)
        while True:
            out = np.zeros(cap, dtype=dt)
            self._check(self._fn("world_drain_events")(self._h, int(kind), out.ctypes.data, int(cap), C.byref(n)),
                        "world_drain_events")
            return out[:min(n.value, cap)]

    def raycast(self, rays):
        rays = np.ascontiguousarray(rays, dtype=abi.ray_dtype)
        hits = np.zeros(len(rays), dtype=abi.hit_dtype)
        self._check(self._fn("raycast")(self._h, rays.ctypes.data, len(rays), hits.ctypes.data), "raycast")
        return hits

    def raycast_any(self, rays):
        """doesRayHitAnything, batched: one bool per ray, equal to `raycast(rays)["id"] != INVALID_ID` (the search leaves at the first hit)."""
        rays = np.ascontiguousarray(rays, dtype=abi.ray_dtype)
        hit = np.zeros(len(rays), dtype=np.uint8)
        self._check(self._fn("raycast_any")(self._h, rays.ctypes.data, len(rays), hit.ctypes.data), "raycast_any")
        return hit.astype(bool)

    # -- static triangle meshes -------------------------------------------------------------------------------------
    def mesh_create(self, vertices, triangles, materials=None):
        """MeshShapeSettings(vertices, triangles).Create(): returns abi.MeshInfo (mesh_id for static body descs).  `materials`: one
        user-data word per triangle (the material index ray hits report)."""
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(triangles, dtype=np.uint32).reshape(-1, 3)
        info = abi.MeshInfo()
        if materials is None:
            self._check(self._fn("mesh_create")(self._h, v.ctypes.data, len(v), t.ctypes.data, len(t), C.byref(info)), "mesh_create")
        else:
            m = np.ascontiguousarray(materials, dtype=np.uint32).reshape(len(t))
            self._check(self._fn("mesh_create_with_materials")(self._h, v.ctypes.data, len(v), t.ctypes.data, len(t), m.ctypes.data, C.byref(info)),
                        "mesh_create_with_materials")
        return info

    def heightfield_create(self, heights, offset, spacing, scale=(1.0, 1.0, 1.0), quad_materials=None):
        """HeightFieldShapeSettings(heights, offset, spacing).Create() for a static terrain chunk: a W x W array of heights (row z, column x),
        heights along local +y.  Returns abi.MeshInfo: the field is an entry of the mesh table (SGP_SHAPE_MESH, shape[0] = mesh_id).
        `spacing`: a number or (x, z); `quad_materials`: one word per quad, (W - 1) x (W - 1), or None."""
        h = np.ascontiguousarray(heights, dtype=np.float32)
        if h.ndim == 2:
            if h.shape[0] != h.shape[1]:
                raise ValueError(f"heightfield_create: heights must be square, got {h.shape}")
            w = int(h.shape[0])
        elif h.ndim == 1:
            w = int(round(np.sqrt(h.size)))
            if w * w != h.size:
                raise ValueError(f"heightfield_create: {h.size} heights is not W * W")
        else:
            raise ValueError(f"heightfield_create: heights must be W x W or W * W values, got shape {h.shape}")
        h = h.reshape(-1)
        sp = (float(spacing), float(spacing)) if np.ndim(spacing) == 0 else tuple(float(x) for x in spacing)
        d = abi.HeightfieldDesc()
        d.heights = h.ctypes.data
        d.sample_count = w
        d.offset[:] = [float(x) for x in offset]
        d.spacing[:] = sp
        d.scale[:] = [float(x) for x in scale]
        m = None
        if quad_materials is not None:
            m = np.ascontiguousarray(quad_materials, dtype=np.uint32).reshape(-1)
            if w < 2 or m.size != (w - 1) * (w - 1):
                raise ValueError(f"heightfield_create: {m.size} quad materials for a {w} x {w} field, (W - 1)^2 expected")
            d.quad_materials = m.ctypes.data
        info = abi.MeshInfo()
        self._check(self._fn("heightfield_create")(self._h, C.byref(d), C.byref(info)), "heightfield_create")
        return info

    def mesh_destroy(self, mesh_id):
        self._check(self._fn("mesh_destroy")(self._h, int(mesh_id)), "mesh_destroy")

    def hull_destroy(self, hull_id):
        self._check(self._fn("hull_destroy")(self._h, int(hull_id)), "hull_destroy")

    # -- convex hulls ---------------------------------------------------------------------------------------------
    def hull_create(self, points, com_offset=None):
        """ConvexHullShapeSettings(points).Create() (wrapped in OffsetCenterOfMassShape when com_offset is given): returns
        abi.HullInfo (hull_id for body descs, com / rot = body frame in the frame of the points)."""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        info = abi.HullInfo()
        if com_offset is None:
            self._check(self._fn("hull_create")(self._h, pts.ctypes.data, len(pts), C.byref(info)), "hull_create")
        else:
            self._check(self._fn("hull_create_com")(self._h, pts.ctypes.data, len(pts), _fp(_f3(com_offset)), C.byref(info)), "hull_create_com")
        return info

    # -- wheeled vehicles ---------------------------------------------------------------------------------------
    def default_vehicle_desc(self, body=None):
        d = abi.VehicleDesc()
        self._fn("default_vehicle_desc")(C.byref(d))
        if body is not None:
            d.body = int(body)
        return d

    def vehicle_create(self, desc):
        out = C.c_uint32(abi.INVALID_ID)
        self._check(self._fn("vehicle_create")(self._h, C.byref(desc), C.byref(out)), "vehicle_create")
        return out.value

    def vehicle_destroy(self, vid):
        self._check(self._fn("vehicle_destroy")(self._h, int(vid)), "vehicle_destroy")

    def vehicle_set_input(self, vid, forward=0.0, right=0.0, brake=0.0, hand_brake=0.0):
        i = abi.VehicleInput(float(forward), float(right), float(brake), float(hand_brake))
        self._check(self._fn("vehicle_set_input")(self._h, int(vid), C.byref(i)), "vehicle_set_input")

    def vehicle_set_inputs(self, first, inputs):
        inputs = np.ascontiguousarray(inputs, dtype=abi.vehicle_input_dtype)
        self._check(self._fn("vehicle_set_inputs")(self._h, int(first), len(inputs), inputs.ctypes.data), "vehicle_set_inputs")

    def vehicle_get_state(self, vid):
        return self.vehicle_get_states(vid, 1)[0]

    def vehicle_get_states(self, first, n):
        out = np.zeros(n, dtype=abi.vehicle_state_dtype)
        self._check(self._fn("vehicle_get_states")(self._h, int(first), int(n), out.ctypes.data), "vehicle_get_states")
        return out

    def vehicle_enable_lean_controller(self, vid, enabled=True):
        self._check(self._fn("vehicle_enable_lean_controller")(self._h, int(vid), int(bool(enabled))), "vehicle_enable_lean_controller")

    def vehicle_reset_drivetrain(self, vid, engine_rpm=0.0, wheel_angular_velocity=0.0):
        self._check(self._fn("vehicle_reset_drivetrain")(self._h, int(vid), float(engine_rpm), float(wheel_angular_velocity)),
                    "vehicle_reset_drivetrain")

    def particles(self, capacity, event_capacity=4096):
        """A batch of up to `capacity` point particles that belongs to this world."""
        return Particles(self, capacity, event_capacity)

    def crafts(self, capacity):
        """A batch of up to `capacity` hover cars and boats that belongs to this world (close it before the world)."""
        return Crafts(self, capacity)

    def movers(self, capacity, path_capacity=16):
        """A batch of up to `capacity` path and move-to controllers over `path_capacity` shared paths that belongs to this world (close it before the world)."""
        return Movers(self, capacity, path_capacity)

    def audibility(self, source_capacity, listener_capacity=1, event_capacity=4096):
        """A batch of audio sources and listeners of this world (sgp_audibility)."""
        return Audibility(self, source_capacity, listener_capacity, event_capacity)

    def proximity(self, object_capacity, zone_capacity=16, event_capacity=4096):
        """A batch of up to `object_capacity` watched objects, `zone_capacity` zones and 32 observers that belongs to this world (close it before the world)."""
        return Proximity(self, object_capacity, zone_capacity, event_capacity)

    def characters(self, capacity):
        """A batch of up to `capacity` virtual characters that belongs to this world (close it before the world)."""
        return Characters(self, capacity)

    def collide_capsules(self, queries, cap=4096):
        queries = np.ascontiguousarray(queries, dtype=abi.capsule_query_dtype)
        out = np.zeros(cap, dtype=abi.query_contact_dtype)
        n = C.c_uint32(0)
        self._check(self._fn("collide_capsules")(self._h, queries.ctypes.data, len(queries), out.ctypes.data, int(cap), C.byref(n)), "collide_capsules")
        return out[:min(n.value, cap)]

    def collide_shapes(self, queries, cap=4096):
        """sgp_collide_shapes: overlap queries with spheres, boxes, capsules and hulls (array of abi.shape_query_dtype).  Returns (records, n_total):
        the first min(n_total, cap) records of the whole answer sorted by (query, body, point), and the size of that whole answer."""
        queries = np.ascontiguousarray(queries, dtype=abi.shape_query_dtype)
        out = np.zeros(cap, dtype=abi.query_contact_dtype)
        n = C.c_uint32(0)
        self._check(self._fn("collide_shapes")(self._h, queries.ctypes.data, len(queries), out.ctypes.data, int(cap), C.byref(n)), "collide_shapes")
        return out[:min(n.value, cap)], n.value

    def cast_shapes(self, casts):
        """sgp_cast_shapes: the closest hit of every cast (array of abi.shape_cast_dtype) as an array of abi.cast_hit_dtype; id == abi.INVALID_ID: a miss."""
        casts = np.ascontiguousarray(casts, dtype=abi.shape_cast_dtype)
        hits = np.zeros(len(casts), dtype=abi.cast_hit_dtype)
        self._check(self._fn("cast_shapes")(self._h, casts.ctypes.data, len(casts), hits.ctypes.data), "cast_shapes")
        return hits

    def cast_shapes_counters(self):
        """(pairs of all sgp_cast_shapes calls so far that ran into the iteration cap, runs repeated because a candidate list was too small)"""
        out = (C.c_uint32 * 2)()
        self._check(self._fn("cast_shapes_counters")(self._h, out), "cast_shapes_counters")
        return int(out[0]), int(out[1])

    def spherecast(self, rays, radii):
        rays = np.ascontiguousarray(rays, dtype=abi.ray_dtype)
        radii = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, dtype=np.float32), (len(rays),)), dtype=np.float32)
        hits = np.zeros(len(rays), dtype=abi.hit_dtype)
        self._check(self._fn("spherecast")(self._h, rays.ctypes.data, radii.ctypes.data, len(rays), hits.ctypes.data), "spherecast")
        return hits

    def dump_constraints(self, cap=None):
        cap = (8 * self.max_bodies + 1024) if cap is None else cap
        out = np.zeros(cap, dtype=abi.constraint_dump_dtype)
        n = C.c_uint32(0)
        self._check(self._fn("world_dump_constraints")(self._h, out.ctypes.data, int(cap), C.byref(n)),
                    "world_dump_constraints")
        return out[:min(n.value, cap)]

    def export_boundary(self, lo, hi, margin, cap=1 << 16):
        out = np.empty(cap, dtype=abi.ghost_dtype)          # only the records the call fills in are returned
        n = C.c_uint32(0)
        self._check(self._fn("world_export_boundary")(self._h, _fp(_f3(lo)), _fp(_f3(hi)), float(margin),
                                                      out.ctypes.data, int(cap), C.byref(n)), "world_export_boundary")
        return out[:min(n.value, cap)]

    def import_ghosts(self, recs):
        recs = np.ascontiguousarray(recs, dtype=abi.ghost_dtype)
        self._check(self._fn("world_import_ghosts")(self._h, recs.ctypes.data, len(recs)), "world_import_ghosts")
