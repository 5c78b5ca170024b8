"""ctypes mirror of include/sgp.h (the C ABI behind Substrata's PhysicsWorld facade).

Struct layouts, constants and prototypes here must stay in lock-step with include/sgp.h; tests/test_abi.py
checks sizes/offsets against the compiled library (sgp_abi_sizeof) and that every declared symbol is exported.
"""
import ctypes as C
import numpy as np

ABI_VERSION = 1

OK, ERR_INVALID, ERR_NO_DEVICE, ERR_CAPACITY, ERR_HIP, ERR_BAD_ID, ERR_REJECTED, ERR_PEER = 0, -1, -2, -3, -4, -5, -6, -7

MOTION_STATIC, MOTION_KINEMATIC, MOTION_DYNAMIC = 0, 1, 2
LAYER_NON_MOVING, LAYER_MOVING, LAYER_NON_MOVING_NON_COLLIDABLE, LAYER_MOVING_NON_COLLIDABLE = 0, 1, 2, 3
NUM_LAYERS = 4
SHAPE_SPHERE, SHAPE_BOX, SHAPE_CAPSULE, SHAPE_HULL, SHAPE_MESH = 0, 1, 2, 3, 4
INVALID_ID = 0xFFFFFFFF

EVENT_ACTIVATED, EVENT_DEACTIVATED, EVENT_ENTERED_WATER, EVENT_CONTACT_ADDED, EVENT_CONTACT_PERSISTED = 0, 1, 2, 3, 4
NUM_STAGES = 8
STAGE_NAMES = ["apply_forces", "broadphase", "narrowphase", "setup", "solve_velocity", "integrate",
               "solve_position", "finalize"]

f32, i32, u32, u64 = C.c_float, C.c_int32, C.c_uint32, C.c_uint64


class Settings(C.Structure):
    _fields_ = [("num_velocity_steps", i32), ("num_position_steps", i32), ("baumgarte", f32),
                ("penetration_slop", f32), ("speculative_contact_distance", f32),
                ("min_velocity_for_restitution", f32), ("max_penetration_distance", f32),
                ("time_before_sleep", f32), ("point_velocity_sleep_threshold", f32),
                ("contact_point_preserve_lambda_max_dist_sq", f32), ("max_linear_velocity", f32),
                ("max_angular_velocity", f32), ("allow_sleeping", i32), ("warm_start", i32), ("use_body_pair_contact_cache", i32),
                ("body_pair_cache_max_delta_position_sq", f32), ("body_pair_cache_cos_max_delta_rotation_div2", f32)]


class WorldDesc(C.Structure):
    _fields_ = [("max_bodies", u32), ("max_body_pairs", u32), ("max_manifolds", u32), ("device", i32),
                ("gravity", f32 * 3), ("large_body_radius", f32), ("settings", Settings)]


class BodyDesc(C.Structure):
    _fields_ = [("pos", f32 * 3), ("rot", f32 * 4), ("lin_vel", f32 * 3), ("ang_vel", f32 * 3),
                ("shape_type", i32), ("shape", f32 * 4), ("motion_type", i32), ("layer", i32),
                ("mass", f32), ("friction", f32), ("restitution", f32), ("gravity_factor", f32),
                ("linear_damping", f32), ("angular_damping", f32), ("is_sensor", i32),
                ("allow_sleeping", i32), ("activate", i32), ("use_zero_linear_drag", i32), ("userdata", u64)]


class BodyState(C.Structure):
    _fields_ = [("pos", f32 * 3), ("rot", f32 * 4), ("lin_vel", f32 * 3), ("ang_vel", f32 * 3),
                ("active", u32), ("underwater", u32), ("submerged_volume", f32), ("id", u32)]


class BodyPose(C.Structure):
    _fields_ = [("pos", f32 * 3), ("id", u32), ("rot", f32 * 4)]


class PoseVel(C.Structure):
    _fields_ = [("pos", f32 * 3), ("rot", f32 * 4), ("lin_vel", f32 * 3), ("ang_vel", f32 * 3)]


PHYSICS_UPDATE_BYTES = 80


class BodyEvent(C.Structure):
    _fields_ = [("id", u32), ("_pad", u32), ("userdata", u64)]


class ContactEvent(C.Structure):
    _fields_ = [("id1", u32), ("id2", u32), ("userdata1", u64), ("userdata2", u64),
                ("lin_vel1", f32 * 3), ("lin_vel2", f32 * 3), ("base_offset", f32 * 3), ("normal", f32 * 3),
                ("num_points", u32), ("rel_points_on1", (f32 * 3) * 4), ("penetration", f32)]


class Ray(C.Structure):
    _fields_ = [("origin", f32 * 3), ("dir", f32 * 3), ("max_t", f32), ("ignore_id", u32), ("collidable_only", u32)]


class Hit(C.Structure):
    _fields_ = [("id", u32), ("t", f32), ("normal", f32 * 3), ("triangle", u32), ("userdata", u64), ("material", u32), ("bary", f32 * 2), ("sub_shape", u32)]


class StepStats(C.Structure):
    _fields_ = [("num_bodies", u32), ("num_active", u32), ("num_pairs", u32), ("num_manifolds", u32),
                ("num_contact_points", u32), ("num_colours", u32), ("num_colour_rounds", u32),
                ("num_overflow_constraints", u32), ("pairs_dropped", u32), ("manifolds_dropped", u32),
                ("num_activated", u32), ("num_deactivated", u32), ("layer_counts", u32 * NUM_LAYERS),
                ("num_cached_manifolds", u32), ("num_component_constraints", u32), ("num_catch_all_constraints", u32),
                ("num_deferred_vehicles", u32), ("num_wake_pairs", u32), ("reserved_", u32), ("device_bytes", u64)]


NUM_KERNEL_CLASSES = 32


class StepProfile(C.Structure):
    _fields_ = [("stage_ms", f32 * NUM_STAGES), ("total_ms", f32), ("kernel_ms", f32 * NUM_KERNEL_CLASSES),
                ("kernel_launches", u32 * NUM_KERNEL_CLASSES), ("sweep_bodies", u32), ("num_constraints", u32),
                ("num_contact_points", u32), ("num_colours", u32), ("row_layout", u32)]


class GhostRecord(C.Structure):
    _fields_ = [("pos", f32 * 3), ("rot", f32 * 4), ("lin_vel", f32 * 3), ("ang_vel", f32 * 3),
                ("shape_type", i32), ("shape", f32 * 4), ("mass", f32), ("friction", f32), ("restitution", f32),
                ("motion_type", u32), ("global_id", u64), ("userdata", u64), ("gravity_factor", f32), ("linear_damping", f32),
                ("angular_damping", f32), ("flags", u32), ("_pad", u32 * 2)]


GHOST_FLAG_LAYER_MASK, GHOST_FLAG_SENSOR, GHOST_FLAG_ALLOW_SLEEP, GHOST_FLAG_ZERO_DRAG = 0x3, 1 << 2, 1 << 3, 1 << 4


class TilesStats(C.Structure):
    _fields_ = [("exported", u32), ("sent", u32), ("received", u32), ("ghosts", u32), ("emigrated", u32), ("immigrated", u32),
                ("fast_imports", u32), ("slow_imports", u32), ("route_retries", u32), ("comm_ranks", u32), ("exchanges", u32),
                ("comm_init_ms", f32), ("last_exchange_ms", f32), ("total_exchange_ms", f32), ("rebalances", u32), ("device_creates", u32)]


class BodyCounts(C.Structure):
    _fields_ = [("num_bodies", u32), ("max_bodies", u32), ("num_static", u32), ("num_dynamic", u32), ("num_kinematic", u32),
                ("num_active_dynamic", u32), ("num_active_kinematic", u32), ("num_meshes", u32), ("num_hulls", u32), ("reserved_", u32),
                ("shape_bytes", u64)]


class Migration(C.Structure):
    _fields_ = [("userdata", u64), ("old_id", u32), ("new_id", u32), ("direction", u32), ("peer", u32)]


class ConstraintDump(C.Structure):
    """Debug/test view of one contact constraint of the last step (not part of the reference facade)."""
    _fields_ = [("a", u32), ("b", u32), ("colour", i32), ("np", i32), ("n", f32 * 3), ("lam_n", f32 * 4),
                ("lam_t1", f32 * 4), ("lam_t2", f32 * 4), ("bias", f32 * 4)]


MAX_WHEELS, MAX_GEARS = 4, 8
VEHICLE_CONTROLLER_WHEELED, VEHICLE_CONTROLLER_MOTORCYCLE = 0, 1
VEHICLE_TESTER_SPHERE, VEHICLE_TESTER_CYLINDER = 0, 1


class WheelDesc(C.Structure):
    _fields_ = [("position", f32 * 3), ("suspension_dir", f32 * 3), ("steering_axis", f32 * 3), ("wheel_up", f32 * 3),
                ("wheel_forward", f32 * 3), ("suspension_min_length", f32), ("suspension_max_length", f32),
                ("suspension_preload", f32), ("spring_frequency", f32), ("spring_damping", f32), ("radius", f32),
                ("width", f32), ("inertia", f32), ("angular_damping", f32), ("max_steer_angle", f32),
                ("max_brake_torque", f32), ("max_handbrake_torque", f32), ("longitudinal_friction", (f32 * 2) * 3),
                ("lateral_friction", (f32 * 2) * 3)]


class DifferentialDesc(C.Structure):
    _fields_ = [("left_wheel", i32), ("right_wheel", i32), ("differential_ratio", f32), ("left_right_split", f32),
                ("limited_slip_ratio", f32), ("engine_torque_ratio", f32)]


class AntiRollBarDesc(C.Structure):
    _fields_ = [("left_wheel", i32), ("right_wheel", i32), ("stiffness", f32)]


class VehicleDesc(C.Structure):
    _fields_ = [("body", u32), ("num_wheels", u32), ("wheels", WheelDesc * MAX_WHEELS), ("up", f32 * 3),
                ("forward", f32 * 3), ("cast_radius", f32), ("max_slope_angle", f32), ("engine_max_torque", f32),
                ("engine_min_rpm", f32), ("engine_max_rpm", f32), ("engine_inertia", f32),
                ("engine_angular_damping", f32), ("engine_torque_curve", (f32 * 2) * 3), ("num_gears", u32),
                ("num_reverse_gears", u32), ("gear_ratios", f32 * MAX_GEARS), ("reverse_gear_ratios", f32 * MAX_GEARS),
                ("switch_time", f32), ("clutch_release_time", f32), ("switch_latency", f32), ("shift_up_rpm", f32),
                ("shift_down_rpm", f32), ("clutch_strength", f32), ("num_differentials", u32),
                ("differentials", DifferentialDesc * 2), ("differential_limited_slip_ratio", f32),
                ("num_anti_roll_bars", u32), ("anti_roll_bars", AntiRollBarDesc * 2), ("controller_type", u32),
                ("max_lean_angle", f32), ("lean_spring_constant", f32), ("lean_spring_damping", f32),
                ("lean_spring_integration_coefficient", f32), ("lean_spring_integration_decay", f32),
                ("lean_smoothing_factor", f32), ("lean_steering_limit", u32), ("collision_tester", u32)]


class VehicleInput(C.Structure):
    _fields_ = [("forward", f32), ("right", f32), ("brake", f32), ("hand_brake", f32)]


class WheelState(C.Structure):
    _fields_ = [("suspension_length", f32), ("steer_angle", f32), ("rotation_angle", f32), ("angular_velocity", f32),
                ("has_contact", i32), ("contact_body", u32), ("contact_position", f32 * 3), ("contact_normal", f32 * 3),
                ("contact_longitudinal", f32 * 3), ("contact_lateral", f32 * 3), ("contact_point_velocity", f32 * 3),
                ("suspension_lambda", f32), ("longitudinal_lambda", f32), ("lateral_lambda", f32),
                ("longitudinal_slip", f32), ("lateral_slip", f32)]


class VehicleState(C.Structure):
    _fields_ = [("wheels", WheelState * MAX_WHEELS), ("engine_rpm", f32), ("current_gear", i32),
                ("clutch_friction", f32), ("active", i32)]


class HullInfo(C.Structure):
    _fields_ = [("hull_id", u32), ("num_vertices", u32), ("num_faces", u32), ("num_edges", u32), ("com", f32 * 3), ("rot", f32 * 4),
                ("volume", f32), ("unit_inertia", f32 * 3), ("aabb_min", f32 * 3), ("aabb_max", f32 * 3)]


class MeshInfo(C.Structure):
    _fields_ = [("mesh_id", u32), ("num_vertices", u32), ("num_triangles", u32), ("num_nodes", u32), ("aabb_min", f32 * 3), ("aabb_max", f32 * 3)]


class HeightfieldDesc(C.Structure):
    _fields_ = [("heights", C.c_void_p), ("sample_count", u32), ("offset", f32 * 3), ("spacing", f32 * 2), ("scale", f32 * 3),
                ("reserved_", u32), ("quad_materials", C.c_void_p)]


class CapsuleQuery(C.Structure):
    _fields_ = [("pos", f32 * 3), ("rot", f32 * 4), ("radius", f32), ("half_height", f32), ("max_separation", f32),
                ("ignore_id", u32), ("collidable_only", u32), ("movement", f32 * 3), ("active_edges", u32)]


QUERY_DEEPEST_ONLY = 1


class ShapeQuery(C.Structure):
    """sgp_shape_query: one overlap query of sgp_collide_shapes (a sphere, box, capsule or convex hull at a pose)."""
    _fields_ = [("pos", f32 * 3), ("rot", f32 * 4), ("shape_type", i32), ("shape", f32 * 4), ("max_separation", f32),
                ("ignore_id", u32), ("layer_mask", u32), ("flags", u32), ("movement", f32 * 3), ("active_edges", u32)]


CAST_TOLERANCE = 1.0e-4      # SGP_CAST_TOLERANCE


class ShapeCast(C.Structure):
    """sgp_shape_cast: one cast of sgp_cast_shapes (a sphere, box, capsule or convex hull translated from a pose along dir)."""
    _fields_ = [("pos", f32 * 3), ("rot", f32 * 4), ("shape_type", i32), ("shape", f32 * 4), ("dir", f32 * 3), ("max_t", f32),
                ("ignore_id", u32), ("layer_mask", u32), ("flags", u32)]


class CastHit(C.Structure):
    """sgp_cast_hit: the closest hit of one cast (id == INVALID_ID: none within max_t)."""
    _fields_ = [("id", u32), ("t", f32), ("normal", f32 * 3), ("point", f32 * 3), ("penetration", f32), ("sub_shape", u32),
                ("triangle", u32), ("material", u32), ("userdata", u64)]


CHAR_EXTENDED, CHAR_NO_SLIDE, CHAR_DISABLED = 1, 2, 4                                   # SGP_CHAR_*
GROUND_ON_GROUND, GROUND_ON_STEEP_GROUND, GROUND_NOT_SUPPORTED, GROUND_IN_AIR = 0, 1, 2, 3    # SGP_GROUND_* (CharacterBase::EGroundState)
CHAR_MAX_CONTACTS = 64


class CharacterDesc(C.Structure):
    """sgp_character_desc: CharacterVirtualSettings + ExtendedUpdateSettings of one character of a batch."""
    _fields_ = [("radius", f32), ("half_height", f32), ("shape_offset", f32 * 3), ("up", f32 * 3), ("supporting_plane", f32 * 4),
                ("max_slope_angle", f32), ("mass", f32), ("max_strength", f32), ("predictive_contact_distance", f32),
                ("character_padding", f32), ("penetration_recovery_speed", f32), ("collision_tolerance", f32),
                ("max_collision_iterations", u32), ("max_constraint_iterations", u32), ("min_time_remaining", f32),
                ("stick_to_floor_step_down", f32 * 3), ("walk_stairs_step_up", f32 * 3), ("walk_stairs_min_step_forward", f32),
                ("walk_stairs_step_forward_test", f32), ("walk_stairs_cos_angle_forward_contact", f32),
                ("walk_stairs_step_down_extra", f32 * 3)]


class CharacterInput(C.Structure):
    _fields_ = [("velocity", f32 * 3), ("ignore_id", u32), ("flags", u32)]


class CharacterState(C.Structure):
    _fields_ = [("pos", f32 * 3), ("lin_vel", f32 * 3), ("ground_state", u32), ("ground_normal", f32 * 3),
                ("ground_velocity", f32 * 3), ("ground_position", f32 * 3), ("ground_body", u32), ("ground_sub_shape", u32),
                ("overflow", u32), ("ground_userdata", u64)]


class CharacterContact(C.Structure):
    """sgp_character_contact: CharacterContactListener::OnContactAdded of one character of a batch."""
    _fields_ = [("character", u32), ("body", u32), ("sub_shape", u32), ("reserved_", u32), ("userdata", u64),
                ("point", f32 * 3), ("normal", f32 * 3)]


DRIVE_ON, DRIVE_FLY, DRIVE_GRAVITY, DRIVE_FREE_CAMERA, DRIVE_SMOOTH_STAIRS = 1, 2, 4, 8, 16    # SGP_DRIVE_*


class CharacterDrive(C.Structure):
    """sgp_character_drive: what a driven character's player asks for (PlayerPhysics' move_desired_vel, modes and constants)."""
    _fields_ = [("move_desired_vel", f32 * 3), ("move_up", f32), ("flags", u32), ("jump_speed", f32), ("max_air_speed", f32), ("eye_height", f32)]


class CharacterDriveState(C.Structure):
    """sgp_character_drive_state: what PlayerPhysics::update leaves besides the character's own state."""
    _fields_ = [("cam_pos", f32 * 3), ("campos_z_delta", f32), ("last_xy_plane_vel_rel_ground", f32 * 3), ("fraction_submerged", f32),
                ("on_ground", u32), ("jumped", u32), ("num_jumps", u32), ("pad_", u32)]


PARTICLE_DIE_ON_HIT = 1                                                  # SGP_PARTICLE_DIE_ON_HIT
PARTICLE_EV_DIED, PARTICLE_EV_FOAM, PARTICLE_EV_REPLACED = 1, 2, 4       # SGP_PARTICLE_EV_*
PARTICLES_MAX_CAPACITY = 1 << 20


class Particle(C.Structure):
    """sgp_particle: what the reference's Particle carries for the simulation (ParticleManager.h:25-60); `tag` stands for the caller's gl_ob."""
    _fields_ = [("pos", f32 * 3), ("vel", f32 * 3), ("area", f32), ("mass", f32), ("restitution", f32), ("width", f32),
                ("dwidth_dt", f32), ("opacity", f32), ("dopacity_dt", f32), ("flags", u32), ("tag", u64)]


class ParticleState(C.Structure):
    """sgp_particle_state: a live particle as sgp_particles_read reports it."""
    _fields_ = [("pos", f32 * 3), ("width", f32), ("vel", f32 * 3), ("opacity", f32), ("tag", u64), ("flags", u32), ("reserved_", u32)]


class ParticleEvent(C.Structure):
    """sgp_particle_event: DIED / FOAM / REPLACED of one particle."""
    _fields_ = [("tag", u64), ("kind", u32), ("pos", f32 * 3), ("width", f32), ("foam_width", f32)]


CRAFT_HOVERCAR, CRAFT_BOAT = 0, 1                                         # SGP_CRAFT_*
CRAFT_MAX_SPLASH_POINTS, CRAFT_MAX_EMIT, CRAFTS_MAX_CAPACITY = 8, 22, 1 << 16
CRAFT_IN_DRIVER, CRAFT_IN_BOOST = 1, 2                                    # SGP_CRAFT_IN_*
CRAFT_ST_BODY_GONE = 1                                                    # SGP_CRAFT_ST_*
CRAFT_BR = {"HOVER": 1 << 0, "UNFLIP": 1 << 1, "DRAG": 1 << 2, "LIFT_TOP": 1 << 3, "LIFT_BOTTOM": 1 << 4, "LIFT_RIGHT": 1 << 5, "LIFT_LEFT": 1 << 6,
            "THRUST": 1 << 7, "RUDDER": 1 << 8, "RIGHTING": 1 << 9, "RAY_BODY": 1 << 10, "RAY_WATER": 1 << 11, "ACTIVATE": 1 << 12, "SPLASH0": 1 << 16}      # SGP_CRAFT_BR_*
CRAFT_PK_SPRAY, CRAFT_PK_DUST, CRAFT_PK_JET, CRAFT_PK_SPLASH = 0, 1, 2, 3   # SGP_CRAFT_PK_*


class CraftDesc(C.Structure):
    """sgp_craft_desc: one hover car (HoverCarPhysicsSettings) or boat (BoatPhysicsSettings / BoatScriptSettings) of a batch."""
    _fields_ = [("kind", u32), ("body", u32), ("mass", f32), ("model_to_y_forwards_rot_1", f32 * 4), ("model_to_y_forwards_rot_2", f32 * 4),
                ("seed", u32), ("tag", u64), ("trace_origin_os", f32 * 3), ("thrust_force", f32), ("propellor_point_os", f32 * 3),
                ("propellor_sideways_offset", f32), ("rudder_deflection_force_factor", f32), ("thrust_vector_lateral_amount", f32),
                ("jet_particle_initial_width", f32), ("front_cross_sectional_area", f32), ("side_cross_sectional_area", f32),
                ("top_cross_sectional_area", f32), ("n_splash_points", u32), ("splash_points", f32 * 32), ("shape_volume", f32)]


class CraftInput(C.Structure):
    _fields_ = [("forward", f32), ("right", f32), ("up", f32), ("hand_brake", f32), ("flags", u32)]


class CraftState(C.Structure):
    """sgp_craft_state: what the last update of a craft did."""
    _fields_ = [("force", f32 * 3), ("torque", f32 * 3), ("branches", u32), ("unflip_time_remaining", f32), ("righting_time_remaining", f32),
                ("trace_origin", f32 * 3), ("trace_t", f32), ("trace_body", u32), ("n_emitted", u32), ("status", u32), ("update_index", u32),
                ("reserved_", u32)]


MOVER_PATH, MOVER_MOVETO = 0, 1                                           # SGP_MOVER_*
WAYPOINT_CURVE_IN, WAYPOINT_CURVE_OUT, WAYPOINT_STATION = 0, 1, 2         # SGP_WAYPOINT_*
MOVER_EASE_LINEAR, MOVER_EASE_SMOOTHSTEP = 0, 1                           # SGP_MOVER_EASE_*
MOVER_ORIENT_ALONG_PATH = 1
MOVER_MAX_WAYPOINTS, MOVER_MAX_SEGMENTS_PER_UPDATE, MOVERS_MAX_CAPACITY, MOVERS_MAX_PATHS = 128, 64, 1 << 16, 1 << 12
MOVER_ST = {"BODY_GONE": 1, "LEADER_GONE": 2, "OVERRUN": 4, "POS_ACTIVE": 8, "ROT_ACTIVE": 16}      # SGP_MOVER_ST_*


class PathWaypoint(C.Structure):
    """sgp_path_waypoint: PathWaypointIn of ObjectPathController."""
    _fields_ = [("pos", f32 * 3), ("type", u32), ("pause_time", f32), ("speed", f32)]


class PathSegment(C.Structure):
    """sgp_path_segment: ObjectPathController::PathWaypoint, the derived values filled by sgp_path_prepare."""
    _fields_ = [("pos", f32 * 3), ("type", u32), ("pause_time", f32), ("speed", f32), ("segment_len", f32), ("just_curve_len", f32),
                ("entry_segment_len", f32), ("curve_angle", f32), ("curve_r", f32), ("exit_segment_unit_dir", f32 * 3)]


class PathProgress(C.Structure):
    _fields_ = [("waypoint_index", u32), ("dist_along_segment", f32), ("time_along_segment", f32)]


class MoverDesc(C.Structure):
    """sgp_mover_desc: one path mover (ObjectPathController) or move-to mover (ObjectMoveToController) of a batch."""
    _fields_ = [("kind", u32), ("body", u32), ("flags", u32), ("path", u32), ("initial_time", C.c_double), ("tag", u64), ("leader", u32),
                ("follow_dist", f32), ("base_rot", f32 * 4), ("hold_pos", f32 * 3), ("hold_rot", f32 * 4), ("reserved_", u32)]


class MoverState(C.Structure):
    """sgp_mover_state: what the last update of a mover did."""
    _fields_ = [("status", u32), ("waypoint_index", u32), ("dist_along_segment", f32), ("time_along_segment", f32), ("pos", f32 * 3),
                ("rot", f32 * 4), ("dir", f32 * 3), ("pos_elapsed", f32), ("rot_elapsed", f32), ("update_index", u32)]


PROX_MAX_OBSERVERS, PROXIMITY_MAX_OBJECTS, PROXIMITY_MAX_ZONES = 32, 1 << 20, 1 << 12      # SGP_PROX_MAX_OBSERVERS, SGP_PROXIMITY_MAX_*
PROX_WANT_NEAR, PROX_WANT_ZONE = 1, 2                                     # SGP_PROX_WANT_*
PROX_OBS_POINT, PROX_OBS_BODY = 0, 1                                      # SGP_PROX_OBS_*
PROX_ST_BODY_GONE, PROX_OBS_ST_BODY_GONE = 1, 1
PROX_EV = {"NEAR": 1, "AWAY": 2, "EXITED": 3, "ENTERED": 4}               # SGP_PROX_EV_*


class ProximityObject(C.Structure):
    """sgp_proximity_object: one watched object of a proximity batch."""
    _fields_ = [("body", u32), ("radius", f32), ("flags", u32), ("reserved_", u32), ("tag", u64)]


class ProximityObserver(C.Structure):
    """sgp_proximity_observer: where an observer is -- a point of the host, or a body plus a world-space offset."""
    _fields_ = [("source", u32), ("body", u32), ("pos", f32 * 3), ("offset", f32 * 3)]


class ProximityEvent(C.Structure):
    """sgp_proximity_event: NEAR / AWAY / EXITED / ENTERED of one (object, observer) pair, or an observer-level zone record."""
    _fields_ = [("kind", u32), ("object", u32), ("observer", u32), ("zone_key", u32), ("tag", u64), ("update_index", u32), ("reserved_", u32)]


class ProximityState(C.Structure):
    _fields_ = [("status", u32), ("near_mask", u32)]


class ProximityObserverState(C.Structure):
    _fields_ = [("pos", f32 * 3), ("zone_key", u32), ("update_index", u32), ("status", u32)]


AUD_MAX_LISTENERS, AUDIBILITY_MAX_SOURCES, AUDIBILITY_MAX_PAIRS = 32, 1 << 20, 1 << 22      # SGP_AUD_MAX_LISTENERS, SGP_AUDIBILITY_MAX_*
AUD_SRC_POINT, AUD_SRC_BODY = 0, 1                                        # SGP_AUD_SRC_*
AUD_LST_POINT, AUD_LST_BODY = 0, 1                                        # SGP_AUD_LST_*
AUD_ONE_SHOT, AUD_WANT_RANGE, AUD_WANT_OCCLUSION, AUD_WANT_VOLUME = 1, 2, 4, 8
AUD_ST_BODY_GONE, AUD_LST_ST_BODY_GONE = 1, 1
AUD_PAIR_IN_RANGE, AUD_PAIR_OCCLUDED = 1, 2                               # SGP_AUD_PAIR_*
AUD_EV = {"IN_RANGE": 1, "OUT_OF_RANGE": 2, "OCCLUDED": 3, "UNOCCLUDED": 4, "VOLUME": 5}      # SGP_AUD_EV_*


class AudibilitySource(C.Structure):
    """sgp_audibility_source: one audio source of an audibility batch."""
    _fields_ = [("kind", u32), ("body", u32), ("pos", f32 * 3), ("volume", f32), ("zone_key", u32), ("flags", u32), ("tag", u64)]


class AudibilityListener(C.Structure):
    """sgp_audibility_listener: where a listener is, what its rays ignore, the parcel it stands in."""
    _fields_ = [("source", u32), ("body", u32), ("pos", f32 * 3), ("offset", f32 * 3), ("ignore_body", u32), ("zone_key", u32), ("mute_outside", u32),
                ("reserved_", u32)]


class AudibilityEvent(C.Structure):
    """sgp_audibility_event: a range, occlusion or volume transition of one (source, listener) pair."""
    _fields_ = [("kind", u32), ("source", u32), ("listener", u32), ("factor", f32), ("tag", u64), ("update_index", u32), ("reserved_", u32)]


class AudibilityState(C.Structure):
    _fields_ = [("status", u32), ("pos", f32 * 3), ("in_range_mask", u32), ("occluded_mask", u32)]


class AudibilityPairState(C.Structure):
    _fields_ = [("bits", u32), ("mute_volume_factor", f32), ("dist", f32)]


class AudibilityListenerState(C.Structure):
    _fields_ = [("pos", f32 * 3), ("zone_key", u32), ("mute_outside", u32), ("update_index", u32), ("status", u32)]


class AudibilityRamp(C.Structure):
    """sgp_audibility_ramp: the five ramp variables of AudioSource."""
    _fields_ = [("mute_change_start_time", C.c_double), ("mute_change_end_time", C.c_double), ("mute_volume_factor", f32), ("mute_vol_fac_start", f32),
                ("mute_vol_fac_end", f32), ("reserved_", u32)]


class CompoundChild(C.Structure):
    _fields_ = [("shape_type", i32), ("shape", f32 * 4), ("pos", f32 * 3), ("rot", f32 * 4)]


class QueryContact(C.Structure):
    _fields_ = [("query", u32), ("body", u32), ("point", f32 * 3), ("normal", f32 * 3), ("distance", f32),
                ("point_velocity", f32 * 3), ("motion_type", u32), ("is_sensor", u32), ("inv_mass", f32), ("sub_shape", u32),
                ("userdata", u64)]


class CheckpointInfo(C.Structure):
    """sgp_checkpoint_info: what a world checkpoint (or its blob) holds."""
    _fields_ = [("device_bytes", u64), ("host_bytes", u64), ("blob_bytes", u64), ("world_device_bytes", u64),
                ("shape_bytes_copied", u64), ("num_bodies", u32), ("high_slot", u32), ("num_cached_contacts", u32),
                ("num_vehicles", u32), ("num_meshes", u32), ("num_hulls", u32), ("num_compounds", u32), ("steps_taken", u32)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


BATCH_CHARACTERS, BATCH_PARTICLES, BATCH_CRAFTS, BATCH_MOVERS, BATCH_PROXIMITY = 1, 2, 3, 4, 5
BATCH_AUDIBILITY = 6


class BatchCheckpointInfo(C.Structure):
    """sgp_batch_checkpoint_info: what a checkpoint of a batch holds."""
    _fields_ = [("device_bytes", u64), ("host_bytes", u64), ("kind", u32), ("capacity", u32), ("high_slot", u32),
                ("num_alive", u32), ("world_steps_taken", u32), ("pad_", u32)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_ if name != "pad_"}


ABI_SIZEOF_ORDER = ["sgp_settings", "sgp_world_desc", "sgp_body_desc", "sgp_body_state", "sgp_body_event",
                    "sgp_contact_event", "sgp_ray", "sgp_hit", "sgp_step_stats", "sgp_step_profile", "sgp_ghost_record",
                    "sgp_vehicle_desc", "sgp_vehicle_input", "sgp_vehicle_state", "sgp_hull_info",
                    "sgp_capsule_query", "sgp_query_contact", "sgp_mesh_info", "sgp_heightfield_desc", "sgp_checkpoint_info"]

# structs appended to sgp_abi_sizeof after ABI_SIZEOF_ORDER was fixed (their indices follow its last one; nothing before them moves)
# (index 21 is not used and answers -1 for good: bindings that know 21 structs probe it for the end of the list)
# (likewise 24, which the bindings that know 24 structs probe)
ABI_SIZEOF_APPENDED = ["sgp_shape_query", None, "sgp_shape_cast", "sgp_cast_hit",
                       None, "sgp_character_desc", "sgp_character_input", "sgp_character_state", "sgp_character_contact",
                       None, "sgp_particle", "sgp_particle_state", "sgp_particle_event",      # (29 likewise)
                       None, "sgp_craft_desc", "sgp_craft_input", "sgp_craft_state",          # (33 likewise)
                       None, "sgp_path_waypoint", "sgp_path_segment", "sgp_path_progress", "sgp_mover_desc", "sgp_mover_state",      # (37 likewise)
                       None, "sgp_batch_checkpoint_info",      # (43 likewise)
                       None, "sgp_proximity_object", "sgp_proximity_observer", "sgp_proximity_event", "sgp_proximity_state",      # (45 likewise)
                       "sgp_proximity_observer_state",
                       None, "sgp_audibility_source", "sgp_audibility_listener", "sgp_audibility_event", "sgp_audibility_state",      # (51 likewise)
                       "sgp_audibility_pair_state", "sgp_audibility_listener_state", "sgp_audibility_ramp",
                       None, "sgp_character_drive", "sgp_character_drive_state"]      # (59 likewise)
ABI_SIZEOF_ALL = ABI_SIZEOF_ORDER + ABI_SIZEOF_APPENDED

STRUCTS = {"sgp_settings": Settings, "sgp_world_desc": WorldDesc, "sgp_body_desc": BodyDesc,
           "sgp_body_state": BodyState, "sgp_body_event": BodyEvent, "sgp_contact_event": ContactEvent,
           "sgp_ray": Ray, "sgp_hit": Hit, "sgp_step_stats": StepStats, "sgp_step_profile": StepProfile,
           "sgp_ghost_record": GhostRecord, "sgp_vehicle_desc": VehicleDesc, "sgp_vehicle_input": VehicleInput,
           "sgp_vehicle_state": VehicleState, "sgp_hull_info": HullInfo, "sgp_capsule_query": CapsuleQuery,
           "sgp_query_contact": QueryContact, "sgp_mesh_info": MeshInfo, "sgp_heightfield_desc": HeightfieldDesc,
           "sgp_checkpoint_info": CheckpointInfo, "sgp_shape_query": ShapeQuery, "sgp_shape_cast": ShapeCast,
           "sgp_cast_hit": CastHit, "sgp_character_desc": CharacterDesc, "sgp_character_input": CharacterInput,
           "sgp_character_state": CharacterState, "sgp_character_contact": CharacterContact,
           "sgp_particle": Particle, "sgp_particle_state": ParticleState, "sgp_particle_event": ParticleEvent,
           "sgp_craft_desc": CraftDesc, "sgp_craft_input": CraftInput, "sgp_craft_state": CraftState,
           "sgp_path_waypoint": PathWaypoint, "sgp_path_segment": PathSegment, "sgp_path_progress": PathProgress,
           "sgp_mover_desc": MoverDesc, "sgp_mover_state": MoverState, "sgp_batch_checkpoint_info": BatchCheckpointInfo,
           "sgp_proximity_object": ProximityObject, "sgp_proximity_observer": ProximityObserver, "sgp_proximity_event": ProximityEvent,
           "sgp_proximity_state": ProximityState, "sgp_proximity_observer_state": ProximityObserverState,
           "sgp_audibility_source": AudibilitySource, "sgp_audibility_listener": AudibilityListener, "sgp_audibility_event": AudibilityEvent,
           "sgp_audibility_state": AudibilityState, "sgp_audibility_pair_state": AudibilityPairState,
           "sgp_audibility_listener_state": AudibilityListenerState, "sgp_audibility_ramp": AudibilityRamp,
           "sgp_character_drive": CharacterDrive, "sgp_character_drive_state": CharacterDriveState}

body_desc_dtype = np.dtype(BodyDesc)
body_state_dtype = np.dtype(BodyState)
body_pose_dtype = np.dtype(BodyPose)
ghost_dtype = np.dtype(GhostRecord)
contact_event_dtype = np.dtype(ContactEvent)
body_event_dtype = np.dtype(BodyEvent)
constraint_dump_dtype = np.dtype(ConstraintDump)
ray_dtype = np.dtype(Ray)
hit_dtype = np.dtype(Hit)
pose_vel_dtype = np.dtype(PoseVel)
vehicle_input_dtype = np.dtype(VehicleInput)
vehicle_state_dtype = np.dtype(VehicleState)
capsule_query_dtype = np.dtype(CapsuleQuery)
query_contact_dtype = np.dtype(QueryContact)
shape_query_dtype = np.dtype(ShapeQuery)
shape_cast_dtype = np.dtype(ShapeCast)
cast_hit_dtype = np.dtype(CastHit)
character_input_dtype = np.dtype(CharacterInput)
character_state_dtype = np.dtype(CharacterState)
character_contact_dtype = np.dtype(CharacterContact)
character_drive_dtype = np.dtype(CharacterDrive)
character_drive_state_dtype = np.dtype(CharacterDriveState)
particle_dtype = np.dtype(Particle)
particle_state_dtype = np.dtype(ParticleState)
particle_event_dtype = np.dtype(ParticleEvent)
craft_desc_dtype = np.dtype(CraftDesc)
craft_input_dtype = np.dtype(CraftInput)
craft_state_dtype = np.dtype(CraftState)
path_waypoint_dtype = np.dtype(PathWaypoint)
path_segment_dtype = np.dtype(PathSegment)
mover_state_dtype = np.dtype(MoverState)
proximity_object_dtype = np.dtype(ProximityObject)
proximity_event_dtype = np.dtype(ProximityEvent)
proximity_state_dtype = np.dtype(ProximityState)
proximity_observer_state_dtype = np.dtype(ProximityObserverState)
audibility_source_dtype = np.dtype(AudibilitySource)
audibility_event_dtype = np.dtype(AudibilityEvent)
audibility_state_dtype = np.dtype(AudibilityState)
audibility_pair_state_dtype = np.dtype(AudibilityPairState)
audibility_listener_state_dtype = np.dtype(AudibilityListenerState)
compound_child_dtype = np.dtype(CompoundChild)
migration_dtype = np.dtype(Migration)

P = C.POINTER
vp = C.c_void_p

# name (without prefix) -> (restype, argtypes); world handle is void*
PROTOTYPES = {
    "init": (C.c_int, []),
    "abi_version": (C.c_int, []),
    "last_error": (C.c_char_p, []),
    "default_settings": (None, [P(Settings)]),
    "default_world_desc": (None, [P(WorldDesc)]),
    "default_body_desc": (None, [P(BodyDesc)]),
    "world_create": (C.c_int, [P(WorldDesc), P(vp)]),
    "world_destroy": (C.c_int, [vp]),
    "body_add": (C.c_int, [vp, P(BodyDesc), P(u32)]),
    "body_add_batch": (C.c_int, [vp, vp, u32, vp]),
    "body_add_compound": (C.c_int, [vp, P(BodyDesc), vp, u32, P(u32)]),
    "body_compound_size": (C.c_int, [vp, u32, P(u32)]),
    "body_remove": (C.c_int, [vp, u32]),
    "body_activate": (C.c_int, [vp, u32]),
    "body_set_layer": (C.c_int, [vp, u32, i32]),
    "body_get_volume": (C.c_int, [vp, u32, P(f32)]),
    "body_get_userdata": (C.c_int, [vp, u32, P(u64)]),
    "body_set_pose_vel": (C.c_int, [vp, u32, P(f32), P(f32), P(f32), P(f32)]),
    "body_set_pose_shape": (C.c_int, [vp, u32, P(f32), P(f32), P(f32)]),
    "body_set_pose_vel_batch": (C.c_int, [vp, vp, vp, u32]),
    "physics_update_encode": (C.c_int, [u64, P(BodyState), C.c_double, vp]),
    "physics_update_decode": (C.c_int, [vp, P(u64), P(PoseVel), P(C.c_double)]),
    "snapshot_queue_create": (C.c_int, [P(vp)]),
    "snapshot_queue_destroy": (C.c_int, [vp]),
    "snapshot_queue_push_wire": (C.c_int, [vp, vp, C.c_double]),
    "snapshot_queue_push": (C.c_int, [vp, u64, P(PoseVel), C.c_double, C.c_double]),
    "snapshot_queue_ownership": (C.c_int, [vp, u64, C.c_double, C.c_double, C.c_int]),
    "snapshot_queue_poll": (C.c_int, [vp, C.c_double, C.c_double, vp, vp, u32, P(u32)]),
    "snapshot_queue_expire": (C.c_int, [vp, C.c_double, C.c_double, P(u32)]),
    "snapshot_queue_peek": (C.c_int, [vp, u64, P(u32), P(u32), P(C.c_double)]),
    "body_set_pos": (C.c_int, [vp, u32, P(f32)]),
    "body_set_vel": (C.c_int, [vp, u32, P(f32), P(f32)]),
    "body_move_kinematic": (C.c_int, [vp, u32, P(f32), P(f32), f32]),
    "body_add_force": (C.c_int, [vp, u32, P(f32)]),
    "body_add_force_at": (C.c_int, [vp, u32, P(f32), P(f32)]),
    "body_add_torque": (C.c_int, [vp, u32, P(f32)]),
    "body_get_state": (C.c_int, [vp, vp, u32, vp]),
    "world_read_states": (C.c_int, [vp, u32, u32, vp]),
    "world_read_active": (C.c_int, [vp, vp, u32, P(u32)]),
    "world_read_active_view": (C.c_int, [vp, P(vp), P(u32)]),
    "world_read_active_poses_view": (C.c_int, [vp, P(vp), P(u32)]),
    "world_set_water": (C.c_int, [vp, C.c_int, f32]),
    "world_set_contact_events": (C.c_int, [vp, C.c_int]),
    "world_step": (C.c_int, [vp, f32]),
    "world_step_n": (C.c_int, [vp, f32, u32]),
    "world_step_profiled": (C.c_int, [vp, f32, P(StepProfile)]),
    "world_stats": (C.c_int, [vp, P(StepStats)]),
    "world_launch_counts": (C.c_int, [vp, P(u32), P(u32), P(u32)]),
    "kernel_class_name": (C.c_char_p, [C.c_int]),
    "abi_sizeof": (C.c_int, [C.c_int]),
    "world_drain_events": (C.c_int, [vp, C.c_int, vp, u32, P(u32)]),
    "world_event_counts": (C.c_int, [vp, P(u32)]),
    "world_num_bodies": (C.c_int, [vp, P(u32)]),
    "world_body_counts": (C.c_int, [vp, P(BodyCounts)]),
    "raycast": (C.c_int, [vp, vp, u32, vp]),
    "raycast_any": (C.c_int, [vp, vp, u32, vp]),      # rays, n, one byte per ray out (1 = hits something within max_t)
    "collide_capsules": (C.c_int, [vp, vp, u32, vp, u32, P(u32)]),
    "spherecast": (C.c_int, [vp, vp, vp, u32, vp]),
    "collide_shapes": (C.c_int, [vp, vp, u32, vp, u32, P(u32)]),
    "cast_shapes": (C.c_int, [vp, vp, u32, vp]),
    "cast_shapes_counters": (C.c_int, [vp, P(u32)]),
    # batched virtual characters (handle: void*)
    "default_character_desc": (None, [P(CharacterDesc)]),
    "characters_create": (C.c_int, [vp, u32, P(vp)]),
    "characters_destroy": (C.c_int, [vp]),
    "character_add": (C.c_int, [vp, P(CharacterDesc), P(f32), P(u32)]),
    "character_remove": (C.c_int, [vp, u32]),
    "characters_set_pose": (C.c_int, [vp, vp, vp, u32]),
    "characters_set_shape": (C.c_int, [vp, u32, f32, f32, P(f32)]),
    "characters_set_inputs": (C.c_int, [vp, u32, u32, vp]),
    "characters_update": (C.c_int, [vp, f32]),
    "characters_get_states": (C.c_int, [vp, u32, u32, vp]),
    "characters_drain_contacts": (C.c_int, [vp, vp, u32, P(u32)]),
    "default_character_drive": (None, [P(CharacterDrive)]),
    "characters_set_drive": (C.c_int, [vp, u32, u32, vp]),
    "characters_jump": (C.c_int, [vp, vp, u32, C.c_double]),
    "characters_update_at": (C.c_int, [vp, f32, C.c_double]),
    "characters_get_drive_states": (C.c_int, [vp, u32, u32, vp]),
    # batched point particles (handle: void*)
    "default_particle": (None, [P(Particle)]),
    "particles_create": (C.c_int, [vp, u32, u32, P(vp)]),
    "particles_destroy": (C.c_int, [vp]),
    "particles_add": (C.c_int, [vp, vp, u32]),
    "particles_update": (C.c_int, [vp, f32]),
    "particles_read": (C.c_int, [vp, vp, u32, P(u32)]),
    "particles_drain_events": (C.c_int, [vp, vp, u32, P(u32), P(u32)]),
    "particles_clear": (C.c_int, [vp]),
    # batched hover cars and boats (handle: void*)
    "default_craft_desc": (None, [u32, P(CraftDesc)]),
    "crafts_create": (C.c_int, [vp, u32, P(vp)]),
    "crafts_destroy": (C.c_int, [vp]),
    "craft_add": (C.c_int, [vp, P(CraftDesc), P(u32)]),
    "craft_remove": (C.c_int, [vp, u32]),
    "crafts_set_inputs": (C.c_int, [vp, u32, u32, vp]),
    "crafts_start_righting": (C.c_int, [vp, vp, u32]),
    "crafts_attach_particles": (C.c_int, [vp, vp]),
    "crafts_update": (C.c_int, [vp, f32]),
    "crafts_get_states": (C.c_int, [vp, u32, u32, vp]),
    "path_prepare": (C.c_int, [vp, u32, vp, P(C.c_double)]),
    "path_advance": (C.c_int, [vp, u32, P(PathProgress), f32, P(u32)]),
    "movers_create": (C.c_int, [vp, u32, u32, P(vp)]),
    "movers_destroy": (C.c_int, [vp]),
    "movers_path_add": (C.c_int, [vp, vp, u32, P(u32)]),
    "movers_path_remove": (C.c_int, [vp, u32]),
    "movers_path_get": (C.c_int, [vp, u32, vp, u32, P(u32)]),
    "mover_add": (C.c_int, [vp, P(MoverDesc), P(u32)]),
    "mover_remove": (C.c_int, [vp, u32]),
    "movers_set_position_track": (C.c_int, [vp, u32, P(f32), P(f32), f32, u32, f32]),
    "movers_set_rotation_track": (C.c_int, [vp, u32, P(f32), P(f32), f32, u32, f32]),
    "movers_update": (C.c_int, [vp, f32]),
    "movers_get_states": (C.c_int, [vp, u32, u32, vp]),
    "world_export_boundary": (C.c_int, [vp, P(f32), P(f32), f32, vp, u32, P(u32)]),
    "world_import_ghosts": (C.c_int, [vp, vp, u32]),
    "tiles_route": (C.c_int, [vp, u32, u32, vp, u32, f32, vp, u32, vp, vp, u32, P(u32)]),
    "tiles_split": (C.c_int, [vp, u32, vp, vp, vp, P(u32), vp, P(u32)]),
    "tiles_unique_id": (C.c_int, [vp]),
    "tiles_create": (C.c_int, [vp, u32, u32, vp, f32, f32, vp, P(vp)]),
    "tiles_destroy": (C.c_int, [vp]),
    "tiles_exchange": (C.c_int, [vp]),
    "tiles_exchange_group": (C.c_int, [vp, u32]),
    "tiles_get_stats": (C.c_int, [vp, P(TilesStats)]),
    "tiles_rebalance": (C.c_int, [vp, u32, u32, u32, C.c_int]),
    "tiles_rebalance_group": (C.c_int, [vp, u32, u32, u32, u32, C.c_int]),
    "tiles_get_boxes": (C.c_int, [vp, vp]),
    "tiles_drain_migrations": (C.c_int, [vp, vp, u32, P(u32)]),
    "world_device_array": (C.c_int, [vp, C.c_int, P(vp), P(u32)]),
    "world_stream": (C.c_int, [vp, P(vp)]),
    "mesh_create": (C.c_int, [vp, vp, u32, vp, u32, P(MeshInfo)]),
    "mesh_create_with_materials": (C.c_int, [vp, vp, u32, vp, u32, vp, P(MeshInfo)]),
    "mesh_destroy": (C.c_int, [vp, u32]),
    "heightfield_create": (C.c_int, [vp, P(HeightfieldDesc), P(MeshInfo)]),
    "mesh_edge_flags": (C.c_int, [vp, u32, vp, u32]),
    "hull_destroy": (C.c_int, [vp, u32]),
    "hull_create": (C.c_int, [vp, vp, u32, P(HullInfo)]),
    "hull_create_com": (C.c_int, [vp, vp, u32, P(f32), P(HullInfo)]),
    "default_vehicle_desc": (None, [P(VehicleDesc)]),
    "vehicle_create": (C.c_int, [vp, P(VehicleDesc), P(u32)]),
    "vehicle_destroy": (C.c_int, [vp, u32]),
    "vehicle_set_input": (C.c_int, [vp, u32, P(VehicleInput)]),
    "vehicle_set_inputs": (C.c_int, [vp, u32, u32, vp]),
    "vehicle_get_state": (C.c_int, [vp, u32, P(VehicleState)]),
    "vehicle_get_states": (C.c_int, [vp, u32, u32, vp]),
    "vehicle_reset_drivetrain": (C.c_int, [vp, u32, f32, f32]),
    "vehicle_enable_lean_controller": (C.c_int, [vp, u32, C.c_int]),
    # world checkpoints
    "world_checkpoint": (C.c_int, [vp, P(vp)]),
    "world_rollback": (C.c_int, [vp, vp]),
    "checkpoint_destroy": (C.c_int, [vp]),
    "checkpoint_get_info": (C.c_int, [vp, P(CheckpointInfo)]),
    "checkpoint_write": (C.c_int, [vp, vp, u64, P(u64)]),
    "world_restore": (C.c_int, [vp, vp, u64]),
    "checkpoint_blob_info": (C.c_int, [vp, u64, P(CheckpointInfo)]),
    # batch checkpoints
    "characters_checkpoint": (C.c_int, [vp, P(vp)]),
    "characters_rollback": (C.c_int, [vp, vp]),
    "particles_checkpoint": (C.c_int, [vp, P(vp)]),
    "particles_rollback": (C.c_int, [vp, vp]),
    "crafts_checkpoint": (C.c_int, [vp, P(vp)]),
    "crafts_rollback": (C.c_int, [vp, vp]),
    "proximity_create": (C.c_int, [vp, u32, u32, u32, P(vp)]),
    "proximity_destroy": (C.c_int, [vp]),
    "proximity_add": (C.c_int, [vp, vp, u32, vp]),
    "proximity_remove": (C.c_int, [vp, u32]),
    "proximity_set_flags": (C.c_int, [vp, u32, u32]),
    "proximity_set_observer": (C.c_int, [vp, u32, P(ProximityObserver)]),
    "proximity_set_points": (C.c_int, [vp, u32, u32, vp]),
    "proximity_remove_observer": (C.c_int, [vp, u32]),
    "proximity_zone_add": (C.c_int, [vp, P(f32), P(f32), u32, P(u32)]),
    "proximity_zone_remove": (C.c_int, [vp, u32]),
    "proximity_update": (C.c_int, [vp]),
    "proximity_drain_events": (C.c_int, [vp, vp, u32, P(u32), P(u32)]),
    "proximity_get_states": (C.c_int, [vp, u32, u32, vp]),
    "proximity_get_observers": (C.c_int, [vp, u32, u32, vp]),
    "proximity_checkpoint": (C.c_int, [vp, P(vp)]),
    "proximity_rollback": (C.c_int, [vp, vp]),
    "proximity_test_point": (C.c_int, [P(f32), P(f32), P(f32), f32, P(u32), P(f32)]),
    "proximity_pick_zone": (C.c_int, [vp, vp, vp, vp, u32, u32, P(f32), P(u32)]),
    "audibility_create": (C.c_int, [vp, u32, u32, u32, P(vp)]),
    "audibility_destroy": (C.c_int, [vp]),
    "audibility_add": (C.c_int, [vp, vp, u32, vp]),
    "audibility_remove": (C.c_int, [vp, u32]),
    "audibility_set_points": (C.c_int, [vp, u32, u32, vp]),
    "audibility_set_volume": (C.c_int, [vp, u32, f32]),
    "audibility_set_flags": (C.c_int, [vp, u32, u32]),
    "audibility_set_listener": (C.c_int, [vp, u32, P(AudibilityListener)]),
    "audibility_remove_listener": (C.c_int, [vp, u32]),
    "audibility_set_listener_points": (C.c_int, [vp, u32, u32, vp]),
    "audibility_set_listener_zone": (C.c_int, [vp, u32, u32, u32]),
    "audibility_set_transition": (C.c_int, [vp, C.c_double]),
    "audibility_attach_proximity": (C.c_int, [vp, vp]),
    "audibility_set_muting_keys": (C.c_int, [vp, vp, u32]),
    "audibility_update": (C.c_int, [vp, C.c_double]),
    "audibility_drain_events": (C.c_int, [vp, vp, u32, P(u32), P(u32)]),
    "audibility_get_states": (C.c_int, [vp, u32, u32, vp]),
    "audibility_get_pair_states": (C.c_int, [vp, u32, u32, vp]),
    "audibility_get_listeners": (C.c_int, [vp, u32, u32, vp]),
    "audibility_checkpoint": (C.c_int, [vp, P(vp)]),
    "audibility_rollback": (C.c_int, [vp, vp]),
    "audibility_pair_ray": (C.c_int, [P(f32), P(f32), f32, u32, P(u32), P(u32), P(f32), P(f32), P(f32)]),
    "audibility_ramp_step": (C.c_int, [P(AudibilityRamp), u32, C.c_double, C.c_double, P(u32)]),
    "movers_checkpoint": (C.c_int, [vp, P(vp)]),
    "movers_rollback": (C.c_int, [vp, vp]),
    "batch_checkpoint_destroy": (C.c_int, [vp]),
    "batch_checkpoint_get_info": (C.c_int, [vp, P(BatchCheckpointInfo)]),
    # test/debug helper, not a facade entry point
    "world_dump_constraints": (C.c_int, [vp, vp, u32, P(u32)]),
}


def bind(lib, prefix, names=None):
    """Attach argtypes/restype for every prototype the library exports under `prefix`. Returns the bound names."""
    bound = []
    for name, (res, args) in PROTOTYPES.items():
        if names is not None and name not in names:
            continue
        fn = getattr(lib, prefix + name, None)
        if fn is None:
            continue
        fn.restype = res
        fn.argtypes = args
        bound.append(name)
    return bound


def blob_info(blob, lib=None, prefix="sgp_"):
    """sgp_checkpoint_blob_info: validates a checkpoint blob and returns its counts as a dict.  Host only (no device needed)."""
    if lib is None:
        from . import lib as _l
        lib = _l.load()
    buf = bytes(blob)
    info = CheckpointInfo()
    fn = getattr(lib, prefix + "checkpoint_blob_info")
    fn.restype, fn.argtypes = PROTOTYPES["checkpoint_blob_info"]
    rc = fn(C.cast(C.c_char_p(buf), vp), len(buf), C.byref(info))
    if rc != OK:
        from .world import SgpError
        msg = getattr(lib, prefix + "last_error")
        msg.restype = C.c_char_p
        raise SgpError(f"{prefix}checkpoint_blob_info failed: rc={rc} {(msg() or b'').decode()}")
    return info.as_dict()
