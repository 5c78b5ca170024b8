/*
 * sgp.h -- C ABI of the MI355X-native rigid-body stepper that sits behind Substrata's
 *          PhysicsWorld / PhysicsObject facade.
 *
 * Every entry point replaces one piece of the reference's physics facade, which today forwards to
 * JoltPhysics v5.3.0 (an un-vendored dependency).  Citations are relative to /root/reference.
 * There is no FFI seam in the reference: the boundary is the C++ class `PhysicsWorld`
 * (gui_client/PhysicsWorld.h:98-218).  This header is what a thin `PhysicsWorld.cpp` binds instead
 * of `#include <Jolt/...>`; INTEGRATION.md shows that binding.
 *
 * Conventions
 *   - every function returns an int status: SGP_OK (0) or a negative SGP_ERR_* code; nothing throws;
 *   - plain pointers and sizes only; all buffers are caller-owned host memory unless a parameter is
 *     documented as a device pointer;
 *   - one world per handle; calls on one world are externally synchronised (the reference calls the
 *     facade from the main thread only, PhysicsWorld.h:135 / GUIClient.cpp:6365-6515);
 *   - z is up, gravity defaults to (0,0,-9.81)                       (PhysicsWorld.cpp:520);
 *   - quaternions are (x,y,z,w), same memory order as Quatf / JPH::Quat (JoltUtils.h:48-56);
 *   - all arithmetic is fp32 (Jolt is built single precision; dt arrives as double and is narrowed,
 *     PhysicsWorld.cpp:1363).
 *
 * There is NO CPU fallback: every function that needs the device returns SGP_ERR_NO_DEVICE when no
 * gfx950 GPU is usable.
 */
#ifndef SGP_H
#define SGP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGP_ABI_VERSION 1

/* ---- status codes ---------------------------------------------------------------------------- */
#define SGP_OK                 0
#define SGP_ERR_INVALID       -1   /* bad argument / NULL handle                                   */
#define SGP_ERR_NO_DEVICE     -2   /* no usable HIP device (never falls back to the CPU)            */
#define SGP_ERR_CAPACITY      -3   /* max_bodies exceeded (cf. cMaxBodies, PhysicsWorld.cpp:492)    */
#define SGP_ERR_HIP           -4   /* a HIP runtime call failed; see sgp_last_error()               */
#define SGP_ERR_BAD_ID        -5   /* body id is not live                                           */
#define SGP_ERR_REJECTED      -6   /* addObject's silent rejections (PhysicsWorld.cpp:1178-1189)    */
#define SGP_ERR_PEER          -7   /* sgp_tiles_exchange: ANOTHER rank reported a failure in this exchange; every rank returns (nobody is left waiting) */

/* ---- enums (values are ABI) ------------------------------------------------------------------ */
/* Motion type: JPH::EMotionType as chosen at PhysicsWorld.cpp:1209-1217. */
#define SGP_MOTION_STATIC      0
#define SGP_MOTION_KINEMATIC   1
#define SGP_MOTION_DYNAMIC     2

/* Object layers: namespace Layers, PhysicsWorld.h:67-74; collide matrix PhysicsWorld.cpp:151-189. */
#define SGP_LAYER_NON_MOVING                 0
#define SGP_LAYER_MOVING                     1
#define SGP_LAYER_NON_MOVING_NON_COLLIDABLE  2
#define SGP_LAYER_MOVING_NON_COLLIDABLE      3
#define SGP_NUM_LAYERS                       4

/* Shapes the stepper collides natively.  Sizes are FINAL (scale already applied by the caller):
 *   SPHERE : p[0] = radius                      (unit sphere r=0.5 * scale.x, PhysicsWorld.cpp:1221-1227)
 *   BOX    : p[0..2] = half extents             (unit cube half 0.5 * scale,  PhysicsWorld.cpp:1249-1255;
 *                                                ground quad (w/2,w/2,0.5),   PhysicsWorld.cpp:1123)
 *   CAPSULE: p[0] = radius, p[1] = half height of the cylinder part, axis = local z
 *                                               (player capsule, PlayerPhysics.cpp:31-32,74)            */
#define SGP_SHAPE_SPHERE   0
#define SGP_SHAPE_BOX      1
#define SGP_SHAPE_CAPSULE  2
#define SGP_SHAPE_MESH     4   /* static triangle mesh created with sgp_mesh_create; shape[0] = (float) mesh id; static and kinematic bodies (JPH::MeshShape has no mass properties; a scripted object is a kinematic mesh body moved with sgp_body_move_kinematic).
                                  A mesh body occupies three consecutive body ids (the id returned + two internal aliases that carry
                                  the second and third contact manifold of a body touching the mesh from several sides)             */
#define SGP_SHAPE_HULL     3   /* convex hull created with sgp_hull_create; shape[0] = (float) hull id, body frame = the hull's
                                  centre-of-mass / principal-axes frame (see sgp_hull_info)                                  */

#define SGP_INVALID_ID 0xFFFFFFFFu   /* JPH::BodyID() default = invalid (PhysicsObject.h:106)        */

/* ---- settings: Jolt v5.3.0 PhysicsSettings defaults (Substrata never overrides them) ----------- */
typedef struct sgp_settings {
	int32_t num_velocity_steps;              /* 10   */
	int32_t num_position_steps;              /* 2    */
	float   baumgarte;                       /* 0.2  */
	float   penetration_slop;                /* 0.02 */
	float   speculative_contact_distance;    /* 0.02 */
	float   min_velocity_for_restitution;    /* 1.0  */
	float   max_penetration_distance;        /* 0.2  */
	float   time_before_sleep;               /* 0.5  */
	float   point_velocity_sleep_threshold;  /* 0.03 */
	float   contact_point_preserve_lambda_max_dist_sq; /* 0.01^2 */
	float   max_linear_velocity;             /* 500  */
	float   max_angular_velocity;            /* 0.25*pi*60 */
	int32_t allow_sleeping;                  /* 1    */
	int32_t warm_start;                      /* 1    */
	/* the body-pair contact cache: a pair whose relative pose moved less than this since its manifold was last computed reuses the manifold */
	int32_t use_body_pair_contact_cache;                 /* 1                  */
	float   body_pair_cache_max_delta_position_sq;       /* 0.001^2            */
	float   body_pair_cache_cos_max_delta_rotation_div2; /* cos(2 deg / 2)     */
} sgp_settings;

typedef struct sgp_world_desc {
	uint32_t max_bodies;        /* capacity; reference: 65536 (PhysicsWorld.cpp:492)                 */
	uint32_t max_body_pairs;    /* 0 = 16*max_bodies+1024; reference: 65536 in flight (:501)          */
	uint32_t max_manifolds;     /* 0 = 8*max_bodies+1024;  reference: 10240 constraints (:506)        */
	int32_t  device;            /* HIP device ordinal                                                 */
	float    gravity[3];        /* (0,0,-9.81)                                                        */
	float    large_body_radius; /* bodies with bounding radius above this skip the hashed grid; 0 = 4 m */
	sgp_settings settings;
} sgp_world_desc;

/* One body, as PhysicsWorld::addObject builds it (PhysicsWorld.cpp:1169-1311). */
typedef struct sgp_body_desc {
	float    pos[3];
	float    rot[4];            /* x,y,z,w */
	float    lin_vel[3];
	float    ang_vel[3];
	int32_t  shape_type;        /* SGP_SHAPE_* */
	float    shape[4];          /* see SGP_SHAPE_* */
	int32_t  motion_type;       /* SGP_MOTION_* */
	int32_t  layer;             /* SGP_LAYER_* */
	float    mass;              /* clamped to >= 0.001 (PhysicsWorld.cpp:1238); inertia from shape+mass */
	float    friction;          /* clamped to [0,1] (:1236) */
	float    restitution;       /* clamped to [0,1] (:1237) */
	float    gravity_factor;    /* Jolt default 1 */
	float    linear_damping;    /* Jolt default 0.05 */
	float    angular_damping;   /* Jolt default 0.05 */
	int32_t  is_sensor;         /* mIsSensor (:1235) */
	int32_t  allow_sleeping;    /* Jolt default 1 */
	int32_t  activate;          /* reference adds with EActivation::DontActivate, then activateObject() */
	int32_t  use_zero_linear_drag; /* PhysicsObject::use_zero_linear_drag (buoyancy, PhysicsWorld.cpp:1405) */
	uint64_t userdata;          /* mUserData = (uint64)PhysicsObject* (:1241) */
} sgp_body_desc;

/* Read-back record for one body (what GUIClient.cpp:6581-6690 pulls per active object). */
typedef struct sgp_body_state {
	float    pos[3];
	float    rot[4];
	float    lin_vel[3];
	float    ang_vel[3];
	uint32_t active;            /* 1 = awake */
	uint32_t underwater;        /* PhysicsObject::underwater */
	float    submerged_volume;  /* PhysicsObject::last_submerged_volume */
	uint32_t id;
} sgp_body_state;

/* Event kinds for sgp_world_drain_events. */
#define SGP_EVENT_ACTIVATED         0  /* OnBodyActivated   (PhysicsWorld.cpp:1448-1467)  payload: sgp_body_event    */
#define SGP_EVENT_DEACTIVATED       1  /* OnBodyDeactivated (PhysicsWorld.cpp:1471-1486)  payload: sgp_body_event    */
#define SGP_EVENT_ENTERED_WATER     2  /* physicsObjectEnteredWater (:1416-1420)          payload: sgp_body_event    */
#define SGP_EVENT_CONTACT_ADDED     3  /* OnContactAdded     (:1499-1503)                 payload: sgp_contact_event */
#define SGP_EVENT_CONTACT_PERSISTED 4  /* OnContactPersisted (:1516-1520)                 payload: sgp_contact_event */

typedef struct sgp_body_event {
	uint32_t id;
	uint32_t _pad;
	uint64_t userdata;
} sgp_body_event;

/* What GUIClient::contactAdded/Persisted read from JPH::Body / JPH::ContactManifold
 * (GUIClient.cpp:10588-10632): both linear velocities, mBaseOffset, mRelativeContactPointsOn1. */
typedef struct sgp_contact_event {
	uint32_t id1, id2;              /* id1 < id2 */
	uint64_t userdata1, userdata2;
	float    lin_vel1[3], lin_vel2[3];
	float    base_offset[3];        /* = first contact point on body 1 (world) */
	float    normal[3];             /* from body 1 to body 2 */
	uint32_t num_points;            /* 1..4 */
	float    rel_points_on1[4][3];  /* relative to base_offset */
	float    penetration;           /* max over points, > 0 if overlapping */
} sgp_contact_event;

typedef struct sgp_ray {
	float    origin[3];
	float    dir[3];           /* unit */
	float    max_t;
	uint32_t ignore_id;        /* JPH::BodyID ignore_body_id (PhysicsWorld.h:178) */
	uint32_t collidable_only;  /* traceRayAgainstCollidableObs (PhysicsWorld.cpp:1711-1715) */
} sgp_ray;

typedef struct sgp_hit {
	uint32_t id;               /* SGP_INVALID_ID if no hit */
	float    t;                /* RayTraceResult::hit_t */
	float    normal[3];        /* RayTraceResult::hit_normal_ws */
	uint32_t triangle;         /* mesh hits (ray casts): index of the triangle in the caller's order; SGP_INVALID_ID otherwise            */
	uint64_t userdata;         /* -> RayTraceResult::hit_object */
	uint32_t material;         /* mesh hits: the triangle's user data = material index, MeshShape::GetTriangleUserData
	                              (PhysicsWorld.cpp:1700-1704 -> RayTraceResult::hit_mat_index); 0 otherwise                               */
	float    bary[2];          /* mesh hits: barycentric coordinates (u, v) of the hit, point = (1 - u - v) a + u b + v c; 0 otherwise.
	                              (The reference leaves RayTraceResult::coords at 0, :1693; the facade does the same.)                     */
	uint32_t sub_shape;        /* compound bodies (sgp_body_add_compound): index of the child that was hit, `id` is the compound's id; 0 otherwise */
} sgp_hit;

/* Counters of the last step (getDiagnostics, PhysicsWorld.cpp:1578-1604, plus stage sizes). */
typedef struct sgp_step_stats {
	uint32_t num_bodies;
	uint32_t num_active;
	uint32_t num_pairs;
	uint32_t num_manifolds;
	uint32_t num_contact_points;
	uint32_t num_colours;
	uint32_t num_colour_rounds;
	uint32_t num_overflow_constraints;
	uint32_t pairs_dropped;
	uint32_t manifolds_dropped;
	uint32_t num_activated;      /* activation / deactivation events raised since the end of the previous step */
	uint32_t num_deactivated;
	uint32_t layer_counts[SGP_NUM_LAYERS];
	uint32_t num_cached_manifolds;       /* manifolds taken from the body-pair contact cache instead of a collision test */
	uint32_t num_component_constraints;  /* constraints of the high colours, solved component by component in one launch per pass (device launch plan; 0 on the oracle) */
	uint32_t num_catch_all_constraints;  /* ... of them in components too large for a workgroup (solved serially; the plan then takes fewer colours) */
	uint32_t num_deferred_vehicles;      /* vehicles that shared a movable body (a dynamic body under a wheel, a chassis a wheel stands on) with a vehicle of lower index this step: their rows are solved after the others', in index order */
	uint32_t num_wake_pairs;             /* in-step activation: pairs of the bodies this step woke with what was not awake when it began (part of num_pairs) */
	uint32_t reserved_;                  /* always 0 (keeps device_bytes at its offset) */
	uint64_t device_bytes;
} sgp_step_stats;

/* Per-stage device time of the last profiled step, measured with HIP events on the world's stream. */
#define SGP_STAGE_APPLY_FORCES   0
#define SGP_STAGE_BROADPHASE     1
#define SGP_STAGE_NARROWPHASE    2
#define SGP_STAGE_SETUP          3   /* islands, colouring, constraint setup + cache match */
#define SGP_STAGE_SOLVE_VELOCITY 4
#define SGP_STAGE_INTEGRATE      5   /* the body-array sweep (pose integrate + AABB)  */
#define SGP_STAGE_SOLVE_POSITION 6
#define SGP_STAGE_FINALIZE       7   /* AABB refresh, sleep test, islands sleep, buoyancy, events */
#define SGP_NUM_STAGES           8

#define SGP_NUM_KERNEL_CLASSES 32
typedef struct sgp_step_profile {
	float    stage_ms[SGP_NUM_STAGES];
	float    total_ms;              /* first launch -> last launch of the step, device time */
	float    kernel_ms[SGP_NUM_KERNEL_CLASSES];       /* summed launch durations per kernel class (HIP events) */
	uint32_t kernel_launches[SGP_NUM_KERNEL_CLASSES]; /* launches per class; name: sgp_kernel_class_name() */
	uint32_t sweep_bodies;          /* body slots one launch of the body-array sweep covers */
	uint32_t num_constraints;
	uint32_t num_contact_points;
	uint32_t num_colours;
	uint32_t row_layout;            /* what the velocity iterations of this step read per contact point: 0 full rows (192 B), 1 r x axis only (96 B), 2 none (lever arms + effective masses: 40 B per lane) */
} sgp_step_profile;

typedef struct sgp_world sgp_world;

/* ---- lifecycle ------------------------------------------------------------------------------- */
/* PhysicsWorld::init() (PhysicsWorld.cpp:250-273): once per process. Returns the device count found. */
int  sgp_init(void);
int  sgp_abi_version(void);
const char* sgp_last_error(void);
void sgp_default_settings(sgp_settings* out);
void sgp_default_world_desc(sgp_world_desc* out);
void sgp_default_body_desc(sgp_body_desc* out);
/* PhysicsWorld ctor / dtor (PhysicsWorld.cpp:462-543). */
int  sgp_world_create(const sgp_world_desc* desc, sgp_world** out);
int  sgp_world_destroy(sgp_world* w);

/* ---- bodies ---------------------------------------------------------------------------------- */
/* addObject (PhysicsWorld.cpp:1169-1311).  Returns SGP_ERR_REJECTED for |pos|>1e9 etc. */
int  sgp_body_add(sgp_world* w, const sgp_body_desc* d, uint32_t* id_out);
int  sgp_body_add_batch(sgp_world* w, const sgp_body_desc* d, uint32_t n, uint32_t* ids_out);
/* removeObject (:1315-1339) */
int  sgp_body_remove(sgp_world* w, uint32_t id);
/* activateObject (:1342-1346) */
int  sgp_body_activate(sgp_world* w, uint32_t id);
/* Body::GetShape()->GetVolume() through GetBodyLockInterface().TryGetBody() (BoatPhysics.cpp:40-43) */
int  sgp_body_get_volume(sgp_world* w, uint32_t id, float* volume_out);
/* setObjectLayer (:1349-1353) */
int  sgp_body_set_layer(sgp_world* w, uint32_t id, int32_t layer);
/* Every setter below returns SGP_ERR_INVALID for a non-finite argument and leaves the body untouched (the reference asserts finite
 * inputs, PhysicsWorld.cpp:548-556,625,710). */
/* setNewObToWorldTransform(pos,rot,linvel,angvel) (:607-620); SetPositionRotationAndVelocity. Does not activate. */
int  sgp_body_set_pose_vel(sgp_world* w, uint32_t id, const float pos[3], const float rot[4],
                           const float lin_vel[3], const float ang_vel[3]);
/* setNewObToWorldTransform(pos,rot,scale) (:546-604): zero velocity, new final shape size, activates. */
int  sgp_body_set_pose_shape(sgp_world* w, uint32_t id, const float pos[3], const float rot[4],
                             const float shape[4]);
/* setNewPosition (:623-633): SetPosition, DontActivate. */
int  sgp_body_set_pos(sgp_world* w, uint32_t id, const float pos[3]);
/* setLinearAndAngularVelToZero (:649-657) */
int  sgp_body_set_vel(sgp_world* w, uint32_t id, const float lin_vel[3], const float ang_vel[3]);
/* moveKinematicObject (:707-722): BodyInterface::MoveKinematic; no-op for non-kinematic bodies. */
int  sgp_body_move_kinematic(sgp_world* w, uint32_t id, const float target_pos[3], const float target_rot[4], float dt);
/* BodyInterface::AddForce / AddTorque / AddForce(at point) used by HoverCarPhysics.cpp:113-348, BoatPhysics.cpp:221-267.
 * Accumulate until the next step, then cleared. Activate the body. */
int  sgp_body_add_force(sgp_world* w, uint32_t id, const float force[3]);
int  sgp_body_add_force_at(sgp_world* w, uint32_t id, const float force[3], const float point[3]);
int  sgp_body_add_torque(sgp_world* w, uint32_t id, const float torque[3]);
/* Batched form of setNewObToWorldTransform(pos,rot,linvel,angvel) for network physics snapshots (GUIClient.cpp:7474-7478 inserts
 * one snapshot per object per frame; n objects here cost one upload + one kernel). */
typedef struct sgp_pose_vel { float pos[3]; float rot[4]; float lin_vel[3]; float ang_vel[3]; } sgp_pose_vel;
int  sgp_body_set_pose_vel_batch(sgp_world* w, const uint32_t* ids, const sgp_pose_vel* recs, uint32_t n);

/* ObjectPhysicsTransformUpdate payload (Protocol.h:120, written at GUIClient.cpp:7637-7650): little endian,
 * uid u64 | pos 3 x f64 | rot 4 x f32 (x,y,z,w) | lin vel 3 x f32 | ang vel 3 x f32 | client time f64  = 80 bytes. */
#define SGP_PHYSICS_UPDATE_BYTES 80
int  sgp_physics_update_encode(uint64_t uid, const sgp_body_state* st, double client_time, uint8_t out[SGP_PHYSICS_UPDATE_BYTES]);
int  sgp_physics_update_decode(const uint8_t in[SGP_PHYSICS_UPDATE_BYTES], uint64_t* uid_out, sgp_pose_vel* rec_out, double* client_time_out);

/* ---- network physics snapshots: the de-jitter buffer in front of the step -------------------------------------
 * What the reference keeps per WorldObject (shared/WorldObject.h:540-566: a ring of HISTORY_BUF_SIZE = 4 snapshots, next_snapshot_i,
 * next_insertable_snapshot_i, transmission_time_offset) and does with it:
 *   receive    ClientThread.cpp:736-792   an ObjectPhysicsTransformUpdate from the object's physics owner goes into slot next_snapshot_i % 4
 *   ownership  ClientThread.cpp:957-975   ObjectPhysicsOwnershipTaken: transmission_time_offset = global time now - the sender's time of the
 *                                         change (a renewal only sets it when it is still 0); a change of owner drops the queued snapshots
 *   playback   GUIClient.cpp:7462-7493    once per frame and object: the oldest snapshot not yet inserted is due when
 *                                         global_time >= client_time + transmission_time_offset + padding_delay (0.1 s); it is then fed to
 *                                         setNewObToWorldTransform(pos, rot, lin vel, ang vel) -- here: returned for ONE batched
 *                                         sgp_body_set_pose_vel_batch.  At most one snapshot per object and poll, in arrival order; a ring
 *                                         that overflowed (more than 4 pending) plays back what its slots hold now, exactly as the reference's.
 *   expiry     GUIClient.cpp:7443-7452    an object whose last snapshot arrived more than 1 s ago leaves the active set
 * Host-side state only (no device work); one queue serves any number of objects, keyed by their 64-bit uid. */
typedef struct sgp_snapshot_queue sgp_snapshot_queue;
#define SGP_SNAPSHOT_HISTORY 4
int  sgp_snapshot_queue_create(sgp_snapshot_queue** out);
int  sgp_snapshot_queue_destroy(sgp_snapshot_queue* q);
/* receive: a wire record (sgp_physics_update_decode) or an already decoded one; local_time = the receiver's clock at arrival */
int  sgp_snapshot_queue_push_wire(sgp_snapshot_queue* q, const uint8_t msg[SGP_PHYSICS_UPDATE_BYTES], double local_time);
int  sgp_snapshot_queue_push(sgp_snapshot_queue* q, uint64_t uid, const sgp_pose_vel* rec, double client_time, double local_time);
/* ObjectPhysicsOwnershipTaken for uid */
int  sgp_snapshot_queue_ownership(sgp_snapshot_queue* q, uint64_t uid, double global_time_now, double ownership_change_global_time, int renewal);
/* playback: the snapshots due at global_time, at most one per object, ascending uid; *n_out = how many were due (<= cap are written and consumed) */
int  sgp_snapshot_queue_poll(sgp_snapshot_queue* q, double global_time, double padding_delay,
                             uint64_t* uids_out, sgp_pose_vel* recs_out, uint32_t cap, uint32_t* n_out);
/* expiry: forget the objects whose last snapshot arrived before local_time_now - max_age (reference: 1.0 s); *n_out = objects still tracked */
int  sgp_snapshot_queue_expire(sgp_snapshot_queue* q, double local_time_now, double max_age, uint32_t* n_out);
/* inspection (tests): ring indices and offset of one object; SGP_ERR_BAD_ID when the uid is not tracked */
int  sgp_snapshot_queue_peek(sgp_snapshot_queue* q, uint64_t uid, uint32_t* next_snapshot_i, uint32_t* next_insertable_snapshot_i, double* transmission_time_offset);

/* getObjectLinearVelocity (:636-646), getPosInJolt (:1625-1632), GUIClient.cpp:6588,6673 read-back. */
int  sgp_body_get_state(sgp_world* w, const uint32_t* ids, uint32_t n, sgp_body_state* out);
/* All live bodies in id order [first, first+n). Slots that are not live get id = SGP_INVALID_ID. */
int  sgp_world_read_states(sgp_world* w, uint32_t first, uint32_t n, sgp_body_state* out);
/* The per-frame read-back loop (GUIClient.cpp:6581-6690): compacted states of every ACTIVE body. */
int  sgp_world_read_active(sgp_world* w, sgp_body_state* out, uint32_t cap, uint32_t* n_out);
/* The same without the copy into the caller's buffer: *view_out points at a pinned host buffer of the library holding *n_out records.  The
 * buffer belongs to the two *_view calls alone: it stays valid and unchanged across steps, ray casts, queries and state reads, until the next
 * sgp_world_read_active_view / sgp_world_read_active_poses_view on this world or sgp_world_destroy (the loop at GUIClient.cpp:6581-6690
 * reads each record once, and may trace rays while it does). */
int  sgp_world_read_active_view(sgp_world* w, const sgp_body_state** view_out, uint32_t* n_out);
/* ... and with nothing but what that loop reads per activated body (GetPositionAndRotation, GUIClient.cpp:6586-6588): 32 bytes instead of 68. */
typedef struct sgp_body_pose {
	float    pos[3];
	uint32_t id;
	float    rot[4];            /* x, y, z, w */
} sgp_body_pose;
int  sgp_world_read_active_poses_view(sgp_world* w, const sgp_body_pose** view_out, uint32_t* n_out);

/* ---- world state ----------------------------------------------------------------------------- */
/* setWaterBuoyancyEnabled / setWaterZ (PhysicsWorld.h:109-112) */
int  sgp_world_set_water(sgp_world* w, int enabled, float water_z);
/* Enable capture of contact added/persisted events (only needed when an event_listener is set). */
int  sgp_world_set_contact_events(sgp_world* w, int enabled);
/* think(dt) (PhysicsWorld.cpp:1356-1443): one PhysicsSystem::Update with 1 collision step + buoyancy sweep.
 * Blocks until the step has finished on the device.  A sleeping body that an awake one touches (or a wheel stands on) wakes up IN this
 * step, together with the island it fell asleep with, and collides in it (PhysicsSystem::JobFindCollisions appends what it wakes to the
 * active list); sgp_step_stats::num_wake_pairs counts the pairs that brings.  A step in which nothing is awake and nothing was edited
 * costs nothing (and forgets the previous step's contacts). */
int  sgp_world_step(sgp_world* w, float dt);
/* Same, n steps back to back with a single host sync at the end (GUIClient's sub-step loop, GUIClient.cpp:6382). */
int  sgp_world_step_n(sgp_world* w, float dt, uint32_t n);
/* Same as sgp_world_step but brackets every stage with HIP events on the world's stream. */
int  sgp_world_step_profiled(sgp_world* w, float dt, sgp_step_profile* out);
int  sgp_world_stats(sgp_world* w, sgp_step_stats* out);
/* How the steps so far were issued: replayed as a captured hipGraph, launched eagerly, or skipped because nothing was awake
 * (diagnostic; any pointer may be NULL). */
int  sgp_world_launch_counts(sgp_world* w, uint32_t* graph_replays_out, uint32_t* eager_steps_out, uint32_t* idle_steps_out);
/* Name of kernel class k of sgp_step_profile (NULL past the last class). */
const char* sgp_kernel_class_name(int k);
/* sizeof() of ABI struct number `which` (order: settings, world_desc, body_desc, body_state, body_event, contact_event,
 * ray, hit, step_stats, step_profile, ghost_record, vehicle_desc, vehicle_input, vehicle_state, hull_info, capsule_query,
 * query_contact, mesh_info, heightfield_desc, checkpoint_info, shape_query, -- 21 is not used and stays -1 --, shape_cast, cast_hit,
 * -- 24 is not used and stays -1 --, character_desc, character_input, character_state, character_contact, -- 29 is not used and stays -1 --,
 * particle, particle_state, particle_event) so bindings can verify their layout. */
int  sgp_abi_sizeof(int which);
/* activated_obs / newly_activated_obs maintenance + listener callbacks (PhysicsWorld.h:194-200). */
int  sgp_world_drain_events(sgp_world* w, int kind, void* out, uint32_t cap, uint32_t* n_out);
/* Events waiting per kind (index = SGP_EVENT_*), nothing drained: lets the caller size its buffers to what a step produced instead of to the
 * world's capacity (the facade's think() runs every frame: PhysicsWorld.cpp:1356-1443; its listeners get one call per event, :1499-1520). */
int  sgp_world_event_counts(sgp_world* w, uint32_t counts_out[5]);
/* ---- static compound bodies ---------------------------------------------------
 * Replaces JPH::StaticCompoundShapeSettings::AddShape(position, rotation, shape, user data) x n + Create() as MeshBuilding.cpp:396-407
 * uses it for portals (the arch mesh + a thin box across the opening).  The compound is a STATIC body made of n child shapes, each with
 * a pose in the compound's frame; every child occupies its own body slot(s) (world pose = compound pose o child pose, all children share
 * the desc's material, layer and userdata), so the broad phase, narrow phase and queries need no notion of a sub-shape.  The id returned
 * (= the first child's slot) stands for the whole compound: pose setters, layer changes and removal act on every child; ray hits,
 * capsule-query contacts and contact events report this id, with the child index in `sub_shape` where the struct has one.  `base` gives
 * pose, layer, friction, restitution, sensor flag and userdata; its shape fields are ignored; motion_type must be SGP_MOTION_STATIC. */
typedef struct sgp_compound_child {
	int32_t shape_type;         /* SGP_SHAPE_SPHERE / BOX / CAPSULE / HULL / MESH */
	float   shape[4];           /* as sgp_body_desc::shape */
	float   pos[3];             /* of the child's body frame in the compound's frame */
	float   rot[4];
} sgp_compound_child;
#define SGP_MAX_COMPOUND_CHILDREN 64
int  sgp_body_add_compound(sgp_world* w, const sgp_body_desc* base, const sgp_compound_child* children, uint32_t num_children, uint32_t* id_out);
/* Number of children of compound `id` (0 = not a compound). */
int  sgp_body_compound_size(sgp_world* w, uint32_t id, uint32_t* num_children_out);

/* Body::GetUserData() of a live body (what JPH::BodyLockRead users read, PlayerPhysics.cpp:519-530); host-side lookup, no device access. */
int  sgp_body_get_userdata(sgp_world* w, uint32_t id, uint64_t* userdata_out);
/* getNumObjects (:1635-1638) */
int  sgp_world_num_bodies(sgp_world* w, uint32_t* n_out);
/* The counters PhysicsWorld::getDiagnostics prints (PhysicsWorld.cpp:1578-1604: JPH::BodyManager::BodyStats + the mesh count of getMemUsageStats). */
typedef struct sgp_body_counts {
	uint32_t num_bodies, max_bodies;
	uint32_t num_static, num_dynamic, num_kinematic;
	uint32_t num_active_dynamic, num_active_kinematic;
	uint32_t num_meshes;             /* live triangle-mesh shapes */
	uint32_t num_hulls;              /* live convex-hull shapes   */
	uint32_t reserved_;
	uint64_t shape_bytes;            /* device bytes held by the mesh and hull tables */
} sgp_body_counts;
int  sgp_world_body_counts(sgp_world* w, sgp_body_counts* out);

/* Debug / test view (not a facade entry point): the contact constraints of the last step, sorted by (a,b).
 * Record layout: {u32 a,b; i32 colour,np; f32 n[3], lam_n[4], lam_t1[4], lam_t2[4], bias[4]}. */
int  sgp_world_dump_constraints(sgp_world* w, void* out, uint32_t cap, uint32_t* n_out);

/* ---- queries --------------------------------------------------------------------------------- */
/* traceRay / traceRayAgainstCollidableObs / doesRayHitAnything (PhysicsWorld.cpp:1668-1725), batched. */
int  sgp_raycast(sgp_world* w, const sgp_ray* rays, uint32_t n, sgp_hit* hits_out);
/* "Does this ray hit anything within max_t" (what doesRayHitAnything keeps of a ray: JPH::NarrowPhaseQuery::CastRay with the plain result, which may stop
 * at the first hit), batched: hit_out[i] is 1 or 0 and equals (sgp_raycast's hits_out[i].id != SGP_INVALID_ID) for the same ray -- the same stages, filters
 * (alive, ignore_id, collidable_only) and per-shape tests, leaving at the first accepted hit: no closest hit, normal, triangle or barycentrics.  One thread
 * per ray whatever n is: like every query it flushes pending edits, and it tells a resident ray server to leave instead of using it. */
int  sgp_raycast_any(sgp_world* w, const sgp_ray* rays, uint32_t n, uint8_t* hit_out);

/* ---- convex hull shapes ---------------------------------------------------------
 * Replaces JPH::ConvexHullShapeSettings(points).Create() (+ OffsetCenterOfMassShape / the principal-axes decomposition Jolt does
 * inside MassProperties) for dynamic meshes and vehicle bodies (gui_client/PhysicsWorld.cpp:735-1166 with is_dynamic,
 * CarPhysics.cpp:66-92, BikePhysics.cpp:76-112).  Up to 256 hull vertices / 512 faces / 768 edges (JPH::ConvexHullShape::cMaxPointsInHull; 32 / 60 before round 5); larger clouds are
 * reduced to their extreme points (every input point takes part, up to 100000).  Points must already carry the object's scale (ScaledShape is baked in).
 * The hull is stored in its BODY frame (origin = centre of mass, axes = principal axes of inertia).  `com` / `rot` give that
 * frame in the frame of the input points:  input point = com + rot * body point.  A caller that thinks in the points' frame
 * (object space) places the body at  pos_body = pos_obj + R_obj * com,  rot_body = rot_obj * rot. */
typedef struct sgp_hull_info {
	uint32_t hull_id;                 /* >= 1; goes into sgp_body_desc::shape[0] with shape_type = SGP_SHAPE_HULL                */
	uint32_t num_vertices, num_faces, num_edges;
	float com[3];  float rot[4];
	float volume;  float unit_inertia[3];     /* principal moments for density 1 (body inertia = unit_inertia * mass / volume)    */
	float aabb_min[3], aabb_max[3];           /* body frame                                                                      */
} sgp_hull_info;
int  sgp_hull_create(sgp_world* w, const float* points_xyz, uint32_t num_points, sgp_hull_info* info_out);
/* The same wrapped in JPH::OffsetCenterOfMassShapeSettings(com_offset, hull) (PhysicsWorld.cpp:1138-1153, CarPhysics.cpp:76-78,
 * BikePhysics.cpp:103-105): the body's centre of mass sits at hull centre of mass + com_offset (frame of the points). */
int  sgp_hull_create_com(sgp_world* w, const float* points_xyz, uint32_t num_points, const float com_offset[3], sgp_hull_info* info_out);
/* The last JPH::Ref<JPH::Shape> to the hull going away: its id becomes reusable.  SGP_ERR_REJECTED while a body still uses it. */
int  sgp_hull_destroy(sgp_world* w, uint32_t hull_id);

/* ---- static triangle meshes ---------------------------------------------------
 * Replaces JPH::MeshShapeSettings(vertices, triangles).Create() for static mesh objects and -- through a triangulated grid --
 * JPH::HeightFieldShapeSettings for the terrain (gui_client/PhysicsWorld.cpp:735-1166 with is_dynamic = false, :1020-1120;
 * TerrainSystem.cpp:1300).  Vertices must already carry the object's scale.  Front faces (counter-clockwise) collide, back
 * faces do not.  Mesh bodies are static, live in the mesh's own frame (no centre-of-mass shift) and take three body ids. */
typedef struct sgp_mesh_info {
	uint32_t mesh_id;                 /* >= 1; goes into sgp_body_desc::shape[0] with shape_type = SGP_SHAPE_MESH */
	uint32_t num_vertices, num_triangles, num_nodes;
	float aabb_min[3], aabb_max[3];
} sgp_mesh_info;
int  sgp_mesh_create(sgp_world* w, const float* vertices_xyz, uint32_t num_vertices, const uint32_t* indices, uint32_t num_triangles, sgp_mesh_info* info_out);
/* The last JPH::Ref<JPH::Shape> to the mesh going away: its id and its vertex / triangle / node storage become reusable (Substrata streams
 * static meshes in and out as the camera moves).  SGP_ERR_REJECTED while a body still uses it. */
/* The active-edge bits of a mesh's triangles in the caller's triangle order: bit k set = edge k (vertex k -> vertex k + 1) collides with its own normal;
 * a clear bit = an edge shared by two (nearly) coplanar triangles, or a concave one: a contact there takes the triangle's normal (JPH::MeshShape's active
 * edges with the 5 degree default the reference keeps, PhysicsWorld.cpp:1028-1060).  Diagnostics / tests. */
int  sgp_mesh_edge_flags(sgp_world* w, uint32_t mesh_id, uint8_t* flags_out, uint32_t cap);
int  sgp_mesh_destroy(sgp_world* w, uint32_t mesh_id);
/* The same with one user-data word per triangle (JPH::IndexedTriangle::mMaterialIndex / MeshShape::GetTriangleUserData: the reference
 * stores the batch's material index there, PhysicsWorld.cpp:1032-1060), reported by ray hits.  NULL = all 0. */
int  sgp_mesh_create_with_materials(sgp_world* w, const float* vertices_xyz, uint32_t num_vertices, const uint32_t* indices, uint32_t num_triangles,
                                    const uint32_t* triangle_materials, sgp_mesh_info* info_out);

/* ---- height fields (JPH::HeightFieldShape, TerrainSystem.cpp:1300, PhysicsWorld.cpp:1086-1119) -----------------------------
 * A W x W grid of heights that collides exactly like the triangle mesh of the same samples (docs/CONTRACT.md 4d), without the mesh's
 * vertex, triangle and tree storage: triangles are found from the grid.  A field is an entry of the mesh table: bodies use it with
 * SGP_SHAPE_MESH and shape[0] = mesh_id, and sgp_mesh_destroy / sgp_mesh_edge_flags take its id.  sgp_mesh_info reports W * W
 * vertices, 2 (W - 1)^2 triangles, the number of 8 x 8-quad blocks as num_nodes, and the bounds of all vertices.
 *   frame      heights run along local +y; the grid lies in local x-z.
 *   samples    row-major: sample (x, z) is heights[z * W + x].
 *   vertex     of sample (x, z), fp32, in exactly this order, no contraction:
 *                ((spacing[0] * x + offset[0]) * scale[0], (h + offset[1]) * scale[1], (spacing[1] * z + offset[2]) * scale[2])
 *              (offset, spacing: HeightFieldShapeSettings inOffset / inScale; scale: the object's scale, baked in as for meshes)
 *              (with offset (0, 0, -quad_w (W - 1)) and spacing quad_w: the facade's triangulated chunk times the object's scale, bit for bit,
 *              except that a sample of -0.0 becomes +0.0: -0.0 + 0.0 = +0.0)
 *   triangles  the quad (x, z) has corners a = (x, z), b = (x + 1, z), c = (x, z + 1), d = (x + 1, z + 1); triangle 2 (z (W - 1) + x)
 *              is (a, c, d) and triangle 2 (z (W - 1) + x) + 1 is (a, d, b); both face +y.
 *   edges      active edges exactly as sgp_mesh_create finds them for that triangle list.
 *   materials  optional, one word per quad (z (W - 1) + x), reported for both its triangles in sgp_hit::material; NULL = 0.
 * SGP_ERR_INVALID unless W >= 2, every height is finite, spacing > 0, scale > 0 on every axis (a mirroring scale would turn the
 * triangles inside out: use a mesh) and 2 (W - 1)^2 < 2^29.  No power-of-two or block-size rule. */
typedef struct sgp_heightfield_desc {
	const float*    heights;          /* sample_count * sample_count heights, row-major */
	uint32_t        sample_count;     /* W */
	float           offset[3];
	float           spacing[2];       /* x, z */
	float           scale[3];
	uint32_t        reserved_;        /* must be 0 (SGP_ERR_INVALID otherwise) */
	const uint32_t* quad_materials;   /* (W - 1)^2 words or NULL */
} sgp_heightfield_desc;
int  sgp_heightfield_create(sgp_world* w, const sgp_heightfield_desc* desc, sgp_mesh_info* info_out);

/* ---- wheeled vehicles --------------------------------------------------------
 * Replaces JPH::VehicleConstraint + JPH::WheeledVehicleController + JPH::VehicleCollisionTesterCastSphere as CarPhysics
 * (and JPH::MotorcycleController + JPH::VehicleCollisionTesterCastCylinder as BikePhysics, gui_client/BikePhysics.cpp:97-230)
 * sets them up (gui_client/CarPhysics.cpp:62,94-231; script defaults gui_client/Scripting.cpp:315-346).  A vehicle is
 * attached to an existing dynamic body (the chassis; body origin = centre of mass).  Each step, before the forces:
 * one sphere cast per wheel, tyre slip -> friction, engine / clutch / gearbox / differential, brakes, anti-roll bars;
 * then 4 axis rows per wheel (suspension spring, max-up stop, longitudinal, lateral) are solved with the contact
 * constraints (before them in every iteration).  Field names follow JPH::WheelSettingsWV / VehicleEngineSettings /
 * VehicleTransmissionSettings / VehicleDifferentialSettings; sgp_default_vehicle_desc() fills Jolt's defaults. */
#define SGP_MAX_WHEELS 4
#define SGP_MAX_GEARS  8
#define SGP_VEHICLE_CONTROLLER_WHEELED     0   /* JPH::WheeledVehicleController (CarPhysics)                        */
#define SGP_VEHICLE_CONTROLLER_MOTORCYCLE  1   /* JPH::MotorcycleController (BikePhysics): + lean spring, lean steering limit */
#define SGP_VEHICLE_TESTER_SPHERE    0   /* JPH::VehicleCollisionTesterCastSphere of cast_radius (CarPhysics.cpp:62); radius 0: VehicleCollisionTesterRay */
#define SGP_VEHICLE_TESTER_CYLINDER  1   /* JPH::VehicleCollisionTesterCastCylinder(layer, inConvexRadiusFraction = 1) as BikePhysics.cpp:229 makes it: the wheel
                                          * itself is cast -- radius `radius`, width `width`, rounded by half its width -- from the attachment point over
                                          * suspension_max_length; no slope filter.  (Other fractions are not offered.) */
typedef struct sgp_wheel_desc {
	float position[3];            /* mPosition: suspension attachment point, chassis frame                       */
	float suspension_dir[3];      /* mSuspensionDirection (default (0,0,-1))                                      */
	float steering_axis[3];       /* mSteeringAxis (0,0,1)                                                        */
	float wheel_up[3];            /* mWheelUp (0,0,1)                                                             */
	float wheel_forward[3];       /* mWheelForward (0,1,0)                                                        */
	float suspension_min_length, suspension_max_length, suspension_preload;   /* 0.3, 0.5, 0                     */
	float spring_frequency, spring_damping;                                   /* 1.5 Hz, 0.5                     */
	float radius, width;                                                      /* 0.3, 0.1                        */
	float inertia, angular_damping;                                           /* 0.9 kg m^2, 0.2                 */
	float max_steer_angle, max_brake_torque, max_handbrake_torque;            /* 70 deg, 1500, 4000 N m          */
	float longitudinal_friction[3][2];   /* (slip ratio, friction): (0,0) (0.06,1.2) (0.2,1)                      */
	float lateral_friction[3][2];        /* (slip angle in degrees, friction): (0,0) (3,1.2) (20,1)               */
} sgp_wheel_desc;
typedef struct sgp_differential_desc { int32_t left_wheel, right_wheel; float differential_ratio, left_right_split, limited_slip_ratio, engine_torque_ratio; } sgp_differential_desc;
typedef struct sgp_anti_roll_bar_desc { int32_t left_wheel, right_wheel; float stiffness; } sgp_anti_roll_bar_desc;
typedef struct sgp_vehicle_desc {
	uint32_t body;                /* chassis body id                                                              */
	uint32_t num_wheels;          /* 1..SGP_MAX_WHEELS                                                            */
	sgp_wheel_desc wheels[SGP_MAX_WHEELS];
	float up[3], forward[3];      /* VehicleConstraintSettings::mUp / mForward, chassis frame                      */
	float cast_radius;            /* VehicleCollisionTesterCastSphere radius (CarPhysics: 0.5 * wheel width); 0 = ray */
	float max_slope_angle;        /* hits steeper than this against world +z are ignored (80 deg)                  */
	float engine_max_torque, engine_min_rpm, engine_max_rpm, engine_inertia, engine_angular_damping;   /* 500, 1000, 6000, 0.5, 0.2 */
	float engine_torque_curve[3][2];     /* (rpm / max rpm, torque fraction): (0,0.8) (0.66,1) (1,0.8)             */
	uint32_t num_gears, num_reverse_gears;
	float gear_ratios[SGP_MAX_GEARS], reverse_gear_ratios[SGP_MAX_GEARS];    /* 2.66 1.78 1.3 1.0 0.74 / -2.9     */
	float switch_time, clutch_release_time, switch_latency, shift_up_rpm, shift_down_rpm, clutch_strength;   /* .5 .3 .5 4000 2000 10 */
	uint32_t num_differentials;
	sgp_differential_desc differentials[2];
	float differential_limited_slip_ratio;   /* 1.4 */
	uint32_t num_anti_roll_bars;
	sgp_anti_roll_bar_desc anti_roll_bars[2];
	/* JPH::MotorcycleControllerSettings (BikePhysics.cpp:197-205); ignored for SGP_VEHICLE_CONTROLLER_WHEELED */
	uint32_t controller_type;                /* SGP_VEHICLE_CONTROLLER_*                                            */
	float max_lean_angle;                    /* mMaxLeanAngle 45 deg                                               */
	float lean_spring_constant, lean_spring_damping;                       /* 5000, 1000                            */
	float lean_spring_integration_coefficient, lean_spring_integration_decay;   /* 0, 4                              */
	float lean_smoothing_factor;             /* 0.8                                                                */
	uint32_t lean_steering_limit;            /* mEnableLeanSteeringLimit (1)                                       */
	uint32_t collision_tester;               /* SGP_VEHICLE_TESTER_* (0: the sphere / ray of cast_radius)          */
} sgp_vehicle_desc;
/* WheeledVehicleController::SetDriverInput(forward, right, brake, hand brake) (CarPhysics.cpp:366-367) */
typedef struct sgp_vehicle_input { float forward, right, brake, hand_brake; } sgp_vehicle_input;
/* What CarPhysics reads back from JPH::Wheel (CarPhysics.cpp:405-470) and the controller (BikePhysics.cpp:707) */
typedef struct sgp_wheel_state {
	float suspension_length, steer_angle, rotation_angle, angular_velocity;
	int32_t has_contact; uint32_t contact_body;
	float contact_position[3], contact_normal[3], contact_longitudinal[3], contact_lateral[3], contact_point_velocity[3];
	float suspension_lambda, longitudinal_lambda, lateral_lambda;
	float longitudinal_slip, lateral_slip;
} sgp_wheel_state;
typedef struct sgp_vehicle_state {
	sgp_wheel_state wheels[SGP_MAX_WHEELS];
	float engine_rpm; int32_t current_gear; float clutch_friction; int32_t active;
} sgp_vehicle_state;
void sgp_default_vehicle_desc(sgp_vehicle_desc* d);         /* Jolt defaults + CarPhysics' 4-wheel FWD layout, Scripting.cpp defaults */
int  sgp_vehicle_create(sgp_world* w, const sgp_vehicle_desc* d, uint32_t* vehicle_id_out);   /* AddConstraint + AddStepListener, CarPhysics.cpp:224-226 */
int  sgp_vehicle_destroy(sgp_world* w, uint32_t vehicle_id);                                  /* RemoveConstraint / RemoveStepListener, :258-262 */
int  sgp_vehicle_set_input(sgp_world* w, uint32_t vehicle_id, const sgp_vehicle_input* in);
int  sgp_vehicle_set_inputs(sgp_world* w, uint32_t first_vehicle_id, uint32_t n, const sgp_vehicle_input* in);
int  sgp_vehicle_get_state(sgp_world* w, uint32_t vehicle_id, sgp_vehicle_state* out);
int  sgp_vehicle_get_states(sgp_world* w, uint32_t first_vehicle_id, uint32_t n, sgp_vehicle_state* out);
/* MotorcycleController::EnableLeanController (BikePhysics.cpp:493,617) */
int  sgp_vehicle_enable_lean_controller(sgp_world* w, uint32_t vehicle_id, int enabled);
/* vehicleSummoned(): GetEngine().SetCurrentRPM / Wheel::SetAngularVelocity (CarPhysics.cpp:266-272) */
int  sgp_vehicle_reset_drivetrain(sgp_world* w, uint32_t vehicle_id, float engine_rpm, float wheel_angular_velocity);

/* ---- shape queries for the character controller ----------------------------------------------------
 * What JPH::CharacterVirtual asks the world every update (PlayerPhysics.cpp:64-90,258-353,477-481): every body within reach of
 * the character's capsule (CollideShape with a maximum separation) and a swept test of its path.  The controller itself (plane
 * constraints, sliding, ground state, stairs) is host code on top of these two batched queries (shim/Jolt/JoltCharacterLite.h). */
typedef struct sgp_capsule_query {
	float    pos[3];            /* centre of the capsule                                                            */
	float    rot[4];            /* the capsule axis is the local z axis                                             */
	float    radius, half_height;
	float    max_separation;    /* report surfaces closer than this (predictive contact distance + character padding) */
	uint32_t ignore_id;         /* JPH::IgnoreSingleBodyFilter (PlayerPhysics.cpp:477)                             */
	uint32_t collidable_only;   /* PlayerPhysicsObjectLayerFilter (PlayerPhysics.cpp:240-249)                      */
	float    movement[3];       /* CollideShapeSettings::mActiveEdgeMovementDirection (CharacterVirtual passes the direction it moves in); only its direction matters */
	uint32_t active_edges;      /* 1: EActiveEdgeMode::CollideOnlyWithActive -- a hit on an inactive edge of a mesh takes the triangle's normal unless the
	                               movement runs against the triangle more steeply along the found one (what CharacterVirtual asks for); 0: every edge collides with its own normal */
} sgp_capsule_query;
typedef struct sgp_query_contact {
	uint32_t query;             /* index of the query                                                              */
	uint32_t body;
	float    point[3];          /* on the body                                                                     */
	float    normal[3];         /* from the body towards the capsule                                               */
	float    distance;          /* separation along the normal; negative = penetration depth                       */
	float    point_velocity[3]; /* velocity of the body at `point`                                                 */
	uint32_t motion_type;       /* SGP_MOTION_*                                                                    */
	uint32_t is_sensor;
	float    inv_mass;          /* 0 unless dynamic                                                                */
	uint32_t sub_shape;         /* compound bodies: index of the touched child (`body` is the compound's id); 0 otherwise
	                               -> JPH::SubShapeID of CharacterContactListener::OnContactAdded (GUIClient.cpp:6484-6486)   */
	uint64_t userdata;
} sgp_query_contact;
/* Contacts come back sorted by (query, body, point). n_out may exceed cap (then only the first cap are written). */
int  sgp_collide_capsules(sgp_world* w, const sgp_capsule_query* queries, uint32_t n, sgp_query_contact* out, uint32_t cap, uint32_t* n_out);
/* Sphere casts (rays with thickness): hit.t = distance travelled by the centre until first touch, hit.normal at the touch point. */
int  sgp_spherecast(sgp_world* w, const sgp_ray* rays, const float* radii, uint32_t n, sgp_hit* hits_out);

/* ---- batched virtual characters (JPH::CharacterVirtual for many avatars at once) ---------------------
 * A batch of kinematic characters that belongs to one world.  sgp_characters_update runs CharacterVirtual::Update / ExtendedUpdate for
 * every character of the batch in ONE launch on the world's stream -- contacts, plane constraints, sliding, the swept tests, ground
 * state, stick-to-floor and stairs, all on the device, with the character state living there -- and returns without waiting for it.
 * The algorithm, its constants and its fp32 expressions are those of shim/Jolt/JoltCharacterLite.h (the host class that walks one
 * character at a time through sgp_collide_capsules / sgp_spherecast): a character of a batch moves as that class moves it.
 * The capsule's axis is the world z axis (identity rotation, as PlayerPhysics uses it).  Characters do not collide with each other.
 * A world checkpoint holds nothing of a batch; sgp_characters_checkpoint / _rollback do ("batch checkpoints", below). */
typedef struct sgp_characters sgp_characters;
#define SGP_CHAR_EXTENDED  1u   /* ExtendedUpdate (stick to floor, stairs); without it the plain Update of PlayerPhysics::updateForInVehicle */
#define SGP_CHAR_NO_SLIDE  2u   /* PlayerPhysics::OnContactSolve (PlayerPhysics.cpp:536-545): a contact whose velocity is near zero (squared length <= 1e-12)
                                   and whose normal is not too steep leaves the character with zero velocity                                  */
#define SGP_CHAR_DISABLED  4u   /* skipped by sgp_characters_update                                                                          */
/* CharacterBase::EGroundState */
#define SGP_GROUND_ON_GROUND        0
#define SGP_GROUND_ON_STEEP_GROUND  1
#define SGP_GROUND_NOT_SUPPORTED    2
#define SGP_GROUND_IN_AIR           3
#define SGP_CHAR_MAX_CONTACTS 64    /* contacts one query of a character keeps (the buffer of JoltCharacterLite.h); more: the overflow bit */
/* What CharacterVirtualSettings and CharacterVirtual::ExtendedUpdateSettings carry; sgp_default_character_desc fills Jolt's defaults. */
typedef struct sgp_character_desc {
	float    radius, half_height;     /* capsule: 0.3, 0.65 (half height of the cylinder part)                        */
	float    shape_offset[3];         /* from the character position to the capsule centre: (0,0,0)                   */
	float    up[3];                   /* mUp (0,1,0)                                                                  */
	float    supporting_plane[4];     /* mSupportingVolume: normal (0,0,1), constant 1e10                             */
	float    max_slope_angle;         /* 50 degrees, in radians (the library keeps its cosine)                        */
	float    mass, max_strength;      /* 70, 100                                                                      */
	float    predictive_contact_distance, character_padding, penetration_recovery_speed, collision_tolerance;   /* 0.1, 0.02, 1, 1e-3 */
	uint32_t max_collision_iterations, max_constraint_iterations;     /* 5, 15 (at most 16 and 64)                     */
	float    min_time_remaining;      /* 1e-4                                                                         */
	float    stick_to_floor_step_down[3];      /* (0,-0.5,0)                                                          */
	float    walk_stairs_step_up[3];           /* (0,0.4,0)                                                           */
	float    walk_stairs_min_step_forward, walk_stairs_step_forward_test, walk_stairs_cos_angle_forward_contact;   /* 0.02, 0.15, 0.2588 */
	float    walk_stairs_step_down_extra[3];   /* (0,0,0)                                                             */
} sgp_character_desc;
typedef struct sgp_character_input {
	float    velocity[3];             /* CharacterVirtual::SetLinearVelocity                                          */
	uint32_t ignore_id;               /* JPH::IgnoreSingleBodyFilter (PlayerPhysics.cpp:477); SGP_INVALID_ID: none    */
	uint32_t flags;                   /* SGP_CHAR_*                                                                   */
} sgp_character_input;
typedef struct sgp_character_state {
	float    pos[3];
	float    lin_vel[3];              /* GetLinearVelocity: as set, less what ExtendedUpdate cancelled towards steep slopes */
	uint32_t ground_state;            /* SGP_GROUND_*                                                                 */
	float    ground_normal[3], ground_velocity[3], ground_position[3];
	uint32_t ground_body;             /* SGP_INVALID_ID: none; a compound's id for its children                       */
	uint32_t ground_sub_shape;
	uint32_t overflow;                /* bit 0: a query of the last update met more than SGP_CHAR_MAX_CONTACTS contacts; bit 1: more bodies seen, contact
	                                     records or pushes than the character's slots hold (the rest was dropped)                                          */
	uint64_t ground_userdata;
} sgp_character_state;
/* CharacterContactListener::OnContactAdded: one record per (body, sub shape) a character newly touches */
typedef struct sgp_character_contact {
	uint32_t character, body, sub_shape, reserved_;
	uint64_t userdata;
	float    point[3], normal[3];
} sgp_character_contact;
void sgp_default_character_desc(sgp_character_desc* out);
int  sgp_characters_create(sgp_world* w, uint32_t capacity, sgp_characters** out);
/* After sgp_world_destroy of its world this still frees the batch and returns SGP_OK; every other call on such a batch is SGP_ERR_INVALID. */
int  sgp_characters_destroy(sgp_characters* cs);
/* Ids are slots of the batch; a removed slot is reused and carries nothing over.  SGP_ERR_INVALID for a degenerate description (a
 * non-positive or non-finite size, a zero up vector, iteration limits of 0 or beyond 16 / 64), SGP_ERR_CAPACITY for a full batch. */
int  sgp_character_add(sgp_characters* cs, const sgp_character_desc* desc, const float pos[3], uint32_t* id_out);
int  sgp_character_remove(sgp_characters* cs, uint32_t id);
int  sgp_characters_set_pose(sgp_characters* cs, const uint32_t* ids, const float* pos_xyz, uint32_t n);      /* teleport */
/* CharacterVirtual::SetShape with another capsule: the standing / sitting switch of PlayerPhysics.cpp:71-79 */
int  sgp_characters_set_shape(sgp_characters* cs, uint32_t id, float radius, float half_height, const float offset[3]);
/* Inputs of characters [first, first + n); they stay in force until set again.  A non-finite velocity is SGP_ERR_INVALID. */
int  sgp_characters_set_inputs(sgp_characters* cs, uint32_t first, uint32_t n, const sgp_character_input* inputs);
/* Advances every live character that is not disabled by dt: flushes pending body edits, makes the query grid valid (as
 * sgp_collide_capsules does), uploads changed inputs and enqueues the update on the world's stream.  No wait, no copy to the host.
 * Dynamic bodies in a character's way are pushed as CharacterVirtual pushes them: a second launch of the same call applies the push
 * records, waking the bodies on the device, with the effect of sgp_body_activate + sgp_body_add_force_at called in ascending character
 * order, then in order of occurrence -- the same bits on every run.  The world's next step is never skipped as idle after an update. */
int  sgp_characters_update(sgp_characters* cs, float dt);
/* Waits for the updates in flight.  Slots that are not live read as zeros with ground_state = SGP_GROUND_IN_AIR. */
int  sgp_characters_get_states(sgp_characters* cs, uint32_t first, uint32_t n, sgp_character_state* out);
/* The contact-added records since the last drain, ascending character, then order of discovery; *n_out = how many were pending
 * (<= cap are written; all are consumed).  A character holds at most 32 between drains. */
int  sgp_characters_drain_contacts(sgp_characters* cs, sgp_character_contact* out, uint32_t cap, uint32_t* n_out);

/* ---- driven characters: PlayerPhysics::update's velocity rule on the device (gui_client/PlayerPhysics.cpp:251-469) ----
 * A character with SGP_DRIVE_ON gets the velocity of its update from the rule PlayerPhysics::update applies before SetLinearVelocity --
 * walking at the desired velocity plus the ground's, air control capped at max_air_speed, swimming in the world's water, flying, gravity,
 * the 100 m/s falling cap, the jump through the ground normal -- computed inside sgp_characters_update's launch from what the previous
 * update left on the device (velocity, ground state, ground normal) and from a fresh UpdateGroundVelocity (a contact query at the
 * current position, made where the character has a ground body and is not flying, as PlayerPhysics.cpp:269 makes it).  The caller sends
 * what the player asks for and never reads a state back to move a character.  docs/CONTRACT.md 4n writes the rule out.
 * A driven character still honours sgp_character_input: `velocity` is SetLinearVelocity when it is set (a teleport's velocity,
 * addToLinearVel, a bounce pad), and the rule starts from it; ignore_id, SGP_CHAR_EXTENDED and SGP_CHAR_DISABLED act as before;
 * SGP_CHAR_NO_SLIDE is replaced by the rule's own !allow_sliding (allow_sliding = the desired velocity is not zero).
 * An undriven character (the default) moves exactly as before. */
#define SGP_DRIVE_ON            1u   /* the character's velocity comes from the rule, not from sgp_character_input::velocity alone */
#define SGP_DRIVE_FLY           2u   /* fly_mode */
#define SGP_DRIVE_GRAVITY       4u   /* gravity_enabled */
#define SGP_DRIVE_FREE_CAMERA   8u   /* CameraMode_FreeCamera: move_up is honoured as when flying */
#define SGP_DRIVE_SMOOTH_STAIRS 16u  /* camera height: the reference reads pre_stair_walk_position AFTER ExtendedUpdate (its `#if 1` branch), so its dz is 0,
                                        campos_z_delta stays 0 and the camera sits at pos.z + eye_height -- the default here.  With this flag dz is taken against the
                                        position just before the stair walk of the update: the reference's intent (its disabled branch), not its behaviour */
typedef struct sgp_character_drive {
	float    move_desired_vel[3];   /* what processMoveForwards / processStrafeRight summed, in m/s */
	float    move_up;               /* processMoveUp's factor * move_speed * run factor; the device adds (0,0,move_up) if flying, free camera or submerged > 0.3 */
	uint32_t flags;                 /* SGP_DRIVE_* */
	float    jump_speed, max_air_speed, eye_height;   /* 4.5, 8, 1.67 */
} sgp_character_drive;              /* 32 bytes */
typedef struct sgp_character_drive_state {
	float    cam_pos[3];            /* campos_out */
	float    campos_z_delta;
	float    last_xy_plane_vel_rel_ground[3];
	float    fraction_submerged;    /* of the last update */
	uint32_t on_ground, jumped;     /* of the last update */
	uint32_t num_jumps, pad_;       /* jumps since the slot's character was added */
} sgp_character_drive_state;        /* 48 bytes */
/* jump_speed 4.5, max_air_speed 8, eye_height 1.67, flags = SGP_DRIVE_GRAVITY, the rest 0 */
void sgp_default_character_drive(sgp_character_drive* out);
/* The drive of characters [first, first + n); it stays in force until set again.  All or nothing: a non-finite value, an unknown flag, a
 * negative jump_speed or max_air_speed, an eye_height not > 0 or a range beyond the live slots is SGP_ERR_INVALID and changes nothing. */
int  sgp_characters_set_drive(sgp_characters* cs, uint32_t first, uint32_t n, const sgp_character_drive* drives);
/* processJump: last_jump_time = cur_time for the characters named.  The jump fires in the first sgp_characters_update_at whose clock is
 * less than 0.1 s past cur_time and that finds the character supported.  A non-finite cur_time or an id that is not live: SGP_ERR_INVALID. */
int  sgp_characters_jump(sgp_characters* cs, const uint32_t* ids, uint32_t n, double cur_time);
/* sgp_characters_update with the caller's clock (PlayerPhysics::update's cur_time), which the jump window is measured against.
 * sgp_characters_update(cs, dt) is this call with a clock for which no jump window is open: a pending jump stays pending. */
int  sgp_characters_update_at(sgp_characters* cs, float dt, double cur_time);
/* Waits for the updates in flight.  Slots that are not live read as zeros; a character never driven has zeros too, but for cam_pos, which is its
 * position at the time it was added, an eye height up. */
int  sgp_characters_get_drive_states(sgp_characters* cs, uint32_t first, uint32_t n, sgp_character_drive_state* out);

/* ---- batched point particles (ParticleManager, gui_client/ParticleManager.cpp) -----------------------
 * A batch of point particles that belongs to one world and lives on the device.  sgp_particles_update runs ParticleManager::think
 * (ParticleManager.cpp:145-274) for every live particle on the world's stream -- one ray along the velocity for dt, answered by the very
 * function sgp_raycast runs per ray; reflection and restitution on a hit; water, gravity (the reference's literal 9.81) and drag; the
 * fade and growth of the sprite; removal of the dead -- with the fp32 expressions of the reference in its order (docs/CONTRACT.md,
 * "Particles") and returns without waiting.  Any body answers the ray: the facade's traceRay treats a body without userdata as a miss,
 * but every body the facade creates carries its object, so the two agree.  Particles never act on bodies or on each other.
 * Departures from the reference (docs/GAPS.md): the dead are removed by a STABLE compaction (survivors keep their order; the reference
 * swaps with the last), and a full batch replaces its particles in round-robin slot order (the reference picks a random victim).
 * A world checkpoint holds nothing of a batch; sgp_particles_checkpoint / _rollback do ("batch checkpoints", below).  In a tiled world particles see ghost bodies as bodies; nothing is exchanged. */
typedef struct sgp_particles sgp_particles;
#define SGP_PARTICLE_DIE_ON_HIT    1u   /* Particle::die_when_hit_surface (ParticleManager.cpp:189-190,198-206) */
#define SGP_PARTICLE_EV_DIED       1u   /* cur_opacity <= 0 after the update (ParticleManager.cpp:259-267): the particle is gone          */
#define SGP_PARTICLE_EV_FOAM       2u   /* addFoamDecal (ParticleManager.cpp:198-206) at (pos.x, pos.y, water_z) with width foam_width    */
#define SGP_PARTICLE_EV_REPLACED   4u   /* overwritten by a newcomer of a full batch (ParticleManager.cpp:91-96)                          */
#define SGP_PARTICLES_MAX_CAPACITY (1u << 20)
/* What the reference's Particle carries for the simulation (ParticleManager.h:25-60).  Colour, theta and the sprite type are render-only
 * and stay with the caller, keyed by `tag`, which stands for the caller's gl_ob. */
typedef struct sgp_particle {
	float    pos[3];
	float    vel[3];
	float    area;                 /* cross-sectional area (m^2): 1e-6        */
	float    mass;                 /* 1e-6; must be > 0                       */
	float    restitution;          /* 0.5                                     */
	float    width;                /* 1                                       */
	float    dwidth_dt;            /* 0.5                                     */
	float    opacity;              /* cur_opacity: 1                          */
	float    dopacity_dt;          /* -0.3                                    */
	uint32_t flags;                /* SGP_PARTICLE_DIE_ON_HIT                 */
	uint64_t tag;
} sgp_particle;
/* A live particle as sgp_particles_read reports it: what updateObjectTransformData needs (ParticleManager.cpp:250-253), and the rest of the moving state */
typedef struct sgp_particle_state {
	float    pos[3];
	float    width;
	float    vel[3];
	float    opacity;
	uint64_t tag;
	uint32_t flags;
	uint32_t reserved_;
} sgp_particle_state;
typedef struct sgp_particle_event {
	uint64_t tag;
	uint32_t kind;                 /* SGP_PARTICLE_EV_* bits                                                            */
	float    pos[3];               /* of the particle when the event was raised (after the update that raised it)       */
	float    width;                /* likewise                                                                          */
	float    foam_width;           /* FOAM: the decal's width = the particle's width BEFORE this update's growth; else 0 */
} sgp_particle_event;
/* The defaults of Particle() (ParticleManager.h:35-36); pos, vel, flags and tag are zero. */
void sgp_default_particle(sgp_particle* out);
/* capacity in 1 .. SGP_PARTICLES_MAX_CAPACITY (the reference's MAX_NUM_PARTICLES is 2048, ParticleManager.cpp:88); event_capacity: event
 * records the batch holds between two drains (0: events are only counted). */
int  sgp_particles_create(sgp_world* w, uint32_t capacity, uint32_t event_capacity, sgp_particles** out);
/* After sgp_world_destroy of its world this still frees the batch and returns SGP_OK; every other call on such a batch is SGP_ERR_INVALID. */
int  sgp_particles_destroy(sgp_particles* ps);
/* addParticle (ParticleManager.cpp:84-142), n at a time: enqueues an append behind the live particles and returns without waiting (the
 * host need not know the live count).  Newcomers that do not fit replace existing particles at slots cursor++ % capacity of a cursor
 * that lives on the device (ParticleManager.cpp:91-96 picks rng.nextUInt); every replaced particle raises a REPLACED event, in newcomer
 * order.  SGP_ERR_INVALID, with nothing added, for a non-finite pos / vel / scalar, mass <= 0 or an unknown flag; SGP_ERR_CAPACITY for
 * n > capacity. */
int  sgp_particles_add(sgp_particles* ps, const sgp_particle* particles, uint32_t n);
/* think(dt) (ParticleManager.cpp:145-274): flushes pending body edits, makes the query grid valid and parks the resident ray server (as
 * a batched sgp_raycast does), enqueues the update and returns.  No wait, no copy, no allocation; no body and nothing a step reads is
 * altered.  Water is the world's (sgp_world_set_water).  dt must be finite and >= 0. */
int  sgp_particles_update(sgp_particles* ps, float dt);
/* Waits for what is in flight, then writes the live particles in slot order.  *n_out = the live count; it may exceed cap (then only
 * the first cap are written). */
int  sgp_particles_read(sgp_particles* ps, sgp_particle_state* out, uint32_t cap, uint32_t* n_out);
/* The events since the last drain, in the order of the calls that raised them; within one update in ascending slot order, within one
 * add in newcomer order.  A particle that dies in the water raises ONE record with DIED | FOAM.  *n_out = records held (<= cap are
 * written; all are consumed), *n_dropped = events that did not fit event_capacity since the last drain. */
int  sgp_particles_drain_events(sgp_particles* ps, sgp_particle_event* out, uint32_t cap, uint32_t* n_out, uint32_t* n_dropped);
/* clearParticles (ParticleManager.cpp:74-81): no particle is live afterwards and the replacement cursor is back at slot 0; pending
 * events stay.  Enqueued, no wait. */
int  sgp_particles_clear(sgp_particles* ps);

/* ---- batched hover cars and boats (HoverCarPhysics, BoatPhysics of gui_client) ------------------------
 * A batch of scripted craft that belongs to one world and lives on the device.  sgp_crafts_update runs HoverCarPhysics::update
 * (HoverCarPhysics.cpp:76-407) or BoatPhysics::update (BoatPhysics.cpp:105-391) for every craft of the batch in one launch on the world's
 * stream, a lane per craft: it reads the body's pose, velocities and submerged volume where they live, evaluates the reference's fp32
 * expressions in the reference's order (docs/CONTRACT.md, "Crafts") and adds every force and torque to the body's accumulators in the order of
 * the reference's AddForce / AddTorque calls, with the arithmetic of sgp_body_activate / sgp_body_add_force / _force_at / _torque.  A hover
 * car with a driver casts its one ray with the function sgp_raycast runs per ray.  The dust, spray and foam an update makes go to an attached
 * sgp_particles batch without leaving the device.  Nothing is read back, nothing waits.
 * Departures from the reference (docs/GAPS.md): the random numbers are a counter-based generator of this library (glare-core's PCG32 is not
 * reproduced); a world checkpoint holds nothing of a batch (sgp_crafts_checkpoint / _rollback do); tiled worlds are refused; sgp_world_step_n advances n steps with ONE
 * update's forces where the reference updates per sub-step: step one at a time.
 * The caller creates a boat's body with use_zero_linear_drag = 1 (BoatPhysics.cpp:36 sets it on the object: the boat computes its own drag). */
typedef struct sgp_crafts sgp_crafts;
#define SGP_CRAFT_HOVERCAR 0u
#define SGP_CRAFT_BOAT     1u
#define SGP_CRAFT_MAX_SPLASH_POINTS 8
#define SGP_CRAFT_MAX_EMIT 22      /* particles one craft can make in one update: 6 jet foam + 2 x 8 splash (a hover car makes at most 4) */
#define SGP_CRAFTS_MAX_CAPACITY (1u << 16)
#define SGP_CRAFT_IN_DRIVER 1u     /* user_in_driver_seat.  Setting it on a boat stops its righting (BoatPhysics.cpp:80) */
#define SGP_CRAFT_IN_BOOST  2u     /* SHIFT_down: only the speed of a boat's jet foam (BoatPhysics.cpp:202) */
#define SGP_CRAFT_ST_BODY_GONE 1u  /* the body the craft was added on has been removed (its slot may hold another body): the craft is skipped */
/* sgp_craft_state::branches: which branches of the reference fired in the last update */
#define SGP_CRAFT_BR_HOVER       (1u << 0)    /* HoverCarPhysics.cpp:152-160 */
#define SGP_CRAFT_BR_UNFLIP      (1u << 1)    /* :168-175 (the world-space up force) */
#define SGP_CRAFT_BR_DRAG        (1u << 2)    /* :240-267, BoatPhysics.cpp:240-267 */
#define SGP_CRAFT_BR_LIFT_TOP    (1u << 3)    /* :280-287 */
#define SGP_CRAFT_BR_LIFT_BOTTOM (1u << 4)    /* :292-299 */
#define SGP_CRAFT_BR_LIFT_RIGHT  (1u << 5)    /* :309-313 */
#define SGP_CRAFT_BR_LIFT_LEFT   (1u << 6)    /* :318-322 */
#define SGP_CRAFT_BR_THRUST      (1u << 7)    /* BoatPhysics.cpp:183-216 */
#define SGP_CRAFT_BR_RUDDER      (1u << 8)    /* :219-226 */
#define SGP_CRAFT_BR_RIGHTING    (1u << 9)    /* :363-388 */
#define SGP_CRAFT_BR_RAY_BODY    (1u << 10)   /* HoverCarPhysics.cpp:378-400 (dust) */
#define SGP_CRAFT_BR_RAY_WATER   (1u << 11)   /* :353-375 (spray) */
#define SGP_CRAFT_BR_ACTIVATE    (1u << 12)   /* the ActivateBody on user input (:116-117, BoatPhysics.cpp:176-177) */
#define SGP_CRAFT_BR_SPLASH0     (1u << 16)   /* BoatPhysics.cpp:335-355 for splash point p: bit 16 + p */
/* kinds of the particles a craft makes: bits 28..31 of the low word of their tag */
#define SGP_CRAFT_PK_SPRAY  0u     /* hover car over water: Colour3f(0.6), ParticleType_Smoke */
#define SGP_CRAFT_PK_DUST   1u     /* hover car over ground: Colour3f(0.6, 0.4, 0.3), ParticleType_Smoke */
#define SGP_CRAFT_PK_JET    2u     /* boat jet foam: Colour3f(0.6), ParticleType_Foam */
#define SGP_CRAFT_PK_SPLASH 3u     /* boat splash: Colour3f(0.6), ParticleType_Foam */
typedef struct sgp_craft_desc {
	uint32_t kind;                 /* SGP_CRAFT_HOVERCAR | SGP_CRAFT_BOAT                                               */
	uint32_t body;                 /* a live dynamic body, no other craft of the batch on it                            */
	float    mass;                 /* hovercar_mass / boat_mass; > 0                                                    */
	float    model_to_y_forwards_rot_1[4];
	float    model_to_y_forwards_rot_2[4];
	uint32_t seed;                 /* of the craft's random numbers                                                     */
	uint64_t tag;                  /* the caller's (its WorldObject*); not interpreted                                  */
	float    trace_origin_os[3];   /* hover car: where the dust ray starts, object space with the object's scale applied
	                                  (HoverCarPhysics.cpp:331-337: aabb_os.centroid() - up_ms * axisLength * 0.51, scaled) */
	float    thrust_force;         /* the rest: boats (BoatScriptSettings); 40000                                       */
	float    propellor_point_os[3];                /* (0, 0.2, -6.2) */
	float    propellor_sideways_offset;            /* 1     */
	float    rudder_deflection_force_factor;       /* 500   */
	float    thrust_vector_lateral_amount;         /* 0     */
	float    jet_particle_initial_width;           /* 1     */
	float    front_cross_sectional_area;           /* 2     */
	float    side_cross_sectional_area;            /* 4     */
	float    top_cross_sectional_area;             /* 8     */
	uint32_t n_splash_points;      /* <= SGP_CRAFT_MAX_SPLASH_POINTS                                                    */
	float    splash_points[32];    /* SGP_CRAFT_MAX_SPLASH_POINTS x (point_os xyz, right_sign); right_sign is clamped to [-1, 1] (BoatPhysics.cpp:55) */
	float    shape_volume;         /* filled by sgp_craft_add from sgp_body_get_volume (0 -> 1, BoatPhysics.cpp:43-45); what the caller puts here is ignored */
} sgp_craft_desc;
/* Resolved analog values; the key mapping of HoverCarPhysics.cpp:82-110 / BoatPhysics.cpp:110-131 is the facade's (shim/CraftBatch.h). */
typedef struct sgp_craft_input {
	float    forward;              /* boats: with the boost doubling and the 0.2 of reversing already applied           */
	float    right;
	float    up;                   /* hover cars                                                                        */
	float    hand_brake;           /* hover cars: only wakes the body                                                   */
	uint32_t flags;                /* SGP_CRAFT_IN_*                                                                    */
} sgp_craft_input;
typedef struct sgp_craft_state {
	float    force[3];             /* what the last update added to the body's force accumulator                        */
	float    torque[3];            /* ... and to its torque accumulator (forces at a point: about the body position)    */
	uint32_t branches;             /* SGP_CRAFT_BR_*                                                                    */
	float    unflip_time_remaining;      /* unflip_up_force_time_remaining (-1: not unflipping)                         */
	float    righting_time_remaining;
	float    trace_origin[3];      /* last_trace_origin_ws                                                              */
	float    trace_t;              /* hit_t of the last ray; 0 without a hit                                            */
	uint32_t trace_body;           /* SGP_INVALID_ID: no ray cast, or nothing hit                                       */
	uint32_t n_emitted;            /* particles the last update made (counted with or without a batch attached)         */
	uint32_t status;               /* SGP_CRAFT_ST_*                                                                    */
	uint32_t update_index;         /* updates this craft has run                                                        */
	uint32_t reserved_;
} sgp_craft_state;
/* Zeros, identity rotations, and for SGP_CRAFT_BOAT the defaults of Scripting.cpp:229-239; mass 1000. */
void sgp_default_craft_desc(uint32_t kind, sgp_craft_desc* out);
/* capacity in 1 .. SGP_CRAFTS_MAX_CAPACITY.  A world that holds ghost bodies (a tile) is refused, as by sgp_characters_create. */
int  sgp_crafts_create(sgp_world* w, uint32_t capacity, sgp_crafts** out);
/* After sgp_world_destroy of its world this still frees the batch and returns SGP_OK; every other call on such a batch is SGP_ERR_INVALID. */
int  sgp_crafts_destroy(sgp_crafts* cs);
/* Ids are slots of the batch; a removed slot is reused and carries nothing over (timers at -1, update index and particle counter at 0).
 * SGP_ERR_INVALID, with nothing added, for a NULL, a non-finite value, mass <= 0, an unknown kind, a body that is not live and dynamic, a
 * second craft on the same body and n_splash_points > SGP_CRAFT_MAX_SPLASH_POINTS; SGP_ERR_CAPACITY for a full batch. */
int  sgp_craft_add(sgp_crafts* cs, const sgp_craft_desc* desc, uint32_t* id_out);
int  sgp_craft_remove(sgp_crafts* cs, uint32_t id);
/* Inputs of crafts [first, first + n); they stay in force until set again. */
int  sgp_crafts_set_inputs(sgp_crafts* cs, uint32_t first, uint32_t n, const sgp_craft_input* inputs);
/* startRightingVehicle: a boat's righting timer starts at 2 s with its next update (a hover car's does nothing, as in the reference). */
int  sgp_crafts_start_righting(sgp_crafts* cs, const uint32_t* ids, uint32_t n);
/* The batch that receives the particles (NULL: none; they are then only counted).  It must belong to the same world and hold at least
 * crafts capacity x SGP_CRAFT_MAX_EMIT particles (else SGP_ERR_CAPACITY): one update's output then always fits one append.  New particles go
 * behind the live ones in ascending craft order, then the reference's emission order, with the semantics of sgp_particles_add (overflow
 * replaces round-robin and raises REPLACED events in newcomer order).  Particle tag = craft id << 32 | kind << 28 | per-craft counter.
 * Detach (NULL) before the particle batch is destroyed. */
int  sgp_crafts_attach_particles(sgp_crafts* cs, sgp_particles* particles_or_null);
/* One update of every craft: flushes pending body edits, makes the query grid valid (as a batched sgp_raycast does), uploads what the host
 * changed and enqueues the update on the world's stream.  No wait, no copy to the host, no allocation.  The world's next step is never skipped
 * as idle afterwards.  A craft whose body has gone is skipped and touches nothing.  dt must be finite and >= 0. */
int  sgp_crafts_update(sgp_crafts* cs, float dt);
/* Waits for the updates in flight.  Slots that are not live read as zeros with trace_body = SGP_INVALID_ID. */
int  sgp_crafts_get_states(sgp_crafts* cs, uint32_t first, uint32_t n, sgp_craft_state* out);

/* ---- batched path and move-to controllers (ObjectPathController, ObjectMoveToController of gui_client) ----
 * A batch of scripted movers that belongs to one world and lives on the device: trains, trams and lifts on a closed waypoint loop with
 * carriages that follow a leader at a distance (SGP_MOVER_PATH), and doors and platforms with an eased position track and an eased rotation
 * track (SGP_MOVER_MOVETO).  Each is bound to one kinematic body.  sgp_movers_update runs ObjectPathController::update
 * (ObjectPathController.cpp:441-526) or ObjectMoveToController::update (ObjectMoveToController.cpp:58-114) for every mover, a lane per mover,
 * on the world's stream and gives the body the velocities of sgp_body_move_kinematic -- for a mesh body also its two alias slots --; nothing is
 * read back, nothing waits.  Call it before each sgp_world_step, where the reference runs its controllers (GUIClient.cpp:6394-6418).
 * The fp32 expressions and their order: docs/CONTRACT.md 4j.  Departures from the reference (docs/GAPS.md): an update passes at most
 * SGP_MOVER_MAX_SEGMENTS_PER_UPDATE segment ends forwards or segment starts backwards; a follower's leader is a walker on the same path (no
 * chains); a path has at most SGP_MOVER_MAX_WAYPOINTS waypoints; rotations are held as quaternions; a world checkpoint holds nothing of a batch (sgp_movers_checkpoint / _rollback do); tiled worlds are
 * refused; sgp_world_step_n advances n steps on one update. */
typedef struct sgp_movers sgp_movers;
#define SGP_MOVER_PATH   0u
#define SGP_MOVER_MOVETO 1u
#define SGP_WAYPOINT_CURVE_IN  0u     /* PathWaypointIn::CurveIn: start of a circular arc                                      */
#define SGP_WAYPOINT_CURVE_OUT 1u     /* CurveOut: end of a curve                                                              */
#define SGP_WAYPOINT_STATION   2u     /* Station: the object pauses here for pause_time seconds                                */
#define SGP_MOVER_EASE_LINEAR     0u  /* Protocol::MoveTo_EasingLinear                                                         */
#define SGP_MOVER_EASE_SMOOTHSTEP 1u  /* Protocol::MoveTo_EasingSmoothstep                                                     */
#define SGP_MOVER_ORIENT_ALONG_PATH 1u
#define SGP_MOVER_MAX_WAYPOINTS 128
#define SGP_MOVER_MAX_SEGMENTS_PER_UPDATE 64
#define SGP_MOVERS_MAX_CAPACITY (1u << 16)
#define SGP_MOVERS_MAX_PATHS    (1u << 12)
#define SGP_MOVER_ST_BODY_GONE   1u   /* the body is no longer the live kinematic body the mover was added on: the mover is skipped */
#define SGP_MOVER_ST_LEADER_GONE 2u   /* a follower whose leader was removed or lost its body: waypoint 0, direction (1,0,0)   */
#define SGP_MOVER_ST_OVERRUN     4u   /* the last update stopped at the cap of SGP_MOVER_MAX_SEGMENTS_PER_UPDATE               */
#define SGP_MOVER_ST_POS_ACTIVE  8u   /* pos_active after the last update                                                      */
#define SGP_MOVER_ST_ROT_ACTIVE  16u  /* rot_active after the last update                                                      */
typedef struct sgp_path_waypoint {
	float    pos[3];
	uint32_t type;                 /* SGP_WAYPOINT_*                                                                    */
	float    pause_time;           /* Station: seconds; finite, >= 0                                                    */
	float    speed;                /* to the next waypoint; finite, > 0                                                 */
} sgp_path_waypoint;
/* ObjectPathController::PathWaypoint.  The fields behind speed are derived by sgp_path_prepare; those of a curve are 0 on other waypoints. */
typedef struct sgp_path_segment {
	float    pos[3];
	uint32_t type;
	float    pause_time;
	float    speed;
	float    segment_len;          /* length along the segment to the next waypoint                                     */
	float    just_curve_len;       /* length along just the arc                                                         */
	float    entry_segment_len;    /* length of the straight part before the arc                                        */
	float    curve_angle;
	float    curve_r;
	float    exit_segment_unit_dir[3];
} sgp_path_segment;
typedef struct sgp_path_progress {
	uint32_t waypoint_index;       /* cur_waypoint_index: the waypoint we are at or have just passed                    */
	float    dist_along_segment;   /* m_dist_along_segment                                                              */
	float    time_along_segment;   /* m_time_along_segment (a station's pause counts)                                   */
} sgp_path_progress;
typedef struct sgp_mover_desc {
	uint32_t kind;                 /* SGP_MOVER_PATH | SGP_MOVER_MOVETO                                                 */
	uint32_t body;                 /* a live kinematic body: no compound, ghost or alias slot, no other mover of the batch on it */
	uint32_t flags;                /* SGP_MOVER_ORIENT_ALONG_PATH                                                       */
	uint32_t path;                 /* path movers: a path of sgp_movers_path_add                                        */
	double   initial_time;         /* path walkers: the global time; taken modulo the path's traversal time             */
	uint64_t tag;                  /* the caller's (its WorldObject*); not interpreted                                  */
	uint32_t leader;               /* path movers: the mover to follow -- a walker of this batch on the same path --, or SGP_INVALID_ID */
	float    follow_dist;          /* followers: distance behind the leader; finite, >= 0                               */
	float    base_rot[4];          /* path movers: the object's own rotation (fromAxisAndAngle(normalise(axis), angle)) */
	float    hold_pos[3];          /* move-to movers: what an inactive position track holds before any track has run    */
	float    hold_rot[4];          /* ... and an inactive rotation track                                                */
	uint32_t reserved_;
} sgp_mover_desc;
typedef struct sgp_mover_state {
	uint32_t status;               /* SGP_MOVER_ST_*                                                                    */
	uint32_t waypoint_index;       /* walkers: the state after the last update; followers: the segment they were placed on */
	float    dist_along_segment;
	float    time_along_segment;   /* walkers                                                                           */
	float    pos[3];               /* the target the last update moved the body towards                                 */
	float    rot[4];
	float    dir[3];               /* path movers: the direction along the path                                         */
	float    pos_elapsed;          /* move-to movers                                                                    */
	float    rot_elapsed;
	uint32_t update_index;         /* updates this mover has run (skipped ones do not count)                            */
} sgp_mover_state;
/* The constructor's segment loop (ObjectPathController.cpp:60-124) on the host, no world needed: out[0..n) and the traversal time of the loop.
 * SGP_ERR_INVALID for a NULL, n < 2 or > SGP_MOVER_MAX_WAYPOINTS, a segment shorter than 1e-5 or not finite (where the reference throws), and
 * for a speed not finite or not > 0, a pause_time negative or not finite, an unknown type (where the reference runs into undefined behaviour). */
int  sgp_path_prepare(const sgp_path_waypoint* in, uint32_t n, sgp_path_segment* out, double* total_time_out);
/* The state change of walkAlongPathForTime (:233-393) for dt, the arithmetic the device runs: bit-equal to it.  At most
 * SGP_MOVER_MAX_SEGMENTS_PER_UPDATE segment ends are passed: at the cap it stops at the start of the segment reached (dist = time = 0) and
 * ORs SGP_MOVER_ST_OVERRUN into *status_io.  dt <= 0 changes nothing.  SGP_ERR_INVALID for a NULL, n < 2, an index >= n, a dt that is not finite. */
int  sgp_path_advance(const sgp_path_segment* segs, uint32_t n, sgp_path_progress* io, float dt, uint32_t* status_io);
/* capacity in 1 .. SGP_MOVERS_MAX_CAPACITY movers, path_capacity in 1 .. SGP_MOVERS_MAX_PATHS paths of SGP_MOVER_MAX_WAYPOINTS segments each.
 * A world that holds ghost bodies (a tile) is refused, as by sgp_crafts_create. */
int  sgp_movers_create(sgp_world* w, uint32_t capacity, uint32_t path_capacity, sgp_movers** out);
/* After sgp_world_destroy of its world this still frees the batch and returns SGP_OK; every other call on such a batch is SGP_ERR_INVALID. */
int  sgp_movers_destroy(sgp_movers* ms);
/* Paths are shared by movers and counted by reference: sgp_movers_path_remove of a path in use answers SGP_ERR_INVALID and removes nothing. */
int  sgp_movers_path_add(sgp_movers* ms, const sgp_path_waypoint* waypoints, uint32_t n, uint32_t* path_id_out);
int  sgp_movers_path_remove(sgp_movers* ms, uint32_t path_id);
/* Copies the prepared segments of a path (for drawing, evalSegmentCurvePos): up to cap of them; *n_out their number. */
int  sgp_movers_path_get(sgp_movers* ms, uint32_t path_id, sgp_path_segment* out, uint32_t cap, uint32_t* n_out);
/* A walker (leader == SGP_INVALID_ID) starts where walkAlongPathForTime((float) doubleMod(initial_time, traversal time)) leaves it from
 * (0, 0, 0), as the constructor does; the body is not moved by the add.  SGP_ERR_INVALID, with nothing added, for a NULL, an unknown kind or
 * flag, a non-finite value, a body that does not qualify or carries a mover already, a path that is not live, a leader that is not a live
 * walker of this batch on the same path, follow_dist < 0; SGP_ERR_CAPACITY for a full batch. */
int  sgp_mover_add(sgp_movers* ms, const sgp_mover_desc* desc, uint32_t* id_out);
/* The followers of a removed walker take the reference's fallback for a missing leader (SGP_MOVER_ST_LEADER_GONE). */
int  sgp_mover_remove(sgp_movers* ms, uint32_t id);
/* ObjectMoveToController::setPositionTrack / setRotationTrack for a move-to mover: duration is clamped to >= 1e-4 and cur_elapsed to >= 0, the
 * track is active from the next update on and replaces the one that runs.  easing: SGP_MOVER_EASE_*. */
int  sgp_movers_set_position_track(sgp_movers* ms, uint32_t id, const float start[3], const float target[3], float duration, uint32_t easing, float cur_elapsed);
int  sgp_movers_set_rotation_track(sgp_movers* ms, uint32_t id, const float start[4], const float target[4], float duration, uint32_t easing, float cur_elapsed);
/* One update of every mover: flushes pending body edits, uploads what the host changed and enqueues the update on the world's stream -- a
 * second launch for the followers, which see where their leaders went in this update.  No wait, no copy to the host, no allocation.  The
 * world's next step is never skipped as idle afterwards.  A mover whose body has gone, and a move-to mover with both tracks inactive, touch
 * nothing.  dt must be finite and >= 0; dt == 0 returns without a launch. */
int  sgp_movers_update(sgp_movers* ms, float dt);
/* Waits for the updates in flight.  A mover that has not been updated since it was added reads as its initial state; slots that are not live
 * read as zeros. */
int  sgp_movers_get_states(sgp_movers* ms, uint32_t first, uint32_t n, sgp_mover_state* out);

/* ---- overlap queries with any convex shape (JPH::NarrowPhaseQuery::CollideShape) --------------------
 * "What is inside this volume?": a box for a parcel or a trigger volume, a sphere for an explosion or an audio radius, the hull of an
 * object for a placement test before it is added -- thousands of them per call if need be.  Every query reports the contacts of its shape
 * with every body whose surface lies within max_separation of it, as sgp_query_contact records: `normal` points from the body towards
 * the query shape, `point` lies on the body, sensors are reported.  A compound child reports the compound's id and its child index in
 * `sub_shape`. */
#define SGP_QUERY_DEEPEST_ONLY 1u   /* sgp_shape_query::flags */
typedef struct sgp_shape_query {
	float    pos[3], rot[4];
	int32_t  shape_type;        /* SGP_SHAPE_SPHERE | BOX | CAPSULE | HULL; shape[] as in sgp_body_desc (hull: shape[0] = hull id of this world) */
	float    shape[4];
	float    max_separation;    /* report surfaces closer than this; 0 = touching or overlapping only */
	uint32_t ignore_id;
	uint32_t layer_mask;        /* bit l set: bodies of layer l answer; 0 = all four (collidable_only of the capsule query = 0x3) */
	uint32_t flags;             /* SGP_QUERY_DEEPEST_ONLY: one contact per (query, body), the deepest point of its first manifold
	                               (a compound answers once per touched child) */
	float    movement[3];
	uint32_t active_edges;      /* as in sgp_capsule_query */
} sgp_shape_query;
/* Contacts come back sorted by (query, body, point).  n_out is the exact size of the whole answer and may exceed cap: what is written is then
 * the first cap records of the sorted answer.  SGP_ERR_INVALID, with nothing launched and nothing written, when any query names a hull that
 * does not exist, asks with SGP_SHAPE_MESH (or an unknown type), or holds a non-finite pose or a non-positive size.  n == 0 is SGP_OK.
 * Many small volumes are answered from a list of candidate (query, body) pairs, a thread per pair; a few large ones by a wave per query:
 * the same records either way (SGP_QUERY_PATH=wave|pairs, read at world creation, forces one). */
int  sgp_collide_shapes(sgp_world* w, const sgp_shape_query* queries, uint32_t n, sgp_query_contact* out, uint32_t cap, uint32_t* n_out);

/* ---- shape casts with any convex shape (JPH::NarrowPhaseQuery::CastShape) ----------------------------
 * "How far can this volume travel before it touches something?": the hull of an object lowered onto the scene, a kinematic platform moved up
 * to the first obstacle, the box of a projectile, the character's capsule as a whole.  The shape keeps its rotation and translates from `pos`
 * along `dir`; every cast reports its closest hit.  On equal t the lower body id wins, then the lower triangle index (the rule of
 * sgp_spherecast).  Sensors, dead slots, `ignore_id` and masked layers never answer (as for rays and sphere casts).  Bodies of every shape
 * answer; a compound child reports the compound's id and its child index; mesh and height-field triangles answer on their front side only and
 * every edge with its own normal (no active-edge treatment).
 *
 * The contract of t, with SGP_CAST_TOLERANCE (Jolt's default collision tolerance for casts):
 *   - at the reported t the shape and the body are separated by at most SGP_CAST_TOLERANCE along `normal`;
 *   - at no t' < t does the shape overlap a body that passes the filters by more than fp32 rounding;
 *   - a reported miss means no such overlap anywhere in [0, max_t];
 *   - the record is a function of the cast and the world alone: not of the batch it came in, its place in the batch, or the order of any atomics.
 * The sweep is conservative advancement over the library's pairwise separation functions (sgp_k_shapecast.hip); pairs with a rounded shape at
 * an edge or corner converge geometrically, and a cast that runs into the iteration cap reports the t it got to (never past the true hit) and is
 * counted (sgp_cast_shapes_counters). */
#define SGP_CAST_TOLERANCE 1.0e-4f
typedef struct sgp_shape_cast {
	float    pos[3], rot[4];    /* pose at t = 0 */
	int32_t  shape_type;        /* SGP_SHAPE_SPHERE | BOX | CAPSULE | HULL; shape[] as in sgp_shape_query */
	float    shape[4];
	float    dir[3];            /* unit, as in sgp_ray */
	float    max_t;             /* >= 0 */
	uint32_t ignore_id;
	uint32_t layer_mask;        /* as in sgp_shape_query; 0 = all four */
	uint32_t flags;             /* 0; reserved */
} sgp_shape_cast;
typedef struct sgp_cast_hit {
	uint32_t id;                /* SGP_INVALID_ID: nothing within max_t */
	float    t;                 /* distance travelled until first touch; 0 when the shape starts in touch or overlapping */
	float    normal[3];         /* from the body towards the shape, at the touch */
	float    point[3];          /* on the body */
	float    penetration;       /* > 0 only for t == 0 hits that start overlapping */
	uint32_t sub_shape;         /* compound child index, as in sgp_query_contact */
	uint32_t triangle, material;/* mesh / height-field hits, as in sgp_hit; SGP_INVALID_ID / 0 otherwise */
	uint64_t userdata;
} sgp_cast_hit;
/* SGP_ERR_INVALID, with nothing launched and nothing written and the message naming the cast, for what sgp_collide_shapes rejects (unknown
 * hull, SGP_SHAPE_MESH or an unknown type, a non-finite pose, a non-positive size), a `dir` that is not finite or not unit within 1e-3, and a
 * negative or non-finite max_t.  n == 0 is SGP_OK. */
int  sgp_cast_shapes(sgp_world* w, const sgp_shape_cast* casts, uint32_t n, sgp_cast_hit* hits_out);
/* counters_out[0]: (cast, body or triangle) pairs of every call so far that ran into the iteration cap; [1]: runs that were repeated because a
 * candidate list was too small for what the kernels found. */
int  sgp_cast_shapes_counters(sgp_world* w, uint32_t counters_out[2]);

/* ---- multi-GPU tiles: ghost bodies are ordinary kinematic-like bodies owned elsewhere ---- */
/* Pack the ghost record of every owned body whose AABB, inflated by `margin`, crosses outside [lo,hi). */
typedef struct sgp_ghost_record {
	float    pos[3];  float rot[4];  float lin_vel[3];  float ang_vel[3];
	int32_t  shape_type;  float shape[4];
	float    mass;  float friction;  float restitution;
	uint32_t motion_type;
	uint64_t global_id;          /* owner's local body id | owner's rank << 40 */
	/* the rest of the body's description: what an ownership migration needs to re-create the body as it was (128 bytes in all) */
	uint64_t userdata;           /* mUserData = the caller's PhysicsObject*: events and ray hits of the new owner keep reporting the same object */
	float    gravity_factor;  float linear_damping;  float angular_damping;
	uint32_t flags;              /* SGP_GHOST_FLAG_*: layer in bits 0-1, then is_sensor, allow_sleeping, use_zero_linear_drag */
	uint32_t _pad[2];
} sgp_ghost_record;
#define SGP_GHOST_FLAG_LAYER_MASK   0x3u
#define SGP_GHOST_FLAG_SENSOR       (1u << 2)
#define SGP_GHOST_FLAG_ALLOW_SLEEP  (1u << 3)
#define SGP_GHOST_FLAG_ZERO_DRAG    (1u << 4)
#define SGP_GHOST_FLAG_CHASSIS      (1u << 5)   /* the body carries a live vehicle: it never changes owner (the vehicle record -- engine, gearbox, wheel state -- lives with the tile that created it); its neighbours see it as a ghost like any other body */
int  sgp_world_export_boundary(sgp_world* w, const float lo[3], const float hi[3], float margin,
                               sgp_ghost_record* out, uint32_t cap, uint32_t* n_out);
/* Replace this world's ghost set with `n` records (bodies simulated as velocity-driven, infinite mass). */
int  sgp_world_import_ghosts(sgp_world* w, const sgp_ghost_record* in, uint32_t n);
/* Host-side routing of one tile's exported records (pure functions, no world, no device): the per-step bookkeeping of the exchange
 * in substrata_amd/tiles.py, which numpy on 100-byte records is too slow for.
 * sgp_tiles_route: `boxes` holds n_tiles x (lo xyz, hi xyz).  A record goes to every OTHER tile whose region grown by `pad` contains its
 * centre; `send_out` receives the records grouped by destination in rank order (`send_counts[r]` each; a record can appear under several
 * destinations; cap = capacity of send_out in records, exceeded -> SGP_ERR_CAPACITY).  Owned DYNAMIC bodies whose centre has left
 * boxes[my_rank] emigrate: their records carry SGP_GHOST_TAKE_OWNERSHIP in motion_type and the low 32 bits of their global ids (the
 * local body ids) are listed in `emigrant_ids`.  `rank_tag` is OR-ed into bits 40.. of every global_id. */
#define SGP_GHOST_TAKE_OWNERSHIP 0x100u
int  sgp_tiles_route(const sgp_ghost_record* recs, uint32_t n, uint32_t my_rank, const float* boxes, uint32_t n_tiles, float pad,
                     sgp_ghost_record* send_out, uint32_t cap, uint32_t* send_counts,
                     uint32_t* emigrant_ids, uint32_t emigrant_cap, uint32_t* n_emigrants);
/* sgp_tiles_split: what arrived at a tile -> ghosts (records without the flag) and immigrants (flagged records whose centre lies in
 * [lo,hi); flagged records addressed to another tile are dropped).  Both outputs need room for n records. */
int  sgp_tiles_split(const sgp_ghost_record* in, uint32_t n, const float lo[3], const float hi[3],
                     sgp_ghost_record* ghosts_out, uint32_t* n_ghosts, sgp_ghost_record* immigrants_out, uint32_t* n_immigrants);

/* ---- the exchange itself, below the C ABI (what a C++ host with one world per GPU calls once per sub-step before sgp_world_step) ----
 * The routing runs on the device (one record per (boundary body, destination tile), segmented by destination), the per-destination
 * counts are all-gathered over RCCL and the records travel device to device with grouped ncclSend / ncclRecv over xGMI; the receiving
 * tile refreshes its ghosts with a kernel while the ghost set is unchanged, and hands the records to the host (which owns the body
 * slots) only when ghosts appear / disappear or bodies migrate.  Ownership migrates with the body's full description (sgp_ghost_record).
 *
 *   rank 0:  sgp_tiles_unique_id(id)  -> the application broadcasts the 128 bytes (MPI, a socket, torch.distributed ...)
 *   all:     sgp_tiles_create(world, rank, n_tiles, boxes, margin, radius_pad, id, &tiles)        (collective: ncclCommInitRank)
 *   per step: sgp_tiles_exchange(tiles); sgp_world_step(world, dt);
 *
 * Tiles that live in ONE process (several GPUs driven by one thread, or a single-GPU dry run) are created with unique_id = NULL and
 * exchanged together with sgp_tiles_exchange_group (device-to-device copies, no communicator).
 * boxes: n_tiles x (lo xyz, hi xyz).  margin: a body whose AABB grown by it leaves the tile is exported; a record goes to every other
 * tile whose region grown by margin + radius_pad contains the body's centre (radius_pad >= the largest bounding radius). */
typedef struct sgp_tiles sgp_tiles;
#define SGP_TILES_UNIQUE_ID_BYTES 128
typedef struct sgp_tiles_stats {
	uint32_t exported;       /* records this tile produced in the last exchange (a body counts once per destination)     */
	uint32_t sent;
	uint32_t received;       /* records that arrived                                                                     */
	uint32_t ghosts;         /* ... of which ghosts                                                                      */
	uint32_t emigrated, immigrated;
	uint32_t fast_imports, slow_imports;     /* cumulative: exchanges that found the ghost set unchanged (the host saw 16 bytes per record) / whose 128-byte records had to come to the host (round 6: only sets with hull or mesh records; a changed set of primitives costs the host 32 bytes per record, and the newcomers are created on the device from the records: device_creates); the ghosts' POSES go from the received records to the bodies on the device either way */
	uint32_t route_retries;  /* exchanges in which some rank had to grow a send / emigrant / receive buffer: every rank routes again and the counts are gathered once more */
	uint32_t comm_ranks;     /* ranks ncclCommCount reports for this tile's communicator (0: no communicator, e.g. tiles of one process) */
	uint32_t exchanges;      /* sgp_tiles_exchange calls so far                                                           */
	float    comm_init_ms;   /* wall time of ncclCommInitRank                                                             */
	float    last_exchange_ms, total_exchange_ms;    /* host wall time of sgp_tiles_exchange: the last call, all calls    */
	uint32_t rebalances;     /* sgp_tiles_rebalance calls that moved this tile's region                                  */
	uint32_t device_creates; /* cumulative: ghosts and immigrants created on the device straight from the received records (no record to the host, no create command back) */
} sgp_tiles_stats;
#define SGP_MIGRATION_OUT 0
#define SGP_MIGRATION_IN  1
typedef struct sgp_migration {
	uint64_t userdata;       /* the body's user data (its PhysicsObject*): how a caller finds the object whose id changed          */
	uint32_t old_id;         /* OUT: the id it had in this world (now free).  IN: the id it had in its previous owner's world      */
	uint32_t new_id;         /* IN: its id in this world.  OUT: SGP_INVALID_ID                                                     */
	uint32_t direction;      /* SGP_MIGRATION_OUT / SGP_MIGRATION_IN                                                               */
	uint32_t peer;           /* IN: rank of the previous owner                                                                     */
} sgp_migration;
int  sgp_tiles_unique_id(uint8_t id_out[SGP_TILES_UNIQUE_ID_BYTES]);
int  sgp_tiles_create(sgp_world* w, uint32_t rank, uint32_t n_tiles, const float* boxes, float margin, float radius_pad,
                      const uint8_t* unique_id, sgp_tiles** tiles_out);
int  sgp_tiles_destroy(sgp_tiles* t);
int  sgp_tiles_exchange(sgp_tiles* t);
int  sgp_tiles_exchange_group(sgp_tiles** tiles, uint32_t n_tiles);
int  sgp_tiles_get_stats(sgp_tiles* t, sgp_tiles_stats* out);
/* Re-tiling by body count (collective; round 4).  A static split of a scene that moves leaves tiles without work -- BASELINE config 4 is a tower that
 * falls out of its upper tiles.  The grid gx x gy x gz (gx gy gz = n_tiles, tile = ix + gx (iy + gy iz), at most 4 per axis) keeps its topology; its
 * split planes move to the quantiles of where the OWNED dynamic bodies are (x planes from all bodies, the y planes of an x slab from that slab's, the z
 * planes of an (x, y) column from that column's).  Every tile computes the same planes from the same all-gathered counts; bodies then change owner
 * through the ordinary migration of the following exchanges.  sgp_tiles_rebalance: one tile per process, over the communicator;
 * sgp_tiles_rebalance_group: all tiles of one process.  sgp_tiles_get_boxes: the regions now in force (n_tiles x (lo xyz, hi xyz)).
 * by_contacts != 0: a body counts 1 + the contact constraints it was in during the last step (a tile's work is its constraints more than its bodies). */
int  sgp_tiles_rebalance(sgp_tiles* t, uint32_t gx, uint32_t gy, uint32_t gz, int by_contacts);
int  sgp_tiles_rebalance_group(sgp_tiles** tiles, uint32_t n_tiles, uint32_t gx, uint32_t gy, uint32_t gz, int by_contacts);
int  sgp_tiles_get_boxes(sgp_tiles* t, float* boxes_out);
/* Ownership changes since the last drain (both directions), oldest first; n_out = how many were pending. */
int  sgp_tiles_drain_migrations(sgp_tiles* t, sgp_migration* out, uint32_t cap, uint32_t* n_out);

/* ---- device-resident bulk access (bench / torch plumbing; pointers are HIP device pointers) ---- */
/* Raw views of the body records, valid until the world is destroyed; record i = FOUR float4 (64 bytes) at [4 i] .. [4 i + 3], of which the first two are
 * the caller's: which = 0 pose: (position xyz, inverse mass) (rotation quaternion xyzw), then two float4 of body properties; 1 velocity: (linear velocity
 * xyz, -) (angular velocity xyz, -), then two float4 that belong to the solver (the step's world-space inverse inertia). */
int  sgp_world_device_array(sgp_world* w, int which, void** dev_ptr_out, uint32_t* count_out);
/* hipStream_t the world launches on (as void*). */
int  sgp_world_stream(sgp_world* w, void** stream_out);

/* ---- world checkpoints: capture, rollback, restore (JPH::PhysicsSystem::SaveState / RestoreState with a StateRecorder) ---- */
/* A checkpoint holds everything the next step, query or getter can observe of a world (docs/CONTRACT.md, "Checkpoints"): a step is a deterministic
 * function of that state, so a world that is rolled back -- or restored into a fresh world, in this process or another -- continues bit for bit as the
 * world that was never interrupted.  Capturing has no effect on the physics.  A checkpoint is opaque, owns device and host memory and belongs to the
 * world that made it; sgp_checkpoint_write turns it into a pointer-free little-endian blob of this library's own, versioned format (no relation to
 * Jolt's PhysicsScene stream) that sgp_world_restore loads into a world just created with the same sgp_world_desc.
 * Worlds that hold ghost bodies (tiles) are refused.  Environment SGP_CHECKPOINT_FULL=1 (read at world creation): capture and rollback copy every
 * device allocation of the world whole instead of the part the next step reads -- the obviously correct statement, same bits. */
typedef struct sgp_checkpoint sgp_checkpoint;
typedef struct sgp_checkpoint_info {
	uint64_t device_bytes;          /* device memory the checkpoint holds                                                    */
	uint64_t host_bytes;            /* host memory it holds (mirrors, pending events, shape tables and pools)                */
	uint64_t blob_bytes;            /* what sgp_checkpoint_write writes                                                      */
	uint64_t world_device_bytes;    /* the world's own device allocation, for comparison                                     */
	uint64_t shape_bytes_copied;    /* shape-pool bytes the LAST capture into, or rollback from, this checkpoint moved        */
	uint32_t num_bodies, high_slot, num_cached_contacts, num_vehicles, num_meshes, num_hulls, num_compounds;
	uint32_t steps_taken;           /* steps the world had taken when it was captured                                        */
} sgp_checkpoint_info;

/* *io == NULL: creates a checkpoint; else overwrites *io in place, re-using its buffers.  Flushes pending edits first (as a step would). */
int  sgp_world_checkpoint(sgp_world* w, sgp_checkpoint** io);
/* w becomes exactly what it was at the capture: bodies, contact cache, vehicles, shapes, pending events, ids handed out afterwards.
 * SGP_ERR_INVALID (world untouched) for a checkpoint made by another world.  A runtime failure on the way (SGP_ERR_HIP) leaves the world undefined:
 * destroy it. */
int  sgp_world_rollback(sgp_world* w, const sgp_checkpoint* cp);
int  sgp_checkpoint_destroy(sgp_checkpoint* cp);      /* NULL: SGP_OK */
int  sgp_checkpoint_get_info(const sgp_checkpoint* cp, sgp_checkpoint_info* out);
/* out == NULL or cap too small: only *bytes_out is set (SGP_ERR_CAPACITY when out was given).  A checkpoint may outlive its world (get_info and destroy
 * still work); writing it needs the world: SGP_ERR_INVALID once the world has been destroyed. */
int  sgp_checkpoint_write(const sgp_checkpoint* cp, void* out, uint64_t cap, uint64_t* bytes_out);
/* Into a world in which no body or shape has ever been created and whose desc equals the blob's; anything else, and every malformed blob
 * (truncated, wrong magic or version, sizes that do not add up), is SGP_ERR_INVALID with the world untouched.  SGP_ERR_HIP (an allocation or a copy
 * failed half way) leaves the world undefined: destroy it. */
int  sgp_world_restore(sgp_world* fresh, const void* blob, uint64_t bytes);
/* Validates a blob and reads its counts.  Host only: needs no device. */
int  sgp_checkpoint_blob_info(const void* blob, uint64_t bytes, sgp_checkpoint_info* out);

/* ---- batch checkpoints: capture and rollback of sgp_characters, sgp_particles, sgp_crafts and sgp_movers ---- */
/* A world checkpoint holds nothing of the world's batches; these pairs do, by the world's rule (docs/CONTRACT.md, "Batch checkpoints"): after
 * sgp_world_rollback and one rollback per batch, each to the checkpoint taken at the same moment, in any order and with no update or step in
 * between, the whole scene continues bit for bit as one that was never interrupted.  The pairing is the caller's: world_steps_taken is there to
 * check it.  A batch checkpoint is opaque, owns device and host memory, belongs to the batch that made it and may outlive it and its world
 * (get_info and destroy still work).  There is no blob, and no restoring into a fresh batch.
 *
 * Capture: *io == NULL creates a checkpoint, else *io is overwritten in place and its buffers are re-used (device_bytes grows only when the
 * batch's high-water slot did; for particles, the host's bound of the live count).  Host edits that no update has carried yet go to the device
 * first; the copy is enqueued on the world's stream and the call returns without waiting for it.  It changes nothing any later call returns.
 * Rollback: the batch becomes exactly what it was at the capture -- the device's state (for particles: the live ones, their count, the
 * replacement cursor, undrained events and the dropped count; for characters: undrained contact and push records, the drives and the drive states with a pending jump too), the host's records and
 * inputs, tags, the movers' paths with their reference counts, and the slot tables with the free list's order, so that the next *_add returns
 * the id it would have.  Not touched: which particle batch a craft batch is attached to.
 * A craft or mover that was attached to its body at the capture is attached to the same body id again if that is now a live body the batch
 * could be added on (whatever happened to it in between -- the world's rollback brings a removed body back), and BODY_GONE from the next
 * update on otherwise; one that was BODY_GONE at the capture stays so.
 * SGP_ERR_INVALID, with the batch untouched: NULL, a checkpoint of another batch or kind, a batch whose world is gone, a world that holds ghost
 * bodies. */
#define SGP_BATCH_CHARACTERS 1u
#define SGP_BATCH_PARTICLES  2u
#define SGP_BATCH_CRAFTS     3u
#define SGP_BATCH_MOVERS     4u
typedef struct sgp_batch_checkpoint sgp_batch_checkpoint;
typedef struct sgp_batch_checkpoint_info {
	uint64_t device_bytes, host_bytes;   /* what the checkpoint holds                                                             */
	uint32_t kind;                       /* SGP_BATCH_*                                                                           */
	uint32_t capacity, high_slot, num_alive;      /* of the batch at the capture (particles: high_slot and num_alive are the host's bound of the live count) */
	uint32_t world_steps_taken;          /* steps the batch's world had taken at the capture: lets a caller check the pairing     */
	uint32_t pad_;
} sgp_batch_checkpoint_info;
int  sgp_characters_checkpoint(sgp_characters* cs, sgp_batch_checkpoint** io);
int  sgp_characters_rollback(sgp_characters* cs, const sgp_batch_checkpoint* cp);
int  sgp_particles_checkpoint(sgp_particles* ps, sgp_batch_checkpoint** io);
int  sgp_particles_rollback(sgp_particles* ps, const sgp_batch_checkpoint* cp);
int  sgp_crafts_checkpoint(sgp_crafts* cs, sgp_batch_checkpoint** io);
int  sgp_crafts_rollback(sgp_crafts* cs, const sgp_batch_checkpoint* cp);
int  sgp_movers_checkpoint(sgp_movers* ms, sgp_batch_checkpoint** io);
int  sgp_movers_rollback(sgp_movers* ms, const sgp_batch_checkpoint* cp);
int  sgp_batch_checkpoint_destroy(sgp_batch_checkpoint* cp);      /* NULL: SGP_OK */
int  sgp_batch_checkpoint_get_info(const sgp_batch_checkpoint* cp, sgp_batch_checkpoint_info* out);

/* ---- batched proximity and zone watchers (ScriptedObjectProximityChecker, the parcel enter / exit events of GUIClient) ----
 * A batch of watched objects, up to SGP_PROX_MAX_OBSERVERS observers and a table of zones (parcels) that belongs to one world and lives on
 * the device.  sgp_proximity_update runs ScriptedObjectProximityChecker::think (ScriptedObjectProximityChecker.cpp:40-90) for every observer
 * against every watched object, a lane per object, on the bounds the last step or edit flush left in the world (the PHYSICS body's AABB), and
 * the parcel bookkeeping of GUIClient.cpp:6874-6968 for every observer: which zone it stands in, and for the objects whose centroid lies in
 * the zone it left or entered an EXITED or ENTERED event.  The near bit of every (object, observer) pair and every observer's zone stay on
 * the device between updates; only transitions become events.  The arithmetic is written out in docs/CONTRACT.md 4l.  Departures from the
 * reference: docs/GAPS.md ("Proximity watchers").  A world checkpoint holds nothing of a batch (sgp_proximity_checkpoint / _rollback do, by
 * the rule of the batch checkpoints above, with SGP_BATCH_PROXIMITY); tiled worlds are refused. */
typedef struct sgp_proximity sgp_proximity;
#define SGP_BATCH_PROXIMITY 5u
#define SGP_PROX_MAX_OBSERVERS 32
#define SGP_PROXIMITY_MAX_OBJECTS (1u << 20)
#define SGP_PROXIMITY_MAX_ZONES   (1u << 12)
#define SGP_PROX_WANT_NEAR 1u         /* onUserMovedNearToObject / onUserMovedAwayFromObject are wanted                        */
#define SGP_PROX_WANT_ZONE 2u         /* onUserEnteredParcel / onUserExitedParcel are wanted                                   */
#define SGP_PROX_OBS_POINT 0u         /* the observer is where the host puts it                                                */
#define SGP_PROX_OBS_BODY  1u         /* the observer is a body's position plus a world-space offset, read on the device       */
#define SGP_PROX_ST_BODY_GONE 1u      /* the body is no longer the one the object was added on: the object is skipped          */
#define SGP_PROX_OBS_ST_BODY_GONE 1u  /* a body-sourced observer whose body has gone: it is no longer updated and fires nothing */
#define SGP_PROX_EV_NEAR    1u        /* onUserMovedNearToObject                                                               */
#define SGP_PROX_EV_AWAY    2u        /* onUserMovedAwayFromObject                                                             */
#define SGP_PROX_EV_EXITED  3u        /* onUserExitedParcel (object == SGP_INVALID_ID: the observer left the zone)             */
#define SGP_PROX_EV_ENTERED 4u        /* onUserEnteredParcel (object == SGP_INVALID_ID: UserEnteredParcelMessage)              */
typedef struct sgp_proximity_object {
	uint32_t body;                 /* a live body of any motion type: no compound, ghost or alias slot, no other object of the batch on it */
	float    radius;               /* finite, > 0 (the reference: 20)                                                   */
	uint32_t flags;                /* SGP_PROX_WANT_*                                                                   */
	uint32_t reserved_;
	uint64_t tag;                  /* the caller's WorldObject*: not interpreted, reported with every event              */
} sgp_proximity_object;
typedef struct sgp_proximity_observer {
	uint32_t source;               /* SGP_PROX_OBS_POINT | SGP_PROX_OBS_BODY                                            */
	uint32_t body;                 /* BODY: a live body (no compound, ghost or alias slot)                              */
	float    pos[3];               /* POINT: where the observer is                                                      */
	float    offset[3];            /* BODY: added to the body's position, in world space                                */
} sgp_proximity_observer;
typedef struct sgp_proximity_event {
	uint32_t kind;                 /* SGP_PROX_EV_*                                                                     */
	uint32_t object;               /* the object's id, or SGP_INVALID_ID in an observer-level zone record               */
	uint32_t observer;
	uint32_t zone_key;             /* EXITED / ENTERED: the zone's key; else SGP_INVALID_ID                             */
	uint64_t tag;                  /* the object's (0 in an observer-level record)                                      */
	uint32_t update_index;         /* the update of the batch that raised it, counted from 0                            */
	uint32_t reserved_;
} sgp_proximity_event;
typedef struct sgp_proximity_state {
	uint32_t status;               /* SGP_PROX_ST_*                                                                     */
	uint32_t near_mask;            /* bit k: observer k was within the radius at the last update that tested it         */
} sgp_proximity_state;
typedef struct sgp_proximity_observer_state {
	float    pos[3];               /* where the last update found the observer                                          */
	uint32_t zone_key;             /* the zone it stands in, or SGP_INVALID_ID                                          */
	uint32_t update_index;         /* updates this observer has run                                                     */
	uint32_t status;               /* SGP_PROX_OBS_ST_*                                                                 */
} sgp_proximity_observer_state;
/* object_capacity in 1 .. SGP_PROXIMITY_MAX_OBJECTS, zone_capacity in 1 .. SGP_PROXIMITY_MAX_ZONES, event_capacity >= 1: event records the
 * batch holds between two drains.  SGP_ERR_INVALID for a world that holds ghost bodies. */
int  sgp_proximity_create(sgp_world* w, uint32_t object_capacity, uint32_t zone_capacity, uint32_t event_capacity, sgp_proximity** out);
/* After sgp_world_destroy of its world this still frees the batch and returns SGP_OK; every other call on such a batch is SGP_ERR_INVALID. */
int  sgp_proximity_destroy(sgp_proximity* pb);
/* n objects at once, all or none: ids_out[i] is the id of descs[i].  A new object is near nobody.  SGP_ERR_INVALID, with nothing added, for a
 * radius that is not finite and > 0, an unknown flag, a body that does not qualify, carries an object of the batch already or is named
 * twice; SGP_ERR_CAPACITY when the n do not all fit. */
int  sgp_proximity_add(sgp_proximity* pb, const sgp_proximity_object* descs, uint32_t n, uint32_t* ids_out);
int  sgp_proximity_remove(sgp_proximity* pb, uint32_t id);      /* fires nothing */
/* The want flags of a live object.  The near mask is not touched: a transition that passed while the flag was off is not replayed. */
int  sgp_proximity_set_flags(sgp_proximity* pb, uint32_t id, uint32_t flags);
/* Observer k < SGP_PROX_MAX_OBSERVERS.  A slot that held no observer gets a NEW one: near nothing and in no zone, so that its first update
 * fires NEAR for everything in range and ENTERED for its zone (in_script_proximity = false, an invalid cur_in_parcel_id).  On a slot that
 * holds one, only the source changes.  SGP_ERR_INVALID for a non-finite value, an unknown source, a body that does not qualify. */
int  sgp_proximity_set_observer(sgp_proximity* pb, uint32_t k, const sgp_proximity_observer* obs);
/* Moves POINT observers first .. first + n - 1 (all must be live POINT observers): a host write, uploaded by the next update. */
int  sgp_proximity_set_points(sgp_proximity* pb, uint32_t first, uint32_t n, const float* xyz);
/* Clears the observer's bit in every near mask and forgets its zone; fires no events. */
int  sgp_proximity_remove_observer(sgp_proximity* pb, uint32_t k);
/* Bounds are fp32, mn <= mx and finite; `key` is unique among the live zones (the ParcelID: among the zones that contain a point the lowest
 * key wins).  A zone slot carries a generation: an observer that stood in a removed zone sees it as gone even when the slot is refilled. */
int  sgp_proximity_zone_add(sgp_proximity* pb, const float mn[3], const float mx[3], uint32_t key, uint32_t* zone_id_out);
int  sgp_proximity_zone_remove(sgp_proximity* pb, uint32_t zone_id);
/* One update: flushes pending body edits, uploads what the host changed and enqueues four launches on the world's stream -- no wait, no copy
 * to the host, no allocation.  Nothing is launched while the batch has no live object or no live observer.  No body and nothing a step
 * reads is altered. */
int  sgp_proximity_update(sgp_proximity* pb);
/* The events since the last drain in the order of the updates that raised them; within one update first the observer-level zone records by
 * ascending observer, EXITED before ENTERED, then the objects' events by ascending object id, then ascending observer, then kind (NEAR or
 * AWAY, EXITED, ENTERED).  Waits.  *n_out = records held (<= cap are written; all are consumed), *n_dropped = events that did not fit
 * event_capacity since the last drain: always the LAST of that order. */
int  sgp_proximity_drain_events(sgp_proximity* pb, sgp_proximity_event* out, uint32_t cap, uint32_t* n_out, uint32_t* n_dropped);
/* Waits for the updates in flight.  Slots that are not live read as zeroes. */
int  sgp_proximity_get_states(sgp_proximity* pb, uint32_t first, uint32_t n, sgp_proximity_state* out);
int  sgp_proximity_get_observers(sgp_proximity* pb, uint32_t first, uint32_t n, sgp_proximity_observer_state* out);
int  sgp_proximity_checkpoint(sgp_proximity* pb, sgp_batch_checkpoint** io);
int  sgp_proximity_rollback(sgp_proximity* pb, const sgp_batch_checkpoint* cp);
/* The arithmetic of an update on the host, bit-equal to the device (no world, no device).  test_point: closest point of the box [mn, mx] to p,
 * *dist2_out = the squared distance, *near_out = dist2 < radius * radius.  pick_zone: `current` (an index < n, or SGP_INVALID_ID) stays if it is
 * live and contains p; else the live zone of the lowest key that contains p; else SGP_INVALID_ID.  mins / maxs: n * 3 floats; live: n words. */
int  sgp_proximity_test_point(const float mn[3], const float mx[3], const float p[3], float radius, uint32_t* near_out, float* dist2_out);
int  sgp_proximity_pick_zone(const float* mins, const float* maxs, const uint32_t* keys, const uint32_t* live, uint32_t n, uint32_t current, const float p[3], uint32_t* zone_out);

/* ---- batched audio sources: range, occlusion, muting (the two audio walks of GUIClient) ----
 * A batch of audio sources and up to SGP_AUD_MAX_LISTENERS listeners that belongs to one world and lives on the device.  sgp_audibility_update
 * runs, for every (source, listener) pair, the range walk of GUIClient.cpp:4512-4543 (checkForAudioRangeChanges) and, for the pairs in range,
 * the occlusion and muting walk of GUIClient.cpp:6973-7034: one any-hit ray from the listener towards the source (sgp_raycast_any's search) and
 * the mute ramp of AudioSource::startMuting / startUnmuting / updateCurrentMuteVolumeFactor (audio/AudioEngine.cpp:79-121).  Per pair the range
 * bit, the occlusion bit, the five ramp variables and the last distance stay on the device between updates; only transitions become events.
 * The arithmetic is written out in docs/CONTRACT.md 4m.  What is left out: docs/GAPS.md ("Audio sources").  A world checkpoint holds nothing
 * of a batch (sgp_audibility_checkpoint / _rollback do, by the rule of the batch checkpoints above, with SGP_BATCH_AUDIBILITY); tiled worlds
 * are refused. */
typedef struct sgp_audibility sgp_audibility;
#define SGP_BATCH_AUDIBILITY 6u
#define SGP_AUD_MAX_LISTENERS 32
#define SGP_AUDIBILITY_MAX_SOURCES (1u << 20)
#define SGP_AUDIBILITY_MAX_PAIRS   (1u << 22)     /* source_capacity * listener_capacity                                                 */
#define SGP_AUD_SRC_POINT 0u          /* the source is where the host puts it                                                  */
#define SGP_AUD_SRC_BODY  1u          /* the source is the centroid of a body's world AABB (getCentroidWS), read on the device */
#define SGP_AUD_LST_POINT 0u          /* the listener is where the host puts it                                                */
#define SGP_AUD_LST_BODY  1u          /* the listener is a body's position plus a world-space offset, read on the device       */
#define SGP_AUD_ONE_SHOT       1u     /* SourceType_NonStreaming && !looping: never muted (GUIClient.cpp:7010-7011)            */
#define SGP_AUD_WANT_RANGE     2u     /* IN_RANGE / OUT_OF_RANGE are wanted                                                    */
#define SGP_AUD_WANT_OCCLUSION 4u     /* OCCLUDED / UNOCCLUDED are wanted (sourceNumOcclusionsUpdated where the number changed) */
#define SGP_AUD_WANT_VOLUME    8u     /* VOLUME is wanted (sourceVolumeUpdated)                                                */
#define SGP_AUD_ST_BODY_GONE 1u       /* the body is no longer the one the source was added on: the source is frozen           */
#define SGP_AUD_LST_ST_BODY_GONE 1u   /* a body-sourced listener whose body has gone: its pairs are frozen                     */
#define SGP_AUD_EV_IN_RANGE     1u
#define SGP_AUD_EV_OUT_OF_RANGE 2u
#define SGP_AUD_EV_OCCLUDED     3u
#define SGP_AUD_EV_UNOCCLUDED   4u
#define SGP_AUD_EV_VOLUME       5u
#define SGP_AUD_PAIR_IN_RANGE 1u      /* sgp_audibility_pair_state::bits                                                       */
#define SGP_AUD_PAIR_OCCLUDED 2u
typedef struct sgp_audibility_source {
	uint32_t kind;                 /* SGP_AUD_SRC_POINT | SGP_AUD_SRC_BODY                                              */
	uint32_t body;                 /* BODY: a live body (no compound, ghost or alias slot, no other source of the batch on it) */
	float    pos[3];               /* POINT: where the source is                                                        */
	float    volume;               /* finite, >= 0: audible up to 60 * volume metres                                    */
	uint32_t zone_key;             /* AudioSource::userdata_1, the parcel the source belongs to; SGP_INVALID_ID: none   */
	uint32_t flags;                /* SGP_AUD_ONE_SHOT | SGP_AUD_WANT_*                                                 */
	uint64_t tag;                  /* the caller's AudioSource*: not interpreted, reported with every event             */
} sgp_audibility_source;
typedef struct sgp_audibility_listener {
	uint32_t source;               /* SGP_AUD_LST_POINT | SGP_AUD_LST_BODY                                              */
	uint32_t body;                 /* BODY: a live body (no compound, ghost or alias slot)                              */
	float    pos[3];               /* POINT: where the listener is                                                      */
	float    offset[3];            /* BODY: added to the body's position, in world space                                */
	uint32_t ignore_body;          /* the rays' ignore_id; SGP_INVALID_ID: nothing (the reference ignores nothing)      */
	uint32_t zone_key;             /* the parcel the listener stands in, SGP_INVALID_ID: none (a proximity batch attached: taken from its observer) */
	uint32_t mute_outside;         /* that parcel has MUTE_OUTSIDE_AUDIO_FLAG (a proximity batch attached: looked up in the muting keys) */
	uint32_t reserved_;
} sgp_audibility_listener;
typedef struct sgp_audibility_event {
	uint32_t kind;                 /* SGP_AUD_EV_*                                                                      */
	uint32_t source;               /* the source's id                                                                   */
	uint32_t listener;
	float    factor;               /* VOLUME: the pair's new mute_volume_factor; else 0                                 */
	uint64_t tag;                  /* the source's                                                                      */
	uint32_t update_index;         /* the update of the batch that raised it, counted from 0                            */
	uint32_t reserved_;
} sgp_audibility_event;
typedef struct sgp_audibility_state {
	uint32_t status;               /* SGP_AUD_ST_*                                                                      */
	float    pos[3];               /* the position the last update used                                                 */
	uint32_t in_range_mask;        /* bit l: in audio range of listener l (in_audio_proximity)                          */
	uint32_t occluded_mask;        /* bit l: num_occlusions == 1 for listener l                                         */
} sgp_audibility_state;
typedef struct sgp_audibility_pair_state {
	uint32_t bits;                 /* SGP_AUD_PAIR_*                                                                    */
	float    mute_volume_factor;   /* 1 until the pair's ramp has run                                                   */
	float    dist;                 /* of the last update that traced the pair; 0 before                                 */
} sgp_audibility_pair_state;
typedef struct sgp_audibility_listener_state {
	float    pos[3];               /* where the last update found the listener                                          */
	uint32_t zone_key;             /* the key it used                                                                   */
	uint32_t mute_outside;
	uint32_t update_index;         /* updates this listener has run                                                     */
	uint32_t status;               /* SGP_AUD_LST_ST_*                                                                  */
} sgp_audibility_listener_state;
typedef struct sgp_audibility_ramp {      /* the five ramp variables of AudioSource (AudioEngine.h:136-140)            */
	double   mute_change_start_time;
	double   mute_change_end_time;
	float    mute_volume_factor;
	float    mute_vol_fac_start;
	float    mute_vol_fac_end;
	uint32_t reserved_;
} sgp_audibility_ramp;
/* source_capacity in 1 .. SGP_AUDIBILITY_MAX_SOURCES, listener_capacity in 1 .. SGP_AUD_MAX_LISTENERS, their product at most
 * SGP_AUDIBILITY_MAX_PAIRS, event_capacity >= 1: event records the batch holds between two drains.  SGP_ERR_INVALID for a world that holds
 * ghost bodies. */
int  sgp_audibility_create(sgp_world* w, uint32_t source_capacity, uint32_t listener_capacity, uint32_t event_capacity, sgp_audibility** out);
/* After sgp_world_destroy of its world this still frees the batch and returns SGP_OK; every other call on such a batch is SGP_ERR_INVALID. */
int  sgp_audibility_destroy(sgp_audibility* ab);
/* n sources at once, all or none: ids_out[i] is the id of descs[i].  A new source starts as AudioSource's constructor leaves it, for every
 * listener: out of range, not occluded, factor 1, start time -2, end time -1, start and end factor 1.  SGP_ERR_INVALID, with nothing added,
 * for an unknown kind or flag, a volume or position that is not finite (or a volume < 0), a body that does not qualify, carries a source of
 * the batch already or is named twice; SGP_ERR_CAPACITY when the n do not all fit. */
int  sgp_audibility_add(sgp_audibility* ab, const sgp_audibility_source* descs, uint32_t n, uint32_t* ids_out);
int  sgp_audibility_remove(sgp_audibility* ab, uint32_t id);      /* fires nothing */
/* Moves POINT sources first .. first + n - 1 (all must be live POINT sources): a host write, uploaded by the next update. */
int  sgp_audibility_set_points(sgp_audibility* ab, uint32_t first, uint32_t n, const float* xyz);
int  sgp_audibility_set_volume(sgp_audibility* ab, uint32_t id, float volume);
/* SGP_AUD_ONE_SHOT | SGP_AUD_WANT_* of a live source.  The pairs' state is not touched: a transition that passed while a flag was off is not replayed. */
int  sgp_audibility_set_flags(sgp_audibility* ab, uint32_t id, uint32_t flags);
/* Listener k < listener_capacity.  A slot that held no listener gets a NEW one: every pair of it starts as the constructor leaves it.  On a
 * slot that holds one, everything but the pairs' state changes.  SGP_ERR_INVALID for a non-finite value, an unknown source, a body that does
 * not qualify. */
int  sgp_audibility_set_listener(sgp_audibility* ab, uint32_t k, const sgp_audibility_listener* in);
/* Forgets every pair of the listener; fires no events. */
int  sgp_audibility_remove_listener(sgp_audibility* ab, uint32_t k);
/* Moves POINT listeners first .. first + n - 1 (all must be live POINT listeners). */
int  sgp_audibility_set_listener_points(sgp_audibility* ab, uint32_t first, uint32_t n, const float* xyz);
/* The parcel listener k stands in and whether it mutes outside audio: what holds while no proximity batch is attached. */
int  sgp_audibility_set_listener_zone(sgp_audibility* ab, uint32_t k, uint32_t zone_key, uint32_t mute_outside);
/* The transition period of startMuting / startUnmuting in seconds, finite and >= 0 (the reference passes 1, the default). */
int  sgp_audibility_set_transition(sgp_audibility* ab, double seconds);
/* With a proximity batch of the same world attached, listener k takes its zone_key on the device from observer k of that batch -- the key its
 * last launched update left (SGP_INVALID_ID while that observer has run no update) -- and mute_outside is "the key is one of the muting keys".
 * Both batches enqueue on the world's stream: enqueue order is the order.  NULL detaches; destroying an attached proximity batch is the
 * caller's error.  Configuration: not part of a batch checkpoint, like the muting keys. */
int  sgp_audibility_attach_proximity(sgp_audibility* ab, sgp_proximity* pb_or_null);
/* The zone keys whose parcel has MUTE_OUTSIDE_AUDIO_FLAG: strictly ascending, none SGP_INVALID_ID, at most SGP_PROXIMITY_MAX_ZONES. */
int  sgp_audibility_set_muting_keys(sgp_audibility* ab, const uint32_t* keys, uint32_t n);
/* One update at the caller's clock `cur_time` (finite): flushes pending body edits, makes the query grid valid, uploads what the host
 * changed and enqueues eight launches on the world's stream -- no wait, no copy to the host, no allocation.  Nothing is launched, and the
 * update index stays, while the batch has no live source or no live listener.  No body and nothing a step reads is altered. */
int  sgp_audibility_update(sgp_audibility* ab, double cur_time);
/* The events since the last drain in the order of the updates that raised them; within one update by ascending source id, then ascending
 * listener, then kind: IN_RANGE or OUT_OF_RANGE, OCCLUDED or UNOCCLUDED, VOLUME.  Waits.  *n_out = records held (<= cap are written; all are
 * consumed), *n_dropped = events that did not fit event_capacity since the last drain: always the LAST of that order. */
int  sgp_audibility_drain_events(sgp_audibility* ab, sgp_audibility_event* out, uint32_t cap, uint32_t* n_out, uint32_t* n_dropped);
/* Wait for the updates in flight.  Slots that are not live read as zeroes.  get_pair_states: n sources from `first`, listener_capacity
 * records each (source-major); a pair without a live listener or source reads as bits 0, factor 1, dist 0. */
int  sgp_audibility_get_states(sgp_audibility* ab, uint32_t first, uint32_t n, sgp_audibility_state* out);
int  sgp_audibility_get_pair_states(sgp_audibility* ab, uint32_t first, uint32_t n, sgp_audibility_pair_state* out);
int  sgp_audibility_get_listeners(sgp_audibility* ab, uint32_t first, uint32_t n, sgp_audibility_listener_state* out);
int  sgp_audibility_checkpoint(sgp_audibility* ab, sgp_batch_checkpoint** io);
int  sgp_audibility_rollback(sgp_audibility* ab, const sgp_batch_checkpoint* cp);
/* The arithmetic of an update on the host, bit-equal to the device (no world, no device; CONTRACT 4m steps 1-3).  pair_ray: one pair's range
 * decision from `in_range_before` and, where the pair is traced (*traced_out = 1), its distance, unit direction and trace length (else those
 * three are 0).  ramp_step: startMuting (mute != 0) or startUnmuting, then updateCurrentMuteVolumeFactor; *changed_out = the factor changed. */
int  sgp_audibility_pair_ray(const float source_pos[3], const float listener_pos[3], float volume, uint32_t in_range_before,
                             uint32_t* in_range_out, uint32_t* traced_out, float* dist_out, float dir_out[3], float* trace_out);
int  sgp_audibility_ramp_step(sgp_audibility_ramp* io, uint32_t mute, double cur_time, double transition, uint32_t* changed_out);

#ifdef __cplusplus
}
#endif
#endif /* SGP_H */
