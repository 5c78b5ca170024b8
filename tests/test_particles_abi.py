"""CPU-side checks of the batched particle system's entry points (include/sgp.h, "batched point particles"): declared, exported and prototyped, the three
structs have the library's sizes under NEW indices of sgp_abi_sizeof and their fields sit where the header puts them, the defaults are those of the
reference's Particle(), NULL handles and bad capacities are refused, there is no batch without a device, and the facade header compiles.  No device."""
import ctypes as C
import os
import re
import subprocess

import pytest

from substrata_amd import abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = [("sgp_particle", abi.Particle, 64), ("sgp_particle_state", abi.ParticleState, 48), ("sgp_particle_event", abi.ParticleEvent, 32)]
FUNCTIONS = ["default_particle", "particles_create", "particles_destroy", "particles_add", "particles_update", "particles_read",
             "particles_drain_events", "particles_clear"]
SIZES = {"float": 4, "int32_t": 4, "uint32_t": 4, "uint64_t": 8}


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(build.build())
    abi.bind(lib, "sgp_")
    return lib


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgp.h")).read(), flags=re.S)


def header_fields(struct):
    """(name, C type, array length) of the members of `typedef struct <struct> { ... }`, in order."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header(), flags=re.S).group(1)
    out = []
    for ctype, names in re.findall(r"(float|int32_t|uint32_t|uint64_t)\s+([^;]+);", body):
        for nm in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", nm)
            out.append((m.group(1), ctype, int(m.group(2) or 1)))
    return out


@pytest.mark.parametrize("struct, mirror, size", STRUCTS)
def test_field_offsets_follow_the_header(struct, mirror, size):
    fields = header_fields(struct)
    assert [f[0] for f in fields] == [n for n, _ in mirror._fields_]
    off = 0
    for name, ctype, count in fields:
        a = SIZES[ctype]
        off = (off + a - 1) // a * a
        assert getattr(mirror, name).offset == off and getattr(mirror, name).size == a * count, name
        off += a * count
    align = max(SIZES[f[1]] for f in fields)
    assert C.sizeof(mirror) == (off + align - 1) // align * align == size


def test_declared_exported_and_prototyped(lib):
    h = header()
    for name in FUNCTIONS:
        assert re.search(r"\bsgp_%s\s*\(" % name, h), name
        assert hasattr(lib, "sgp_" + name) and name in abi.PROTOTYPES, name
    for macro, value in (("SGP_PARTICLE_DIE_ON_HIT", abi.PARTICLE_DIE_ON_HIT), ("SGP_PARTICLE_EV_DIED", abi.PARTICLE_EV_DIED),
                         ("SGP_PARTICLE_EV_FOAM", abi.PARTICLE_EV_FOAM), ("SGP_PARTICLE_EV_REPLACED", abi.PARTICLE_EV_REPLACED)):
        assert re.search(r"#define %s\s+%du" % (macro, value), h), macro
    assert re.search(r"#define SGP_PARTICLES_MAX_CAPACITY\s+\(1u << 20\)", h) and abi.PARTICLES_MAX_CAPACITY == 1 << 20


def test_structs_have_the_library_sizes_under_new_indices(lib):
    idx = [abi.ABI_SIZEOF_ALL.index(s) for s, _, _ in STRUCTS]
    assert idx == [30, 31, 32]                     # (29 answers -1 for good, as 21 and 24 do: the end of the list as earlier bindings probe it)
    assert lib.sgp_abi_sizeof(29) == -1 and lib.sgp_abi_sizeof(33) == -1
    for (struct, mirror, size), i in zip(STRUCTS, idx):
        assert lib.sgp_abi_sizeof(i) == C.sizeof(mirror) == C.sizeof(abi.STRUCTS[struct]) == size, struct
    for k, name in enumerate(abi.ABI_SIZEOF_ALL):      # nothing that was there before moved
        assert lib.sgp_abi_sizeof(k) == (C.sizeof(abi.STRUCTS[name]) if name is not None else -1), (k, name)
    assert lib.sgp_abi_version() == 1 == abi.ABI_VERSION
    assert (abi.particle_dtype.itemsize, abi.particle_state_dtype.itemsize, abi.particle_event_dtype.itemsize) == (64, 48, 32)


def test_defaults_are_those_of_the_reference_particle(lib):
    """Particle() (ParticleManager.h:35-36): restitution 0.5, width 1, dwidth_dt 0.5, cur_opacity 1, dopacity_dt -0.3, mass 1e-6, area 1e-6, die_when_hit_surface false."""
    f32 = lambda x: C.c_float(x).value
    p = abi.Particle()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    lib.sgp_default_particle(C.byref(p))
    lib.sgp_default_particle(None)      # (returns)
    assert (p.restitution, p.width, p.dwidth_dt, p.opacity, p.dopacity_dt) == (0.5, 1.0, 0.5, 1.0, f32(-0.3))
    assert (p.mass, p.area) == (f32(1.0e-6), f32(1.0e-6))
    assert tuple(p.pos) == (0.0, 0.0, 0.0) and tuple(p.vel) == (0.0, 0.0, 0.0) and p.flags == 0 and p.tag == 0
    # ... and the facade's Particle says the same
    src = open(os.path.join(ROOT, "substrata_amd", "shim", "ParticleBatch.h")).read()
    for text in ("restitution(0.5f)", "width(1.f)", "dwidth_dt(0.5f)", "cur_opacity(1.f)", "dopacity_dt(-0.3f)", "mass(1.0e-6f)", "area(1.0e-6f)", "die_when_hit_surface(false)"):
        assert text in src, text


def test_null_handles_and_bad_capacities_are_refused(lib):
    h = C.c_void_p()
    n, nd = C.c_uint32(0), C.c_uint32(0)
    p = abi.Particle()
    lib.sgp_default_particle(C.byref(p))
    fake_world = C.c_void_p(0)
    assert lib.sgp_particles_create(fake_world, 16, 16, C.byref(h)) == abi.ERR_INVALID and not h.value
    assert b"sgp_particles_create" in lib.sgp_last_error()
    assert lib.sgp_particles_destroy(None) == abi.ERR_INVALID
    assert lib.sgp_particles_add(None, C.byref(p), 1) == abi.ERR_INVALID
    assert lib.sgp_particles_update(None, 1.0 / 60.0) == abi.ERR_INVALID
    assert b"sgp_particles_update" in lib.sgp_last_error()
    assert lib.sgp_particles_read(None, None, 0, C.byref(n)) == abi.ERR_INVALID
    assert lib.sgp_particles_drain_events(None, None, 0, C.byref(n), C.byref(nd)) == abi.ERR_INVALID
    assert lib.sgp_particles_clear(None) == abi.ERR_INVALID
    # capacity 0 and capacity beyond 2^20 are refused before the world is looked at (the argument check is one condition: sgp_world_particles.hip)
    src = open(os.path.join(ROOT, "substrata_amd", "csrc", "sgp_world_particles.hip")).read()
    assert "if (!w || !out || capacity == 0 || capacity > SGP_PARTICLES_MAX_CAPACITY) return fail(SGP_ERR_INVALID" in src
    for cap in (0, (1 << 20) + 1):
        assert lib.sgp_particles_create(fake_world, cap, 16, C.byref(h)) == abi.ERR_INVALID and not h.value


def test_no_batch_without_a_device(lib):
    """Without a GPU there is no world to own a batch: sgp_world_create says SGP_ERR_NO_DEVICE, and the Python wrapper raises."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    d = abi.WorldDesc()
    lib.sgp_default_world_desc(C.byref(d))
    w = C.c_void_p()
    assert lib.sgp_world_create(C.byref(d), C.byref(w)) == abi.ERR_NO_DEVICE and not w.value
    assert b"no CPU fallback" in lib.sgp_last_error()
    from substrata_amd import lib as product
    from substrata_amd.world import SgpError
    with pytest.raises(SgpError):
        product.World(max_bodies=16).particles(16)


def test_facade_header_compiles():
    """shim/ParticleBatch.h on its own, as a caller would include it."""
    shim = os.path.join(ROOT, "substrata_amd", "shim")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", shim, "-x", "c++", os.path.join(shim, "ParticleBatch.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_caller_program_compiles(tmp_path):
    from test_facade_gpu import build_facade_exe
    assert os.path.exists(build_facade_exe(tmp_path, "particles_batch.cpp"))
