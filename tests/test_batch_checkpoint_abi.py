"""CPU-side checks of the batch checkpoint entry points (include/sgp.h, "batch checkpoints"): declared, exported and prototyped, the info struct has the
library's size under a NEW index of sgp_abi_sizeof with nothing before it moved, its fields sit where the header puts them, and NULL handles are refused
without touching the HIP runtime.  No world exists here (no device)."""
import ctypes as C
import os
import re

import pytest

from substrata_amd import abi, build, world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = ["characters", "particles", "crafts", "movers"]
NAMES = [f"{b}_{op}" for b in BATCHES for op in ("checkpoint", "rollback")] + ["batch_checkpoint_destroy", "batch_checkpoint_get_info"]


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(build.build())
    abi.bind(lib, "sgp_")
    lib.sgp_abi_sizeof.restype = C.c_int
    return lib


def test_symbols_declared_exported_and_prototyped(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgp.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\bsgp_%s\s*\(" % n, header), f"include/sgp.h does not declare sgp_{n}"
        assert hasattr(lib, "sgp_" + n), f"libsgp.so does not export sgp_{n}"
        assert n in abi.PROTOTYPES, f"abi.PROTOTYPES lacks {n}"
        assert getattr(lib, "sgp_" + n).argtypes is not None
    for kind, name in enumerate(["CHARACTERS", "PARTICLES", "CRAFTS", "MOVERS"], start=1):
        assert re.search(r"#define\s+SGP_BATCH_%s\s+%du\b" % (name, kind), header) and getattr(abi, "BATCH_" + name) == kind
    for cls in (world.Characters, world.Particles, world.Crafts, world.Movers):
        assert callable(cls.checkpoint) and callable(cls.rollback)
    assert world.BatchCheckpoint._stem == "batch_checkpoint"


def test_info_size_goes_through_abi_sizeof(lib):
    class Mirror(C.Structure):      # the header's struct, field by field
        _fields_ = [("device_bytes", C.c_uint64), ("host_bytes", C.c_uint64), ("kind", C.c_uint32), ("capacity", C.c_uint32), ("high_slot", C.c_uint32),
                    ("num_alive", C.c_uint32), ("world_steps_taken", C.c_uint32), ("pad_", C.c_uint32)]
    i = abi.ABI_SIZEOF_ALL.index("sgp_batch_checkpoint_info")
    assert i == 44 and abi.ABI_SIZEOF_ALL[43] is None and lib.sgp_abi_sizeof(43) == -1 and lib.sgp_abi_sizeof(45) == -1
    assert lib.sgp_abi_sizeof(i) == C.sizeof(Mirror) == C.sizeof(abi.BatchCheckpointInfo) == C.sizeof(abi.STRUCTS["sgp_batch_checkpoint_info"]) == 40
    for (name, _), (mname, _) in zip(abi.BatchCheckpointInfo._fields_, Mirror._fields_):
        assert name == mname and getattr(abi.BatchCheckpointInfo, name).offset == getattr(Mirror, mname).offset
    for k, name in enumerate(abi.ABI_SIZEOF_ALL):      # nothing that was there before moved
        assert lib.sgp_abi_sizeof(k) == (C.sizeof(abi.STRUCTS[name]) if name is not None else -1), (k, name)
    assert abi.ABI_SIZEOF_ORDER[-1] == "sgp_checkpoint_info" and abi.ABI_SIZEOF_ALL[41:43] == ["sgp_mover_desc", "sgp_mover_state"]


def test_null_arguments_are_invalid(lib):
    """Every entry with a NULL batch / NULL checkpoint: SGP_ERR_INVALID, decided before anything asks the HIP runtime."""
    info = abi.BatchCheckpointInfo()
    for b in BATCHES:
        h = C.c_void_p()
        cap, back = getattr(lib, f"sgp_{b}_checkpoint"), getattr(lib, f"sgp_{b}_rollback")
        assert cap(None, C.byref(h)) == abi.ERR_INVALID and h.value is None
        assert cap(None, None) == abi.ERR_INVALID
        assert back(None, None) == abi.ERR_INVALID
        assert lib.sgp_last_error()
    assert lib.sgp_batch_checkpoint_get_info(None, C.byref(info)) == abi.ERR_INVALID
    assert lib.sgp_batch_checkpoint_destroy(None) == abi.OK
