"""CPU-side checks of the checkpoint entry points (include/sgp.h, "world checkpoints"): exported and prototyped, the info struct has the
library's size, NULL handles are refused without touching the HIP runtime, and sgp_checkpoint_blob_info -- which needs no device --
rejects everything that is not a well-formed blob.  No world exists here (no device: sgp_world_create says SGP_ERR_NO_DEVICE)."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

from substrata_amd import abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["world_checkpoint", "world_rollback", "checkpoint_destroy", "checkpoint_get_info", "checkpoint_write", "world_restore",
         "checkpoint_blob_info"]
MAGIC = b"SGPCKPT\0"


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(build.build())
    abi.bind(lib, "sgp_")
    return lib


def test_symbols_exported_and_prototyped(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgp.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\bsgp_%s\s*\(" % n, header), f"include/sgp.h does not declare sgp_{n}"
        assert hasattr(lib, "sgp_" + n), f"libsgp.so does not export sgp_{n}"
        assert n in abi.PROTOTYPES, f"abi.PROTOTYPES lacks {n}"
        assert getattr(lib, "sgp_" + n).argtypes is not None


def test_info_size_matches(lib):
    assert abi.ABI_SIZEOF_ORDER[-1] == "sgp_checkpoint_info"
    i = abi.ABI_SIZEOF_ORDER.index("sgp_checkpoint_info")
    assert lib.sgp_abi_sizeof(i) == C.sizeof(abi.CheckpointInfo) == 72


def test_null_arguments_are_invalid(lib):
    """Every entry with a NULL world / NULL checkpoint: SGP_ERR_INVALID, decided before anything asks the HIP runtime."""
    info = abi.CheckpointInfo()
    h = C.c_void_p()
    n = C.c_uint64(0)
    buf = (C.c_uint8 * 64)()
    assert lib.sgp_world_checkpoint(None, C.byref(h)) == abi.ERR_INVALID
    assert h.value is None
    assert lib.sgp_world_checkpoint(None, None) == abi.ERR_INVALID
    assert lib.sgp_world_rollback(None, None) == abi.ERR_INVALID
    assert lib.sgp_checkpoint_get_info(None, C.byref(info)) == abi.ERR_INVALID
    assert lib.sgp_checkpoint_write(None, buf, 64, C.byref(n)) == abi.ERR_INVALID
    assert lib.sgp_world_restore(None, buf, 64) == abi.ERR_INVALID
    assert lib.sgp_checkpoint_blob_info(None, 64, C.byref(info)) == abi.ERR_INVALID
    assert lib.sgp_checkpoint_blob_info(buf, 64, None) == abi.ERR_INVALID
    assert lib.sgp_last_error()
    assert lib.sgp_checkpoint_destroy(None) == abi.OK


def _blob_info(lib, data):
    info = abi.CheckpointInfo()
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(bytes(data) or b"\0")
    return lib.sgp_checkpoint_blob_info(buf, len(data), C.byref(info))


FORMAT_VERSION = 2      # CKPT_FORMAT_VERSION of sgp_world_checkpoint.hip


def _header(total, host=0, shape=0, table=0, data=0, abi_version=abi.ABI_VERSION, fmt=FORMAT_VERSION, header_bytes=None):
    """The fixed part of a blob's header as include/sgp.h's implementation lays it out: magic, four u32, five u64; the rest zero."""
    desc_bytes = C.sizeof(abi.WorldDesc)
    size = 8 + 16 + 40 + 32 + C.sizeof(abi.CheckpointInfo) + desc_bytes
    hb = (size + 15) & ~15 if header_bytes is None else header_bytes
    h = MAGIC + struct.pack("<4I5Q", abi_version, fmt, hb, desc_bytes, total, host, shape, table, data)
    return h + b"\0" * (hb - len(h))


def test_blob_info_rejects_what_is_not_a_blob(lib):
    assert _blob_info(lib, b"") == abi.ERR_INVALID
    rng = np.random.default_rng(5)
    for n in (1, 7, 64, 300, 4096):
        assert _blob_info(lib, rng.integers(0, 256, n, dtype=np.uint8).tobytes()) == abi.ERR_INVALID
    # random bytes behind a correct magic
    assert _blob_info(lib, MAGIC + rng.integers(0, 256, 1000, dtype=np.uint8).tobytes()) == abi.ERR_INVALID
    # a correct magic with a wrong version (format, then ABI)
    h = _header(0)
    good_len = len(h)
    assert _blob_info(lib, _header(good_len, fmt=FORMAT_VERSION + 1)) == abi.ERR_INVALID
    assert b"version" in lib.sgp_last_error()
    assert _blob_info(lib, _header(good_len, abi_version=abi.ABI_VERSION + 1)) == abi.ERR_INVALID
    assert b"version" in lib.sgp_last_error()
    # a header whose section sizes exceed the buffer, or do not add up to it
    assert _blob_info(lib, _header(good_len, host=1 << 40)) == abi.ERR_INVALID
    assert _blob_info(lib, _header(good_len, data=1 << 62, table=1 << 62)) == abi.ERR_INVALID
    assert _blob_info(lib, _header(good_len, host=8)) == abi.ERR_INVALID
    assert _blob_info(lib, _header(good_len + 8, host=16) + b"\0" * 8) == abi.ERR_INVALID
    # truncated: the header says more than there is
    assert _blob_info(lib, _header(good_len + 4096)) == abi.ERR_INVALID
    # sizes that add up, sections that hold nothing sensible
    assert _blob_info(lib, _header(good_len + 64, host=64) + b"\xff" * 64) == abi.ERR_INVALID
    assert _blob_info(lib, _header(good_len)) == abi.ERR_INVALID


def test_python_blob_info_raises(lib):
    from substrata_amd.world import SgpError
    with pytest.raises(SgpError):
        abi.blob_info(b"not a blob", lib=lib)
