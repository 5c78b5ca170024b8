"""The host bookkeeping of sgp_proximity (substrata_amd/csrc/sgp_proximity_host.h over sgp_batch_slots.h) under AddressSanitizer and UBSan, without a GPU: a
stand-alone program (tests/cpp/proximity_host_check.cpp) fills, refills and restores the zone table with its generations, adds objects in batches against the
body links through the function the library calls, with one walk per call."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_zone_generations_and_batched_add(tmp_path):
    exe = str(tmp_path / "proximity_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    os.path.join(ROOT, "tests", "cpp", "proximity_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout, r.stdout
    assert all(s in r.stdout for s in ("zone table: ok", "batched add: ok")), r.stdout
