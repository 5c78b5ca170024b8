"""The host bookkeeping of sgp_audibility (substrata_amd/csrc/sgp_audibility_host.h over sgp_batch_slots.h) under AddressSanitizer and UBSan, without a GPU: a
stand-alone program (tests/cpp/audibility_host_check.cpp) checks the capacities a batch accepts, indexes the pair table at a listener capacity of 1 and of 32,
fills and looks up the muting-key list, adds POINT and BODY sources in batches against the body links through the function the library calls, and takes the
slot and link tables through a snapshot and back."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pairs_muting_keys_slots_and_snapshots(tmp_path):
    exe = str(tmp_path / "audibility_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    os.path.join(ROOT, "tests", "cpp", "audibility_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout, r.stdout
    assert all(s in r.stdout for s in ("capacities and pairs: ok", "muting keys: ok", "slots and links: ok")), r.stdout
