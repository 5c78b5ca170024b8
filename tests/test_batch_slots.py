"""The host bookkeeping the device-resident batches share (substrata_amd/csrc/sgp_batch_slots.h) under AddressSanitizer and UBSan, without a GPU: a stand-alone
program (tests/cpp/batch_slots_check.cpp) fills slot tables of capacity 1 and 3, frees and reuses their slots, and walks body links through a reborn body, a
body that stops qualifying and a gone slot's detach."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_slots_reuse_order_and_body_links(tmp_path):
    exe = str(tmp_path / "batch_slots_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    os.path.join(ROOT, "tests", "cpp", "batch_slots_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout, r.stdout
    assert r.stdout.count("slot table of ") == 3 and "body links: ok" in r.stdout, r.stdout
