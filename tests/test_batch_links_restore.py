"""What a batch checkpoint keeps of the slot and body-link tables (substrata_amd/csrc/sgp_batch_slots.h) under AddressSanitizer and UBSan, without a GPU: a
stand-alone program (tests/cpp/batch_links_restore_check.cpp) snapshots and restores a BatchSlots (the free list's order and the next id) and walks the relink
rule through a body that still qualifies, a body that has gone, a body another slot took over since the capture, a slot that was gone at the capture and a
table that grew since."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slots_snapshot_and_the_relink_rule(tmp_path):
    exe = str(tmp_path / "batch_links_restore_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    os.path.join(ROOT, "tests", "cpp", "batch_links_restore_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout, r.stdout
    assert "slots snapshot: ok" in r.stdout and "relink rule: ok" in r.stdout, r.stdout
