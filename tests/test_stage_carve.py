"""The stage-carving helper of the query entry points (substrata_amd/csrc/sgp_stage_carve.h) under AddressSanitizer and UBSan, without a GPU: a stand-alone
program (tests/cpp/stage_carve_check.cpp) carves the regions the five entry points request at n = 1 and n = 2^20 and touches both ends of every region."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_carve_regions_are_aligned_disjoint_and_inside_the_total(tmp_path):
    exe = str(tmp_path / "stage_carve_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    os.path.join(ROOT, "tests", "cpp", "stage_carve_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(" regions, ") == 11, r.stdout
