"""Time per frame of N = 1, 64, 1024 characters walking on the ground around the settled config-3 pile: the batched character controller (sgp_characters_*:
update + get_states) against the host walk (JPH::CharacterVirtual of shim/Jolt/JoltCharacterLite.h, one character after the other, every query a launch and a
wait).  Median of 30 frames after 5 of warm-up, both on the same world.   PYTHONPATH=. python tools/experiments/characters_bench.py [frames]"""
import os
import subprocess
import sys
import tempfile

from substrata_amd import build, build_shim, scenes

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.dirname(build.build())
build_shim.build()
frames = sys.argv[1] if len(sys.argv) > 1 else "30"
with tempfile.TemporaryDirectory() as tmp:
    descs = os.path.join(tmp, "config3.bin")
    scenes.config3_100k_mixed().tofile(descs)
    exe = os.path.join(tmp, "characters_bench")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(LIB_DIR, "shim"), os.path.join(HERE, "characters_bench.cpp"), "-o", exe,
                    "-L", LIB_DIR, "-lsgp_shim", "-lsgp", f"-Wl,-rpath,{LIB_DIR}"], check=True)
    sys.exit(subprocess.run([exe, descs, frames]).returncode)
