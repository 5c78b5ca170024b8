"""What a frame of particles costs (tools/experiments/particles_cost.cpp): 2048 particles on the scene of tests/cpp/particle_rays.cpp through the host loop over
the batched traceRays() and through ParticleBatch (sgp_particles_update + one sgp_particles_read per frame), in one process, wall clock and HIP events; then
sgp_particles_update for 65 536 and 1 048 576 particles over config 3's settled pile, and the step's rate with and without particles behind it.
PYTHONPATH=. python tools/experiments/particles_cost.py [frames = 200]"""
import os
import subprocess
import sys
import tempfile

from substrata_amd import build, build_shim, scenes

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.dirname(build.build())
build_shim.build()
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
frames = sys.argv[1] if len(sys.argv) > 1 else "200"
with tempfile.TemporaryDirectory() as tmp:
    descs = os.path.join(tmp, "config3.bin")
    scenes.config3_100k_mixed().tofile(descs)
    exe = os.path.join(tmp, "particles_cost")
    subprocess.run(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", os.path.join(LIB_DIR, "shim"),
                    os.path.join(HERE, "particles_cost.cpp"), "-o", exe, "-L", LIB_DIR, "-lsgp_shim", "-lsgp", "-L", os.path.join(ROCM, "lib"), "-lamdhip64",
                    f"-Wl,-rpath,{LIB_DIR}", f"-Wl,-rpath,{os.path.join(ROCM, 'lib')}"], check=True)
    sys.exit(subprocess.run([exe, descs, frames]).returncode)
