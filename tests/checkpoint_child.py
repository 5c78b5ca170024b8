"""Child process of tests/test_checkpoint_gpu.py (a fresh interpreter; never an exec of a process that has opened the GPU).

  restore <scene> <blob file> <first step> <n> <out prefix>    restores the blob into a fresh world of the scene's description, records n steps
  record  <scene> <n1> <n2> <out prefix>                       builds the scene, steps n1, captures, records n2 steps, rolls back, records n2 again
                                                               (run with SGP_CHECKPOINT_FULL=1 for the full-copy side of the comparison)
The recordings go to <out prefix>.npy (bytes, concatenated) and <out prefix>.len.npy (bytes per step)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import checkpoint_scenes as cs      # noqa: E402
from substrata_amd.lib import World      # noqa: E402

SCENES = {"mixed": cs.MixedPile, "shapes": cs.Shapes, "vehicles": cs.Vehicles}


def save(prefix, recs):
    np.save(prefix + ".npy", np.concatenate(recs))
    np.save(prefix + ".len.npy", np.array([len(r) for r in recs], np.int64))


def main(argv):
    mode, scene = argv[1], SCENES[argv[2]]()
    if mode == "restore":
        blob, first, n, out = open(argv[3], "rb").read(), int(argv[4]), int(argv[5]), argv[6]
        # the ids a scene's build() hands out do not depend on the device: a throw-away build tells the driver what to drive
        w = scene.world(World)
        ctx = scene.ids_only()
        ctx["slots"] = scene.max_bodies
        w.restore(blob)
        save(out, cs.run(w, scene, ctx, first, n))
        w.close()
    elif mode == "record":
        n1, n2, out = int(argv[3]), int(argv[4]), argv[5]
        w = scene.world(World)
        ctx = scene.make(w)
        cs.run(w, scene, ctx, 0, n1, rec=False)
        cp = w.checkpoint()
        a = cs.run(w, scene, ctx, n1, n2)
        w.rollback(cp)
        b = cs.run(w, scene, ctx, n1, n2)
        save(out, a + b)
        cp.close()
        w.close()
    else:
        raise SystemExit("unknown mode " + mode)


if __name__ == "__main__":
    main(sys.argv)
