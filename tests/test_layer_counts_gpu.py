"""sgp_step_stats::layer_counts is kept on the host as bodies come, go and change layer (no walk over the body slots per step): after every kind of
edit that can change it, the step reports what a count over the test's own model of the world gives.  The rule: a slot counts under its layer iff it
is alive and no alias slot of a mesh body -- a plain body is one slot, a mesh body one (its two alias slots do not count), a compound one per child."""
import numpy as np
import pytest

from substrata_amd import abi, scenes
from substrata_amd.lib import World
from helpers import DT
from test_mesh_parity_gpu import grid_mesh, mesh_body
from compound_scene import add_portal

pytestmark = pytest.mark.gpu

L0, L1, L2, L3 = abi.LAYER_NON_MOVING, abi.LAYER_MOVING, abi.LAYER_NON_MOVING_NON_COLLIDABLE, abi.LAYER_MOVING_NON_COLLIDABLE


class Model:
    """id -> (layer, slots that count); compounds make num_bodies differ from the sum"""
    def __init__(self):
        self.b = {}
        self.compounds = 0

    def counts(self):
        c = [0] * abi.NUM_LAYERS
        for layer, slots in self.b.values():
            c[layer] += slots
        return c

    def copy(self):
        m = Model(); m.b = dict(self.b); m.compounds = self.compounds
        return m


def check(w, m, what, steps=1):
    for _ in range(steps):
        w.step(DT)
        st = w.stats()
        assert list(st.layer_counts) == m.counts(), (what, list(st.layer_counts), m.counts())
        assert st.num_bodies == len(m.b), (what, st.num_bodies, len(m.b))
        if m.compounds == 0:
            assert sum(st.layer_counts) == st.num_bodies, what


def batch(w, m, n, layer, motion, z, gravity=1.0, x0=0.0):
    d = scenes._blank(n)
    d["motion_type"] = motion; d["layer"] = layer; d["gravity_factor"] = gravity; d["activate"] = 1 if motion != abi.MOTION_STATIC else 0
    d["mass"] = 50.0
    d["pos"][:, 0] = x0 + 1.5 * (np.arange(n) % 10); d["pos"][:, 1] = 1.5 * (np.arange(n) // 10); d["pos"][:, 2] = z
    ids = [int(i) for i in w.add_batch(d)]
    assert abi.INVALID_ID not in ids
    for i in ids:
        m.b[i] = (layer, 1)
    return ids


def test_layer_counts_follow_every_edit():
    w = World(max_bodies=4096)
    m = Model()
    # a batch over all four layers: ground + static props, a field of boxes resting on the ground, static and weightless bodies that collide with nothing
    g = [int(w.add_batch(scenes.ground())[0])]; m.b[g[0]] = (L0, 1)
    stat = batch(w, m, 12, L0, abi.MOTION_STATIC, 0.5, x0=40.0)
    mov = batch(w, m, 60, L1, abi.MOTION_DYNAMIC, 0.5)
    nstat = batch(w, m, 9, L2, abi.MOTION_STATIC, 5.0, x0=40.0)
    nmov = batch(w, m, 11, L3, abi.MOTION_DYNAMIC, 8.0, gravity=0.0)
    check(w, m, "batch add", steps=3)
    # remove, from every layer
    for i in (stat[0], stat[5], mov[3], mov[17], mov[59], nstat[2], nmov[0], nmov[10]):
        w.remove(i); del m.b[i]
    check(w, m, "remove")
    # set_layer, between the moving layers, between the static ones, and there and back before a step sees it
    for i, layer in ((mov[0], L3), (mov[1], L3), (nmov[1], L1), (stat[1], L2), (nstat[0], L0), (mov[1], L1)):
        w.set_layer(i, layer); m.b[i] = (layer, m.b[i][1])
    check(w, m, "set_layer", steps=2)
    # freed slots are handed out again
    again = batch(w, m, 5, L3, abi.MOTION_DYNAMIC, 9.0, gravity=0.0, x0=60.0)
    check(w, m, "add into freed slots")
    # a mesh body: three slots, one of them counts
    V, T = grid_mesh(9, 6.0, lambda x, y: 0.0 * x)
    info = w.mesh_create(V, T)
    mesh = int(w.add_batch(mesh_body(info, pos=(80.0, 0.0, 0.0)))[0]); m.b[mesh] = (L0, 1)
    check(w, m, "mesh body")
    w.set_layer(mesh, L2); m.b[mesh] = (L2, 1)
    check(w, m, "mesh body, new layer")
    cp = w.checkpoint()
    m_cp = m.copy()
    # a static compound: one object, one counted slot per child (mesh child + box child)
    portal, _ = add_portal(w, (100.0, 0.0, 0.0))
    assert w.compound_size(portal) == 2
    m.b[portal] = (L0, 2); m.compounds += 1
    check(w, m, "compound")
    w.set_layer(portal, L2); m.b[portal] = (L2, 2)
    check(w, m, "compound, new layer")
    w.remove(mesh); del m.b[mesh]
    for i in again[:3]:
        w.remove(i); del m.b[i]
    w.set_layer(mov[0], L1); m.b[mov[0]] = (L1, 1)
    check(w, m, "after the checkpoint: removals")
    # back to the earlier state
    w.rollback(cp)
    m = m_cp.copy()
    check(w, m, "rollback", steps=2)
    portal, _ = add_portal(w, (100.0, 0.0, 0.0))
    m.b[portal] = (L0, 2); m.compounds += 1
    check(w, m, "compound after the rollback")
    w.remove(portal); del m.b[portal]; m.compounds -= 1
    check(w, m, "compound removed")
    # the same state loaded into a fresh world
    blob = cp.to_bytes()
    w2 = World(max_bodies=4096)
    w2.restore(blob)
    check(w2, m_cp, "restore", steps=2)
    w2.close()
    # everything falls asleep: idle steps (nothing is launched) keep reporting the counts
    w.remove(mov[0]); del m.b[mov[0]]      # (it has been falling through the ground since it left the moving layer)
    idle0 = w.launch_counts()[2]
    for s in range(900):
        check(w, m, f"settling, step {s}")
        if w.launch_counts()[2] >= idle0 + 5:
            break
    assert w.launch_counts()[2] >= idle0 + 5, "the scene never fell asleep: no idle step was seen"
    # ... and an edit after idle steps is counted at once
    w.remove(nmov[3]); del m.b[nmov[3]]
    w.set_layer(stat[2], L2); m.b[stat[2]] = (L2, 1)
    check(w, m, "edit after idle steps", steps=3)
    cp.close()
    w.close()


def test_layer_counts_with_ghosts_and_migration():
    """two tile worlds in one process: the ghosts a world holds count under their layer like any body, through creation (host records), refresh, removal,
    and bodies that change owner"""
    from substrata_amd.tiles import route, split, records_to_descs
    boxes = np.array([[-60.0, -60.0, -10.0, 0.0, 60.0, 60.0], [0.0, -60.0, -10.0, 60.0, 60.0, 60.0]], np.float32)
    margin, pad = 2.0, 1.5
    worlds = [World(max_bodies=2048) for _ in range(2)]
    own = []      # per world: layer of each body it owns, by count
    for r, w in enumerate(worlds):
        w.add_batch(scenes.ground())
        sgn = -1.0 if r == 0 else 1.0
        d = scenes.dynamic_bodies(40)
        d["pos"][:, 0] = sgn * (0.8 + 1.3 * (np.arange(40) % 10)); d["pos"][:, 1] = 1.5 * (np.arange(40) // 10) + 20.0 * r; d["pos"][:, 2] = 0.5
        d["layer"] = np.where(np.arange(40) % 4 == 3, L3, L1); d["gravity_factor"] = np.where(np.arange(40) % 4 == 3, 0.0, 1.0)
        d["lin_vel"][:5, 0] = -sgn * 4.0; d["friction"][:5] = 0.0          # five of them are on their way into the other tile
        w.add_batch(d)
        c = [1, 0, 0, 0]
        for layer in d["layer"]:
            c[int(layer)] += 1
        own.append(c)
    saw_ghosts = saw_migration = 0
    for s in range(90):
        sent = []
        for r, w in enumerate(worlds):
            recs = w.export_boundary(boxes[r, :3], boxes[r, 3:], margin)
            send, counts, emig = route(recs, r, boxes, margin + pad)
            off = [0] + [int(x) for x in np.cumsum(counts)]
            sent.append([send[off[q]:off[q + 1]] for q in range(2)])
            for i in emig:
                w.remove(int(i))
            sent[-1].append(len(emig))
        ghost_layers = []
        for r, w in enumerate(worlds):
            arrived = sent[1 - r][r]
            ghosts, immigrants = split(arrived, boxes[r, :3], boxes[r, 3:])
            w.import_ghosts(ghosts)
            if len(immigrants):
                w.add_batch(records_to_descs(immigrants))
            for f in immigrants["flags"]:
                own[r][int(f) & abi.GHOST_FLAG_LAYER_MASK] += 1
                own[1 - r][int(f) & abi.GHOST_FLAG_LAYER_MASK] -= 1
            assert len(immigrants) == sent[1 - r][2]
            saw_migration += len(immigrants)
            g = [0] * abi.NUM_LAYERS
            for f in ghosts["flags"]:
                g[int(f) & abi.GHOST_FLAG_LAYER_MASK] += 1
            ghost_layers.append(g)
            saw_ghosts += len(ghosts)
        for r, w in enumerate(worlds):
            w.step(DT)
            st = w.stats()
            want = [own[r][k] + ghost_layers[r][k] for k in range(abi.NUM_LAYERS)]
            assert list(st.layer_counts) == want, (s, r, list(st.layer_counts), want)
            assert sum(st.layer_counts) == st.num_bodies
    assert saw_ghosts > 0 and saw_migration >= 4
    for w in worlds:
        w.close()
