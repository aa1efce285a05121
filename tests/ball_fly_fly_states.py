"""Poses of the tethered fly (walk_on_ball) in which its own geoms touch, found with the float64 oracle on the CPU: the states behind the
fly-fly tests of tests/test_gpu_ball.py and rows 0-19 of tests/golden/ball_parent_digest.npz (tools/record_ball_digest.py)."""
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BALL_BLOB = os.path.join(ROOT, "flybody_amd", "assets", "fly_ball.ffmb")


@functools.lru_cache(maxsize=4)
def fly_fly_states(n, seed=0, max_depth=0.003):
    """Random joint poses (inside the joint ranges) in which the fly's own geoms touch: legs against legs, mouth parts against
    front legs, abdomen tip against hind tarsi, claws (margin + gap, adhesion) - sphere / capsule pairs - and pairs with an
    ellipsoid or a cylinder on one side (femur / tibia / coxa on an abdomen segment, legs on the thorax or head, ...: the general
    convex collider).  Found with the oracle; returns [(qpos, qvel, act, names of the touching pairs)] with shallow penetrations only.
    (The labrum halves and the haustellum on the head touch in every pose; a pose qualifies by a pair beyond those.)"""
    import json

    from flybody_amd.model.blob import read_blob
    from oracle import oracle as O

    t = read_blob(BALL_BLOB)
    meta = json.load(open(BALL_BLOB.replace(".ffmb", ".json")))
    names, jname = meta["geom_name"], meta["jnt_name"]
    gtype = np.asarray(t["geom_type"])
    m = O.OracleModel(BALL_BLOB)
    d = O.OracleData(m)
    rng = np.random.RandomState(seed)
    hinge = [j for j in range(len(t["jnt_type"])) if t["jnt_type"][j] == 3]
    cand = {"claw": [], "mouth": [], "convex": [], "other": []}
    lo_, hi_ = t["jnt_range"][hinge].T
    qa = t["jnt_qposadr"][hinge]
    always = {("labrum_left_lower_collision", "labrum_right_lower_collision"), ("haustellum_collision", "head_collision")}

    def pose(dq, amp):
        q = t["qpos0"].copy()
        q[qa] = np.clip(q[qa] + amp * dq * (hi_ - lo_) / 2, lo_, hi_)
        d.qpos[:] = q; d.qvel[:] = 0; d.act[:] = 0; d.ctrl[:] = 0
        d.forward()
        c = d.contacts()
        sc = [r for r in c if "ball" not in names[int(r[0])] and "ball" not in names[int(r[1])]]
        return q, c, sc, [r for r in sc if (names[int(r[0])], names[int(r[1])]) not in always]

    for _ in range(4000):
        if all(len(cand[k]) >= n // 4 for k in ("claw", "mouth", "convex")) and len(cand["other"]) >= n:
            break
        # a random direction in joint space, scaled up until the first fly-fly pair touches (bisection), then a little further:
        # a shallow contact, as a simulation would meet it
        dq = rng.uniform(-1, 1, len(hinge))
        # move two legs plus (sometimes) the head / mouth parts and the abdomen; the other legs keep standing on the ball
        moving = list(rng.choice(["T1_left", "T1_right", "T2_left", "T2_right", "T3_left", "T3_right"], 2, replace=False))
        moving += [x for x in ("head", "rostrum", "haustellum", "labrum", "antenna") if rng.rand() < 0.5] + (["abdomen"] if rng.rand() < 0.5 else [])
        dq *= np.array([any(k in jname[j] for k in moving) for j in hinge], dtype=float)
        a0, a1 = 0.0, 1.0
        if not pose(dq, a1)[3]:
            continue
        for _ in range(14):
            am = 0.5 * (a0 + a1)
            if pose(dq, am)[3]:
                a1 = am
            else:
                a0 = am
        q, c, sc, new = pose(dq, a1 + rng.uniform(0.002, 0.02))
        if not new or len(c) > 14 or d.nefc > 40 or any(r[5] < -max_depth for r in sc) or any(r[5] < -0.02 for r in c):
            continue
        pairs = [(names[int(r[0])], names[int(r[1])]) for r in sc]
        newp = [(names[int(r[0])], names[int(r[1])]) for r in new]
        kind = "claw" if any("claw" in x or "claw" in y for x, y in newp) else (
            "convex" if any(gtype[int(r[0])] >= 4 or gtype[int(r[1])] >= 4 for r in new) else (
                "mouth" if any(x.split("_")[0] in ("rostrum", "haustellum", "antenna") for x, y in newp) else "other"))
        cand[kind].append((q.copy(), rng.randn(m.nv) * 2.0, rng.uniform(-0.3, 0.3, m.na), pairs))
    out = cand["claw"][: n // 4] + cand["mouth"][: n // 4] + cand["convex"][: n // 4]   # the rarer kinds first, the rest legs against legs / abdomen tip
    out += cand["other"][: n - len(out)]
    assert len(out) == n, {k: len(v) for k, v in cand.items()}
    return m, names, out
