"""Shared by tests/test_walk_floor_convex_cpu.py and tests/test_gpu_walk_floor_convex.py: the floor plane against the walking fly's
ellipsoids and cylinders (FFE_WALK_FLOOR_CONVEX).

  restatement   `plane_ellipsoid` / `plane_cylinder`: float64 numpy, written from the published formulas of mjc_PlaneConvex and
                mjc_PlaneCylinder (not from csrc/walk_floor_convex.hpp), and `restated(qpos)`: the contacts of the 22 candidates of the
                shipped blob at a pose, from the oracle's geom frames
  witness       the oracle does not restate these two colliders.  A plane-sphere contact of a sphere of radius rho is
                dist = n.(centre - x0) - rho, pos = centre - n (rho + dist / 2), so the plane-convex contact (pos p, dist d) of geom g is
                reproduced exactly by a sphere of radius rho on g's body centred at p + n (rho + d / 2).  `witness_model(qpos)` appends one
                such sphere per restated contact to every per-geom tensor of the shipped blob (a copy of g's row: the pair's parameters
                are g's), visible to the floor alone (the floor gets a second contype bit, the witness that bit as its conaffinity and no
                contype).  The oracle on that blob then has the device's floor contacts and its fly-fly contacts untouched - for the
                collision pass of THAT state only: the spheres do not follow the surface when the pose changes.
  state sets    A (on its abdomen), B (on its back), C (coxae and mouth parts): fallen poses within the kernel's capacities (16 contacts,
                48 rows, 24 rows per block of the inertia), generated once per session on the CPU."""
import functools
import os
import tempfile

import numpy as np

import walk_self_sets as S
from walk_floor_sets import WALK_BLOB

WALK_FLOOR_CONVEX = 32768
FULL = S.SELF | WALK_FLOOR_CONVEX
RHO = 0.01      # cm: radius of a witness sphere
CLEAR = 1e-4    # cm: no candidate of a state may be this close to a switching distance
TINY = 1e-15    # mjMINVAL
_keep = []


# ------------------------------------------------------------------------------------------------ the two colliders, float64
def plane_ellipsoid(n, x0, c, R, s, margin=0.0):
    """[(pos, dist)]: zero or one contact.  d = -R'n, w = s*s*d, p = c + R w / sqrt(d.w), dist = n.(p - x0), kept if dist <= margin."""
    n, x0, c, R, s = (np.asarray(a, dtype=np.float64) for a in (n, x0, c, R, s))
    d = -(R.T @ n)
    w = s * s * d
    p = c + R @ w / np.sqrt(d @ w)
    dist = float(n @ (p - x0))
    return [(p - n * dist / 2, dist)] if dist <= margin else []


def plane_cylinder(n, x0, c, R, r, h, margin=0.0):
    """[(pos, dist)]: zero to four contacts in MuJoCo's order."""
    n, x0, c, R = (np.asarray(a, dtype=np.float64) for a in (n, x0, c, R))
    a = R[:, 2].copy()
    dist0 = float(n @ (c - x0))
    pa = float(n @ a)
    if pa > 0:
        a, pa = -a, -pa
    vec = a * pa - n
    ln = float(np.linalg.norm(vec))
    vec = r * R[:, 0] if ln < TINY else vec * (r / ln)
    pv = float(n @ vec)
    ax = h * a
    pa *= h
    out = []
    d1 = dist0 + pa + pv
    if d1 > margin:
        return out
    out.append((c + vec + ax - n * d1 / 2, d1))
    d2 = dist0 - pa + pv
    if d2 <= margin:
        out.append((c + vec - ax - n * d2 / 2, d2))
    d3 = dist0 + pa - pv / 2
    if d3 <= margin:
        v1 = np.cross(vec, ax)
        v1 *= r * np.sqrt(3.0) / 2 / np.linalg.norm(v1)
        out.append((c + v1 + ax - vec / 2 - n * d3 / 2, d3))
        out.append((c - v1 + ax - vec / 2 - n * d3 / 2, d3))
    return out


# ------------------------------------------------------------------------------------------------ the candidates of the shipped blob
@functools.lru_cache(maxsize=1)
def tables():
    from flybody_amd.model.blob import read_blob

    return read_blob(WALK_BLOB)


def _flat(name):
    return np.asarray(tables()[name]).ravel()


@functools.lru_cache(maxsize=1)
def floor_geom():
    body, ty = _flat("geom_bodyid"), _flat("geom_type")
    (g,) = np.nonzero((body == 0) & (ty == 0))[0]
    return int(g)


def floor_candidates(types):
    """Geoms of the given types that pass mj_collision's filter against the floor geom (contype / conaffinity, <exclude>), model order."""
    t = tables()
    body, ty, ct, ca = _flat("geom_bodyid"), _flat("geom_type"), _flat("geom_contype"), _flat("geom_conaffinity")
    excl = {tuple(sorted(map(int, e))) for e in np.asarray(t["exclude_pairs"]).reshape(-1, 2)}
    f = floor_geom()
    return [g for g in range(len(ty)) if g != f and ty[g] in types and ((ct[f] & ca[g]) or (ct[g] & ca[f])) and (0, int(body[g])) not in excl
            and body[g] != 0]


@functools.lru_cache(maxsize=1)
def plane():
    """(unit normal, point) of the floor in the world; the floor hangs on the world body, whose frame is the world's on this model."""
    t, f = tables(), floor_geom()
    assert np.allclose(np.asarray(t["body_pos"])[0], 0) and np.allclose(np.asarray(t["body_quat"])[0], [1, 0, 0, 0])
    w, x, y, z = np.asarray(t["geom_quat"], dtype=np.float64)[f]
    n = np.array([2 * (x * z + w * y), 2 * (y * z - w * x), 1 - 2 * (x * x + y * y)])
    return n / np.linalg.norm(n), np.asarray(t["geom_pos"], dtype=np.float64)[f].copy()


def pair_margin(g):
    """(margin, margin - gap) of the pair (floor, g): the larger value of each (mj_contactParam)."""
    f = floor_geom()
    mg, gp = _flat("geom_margin"), _flat("geom_gap")
    margin = max(float(mg[g]), float(mg[f]))
    return margin, margin - max(float(gp[g]), float(gp[f]))


def restated_at(geom_xpos, geom_xmat, margin_of=pair_margin):
    """([(geom, pos, dist, active)] of the 22 candidates at the given geom frames (world), in (geom, contact) order, clearance): `active`
    = inside margin - gap; `clearance` = how far every candidate distance, kept or not, stays from a switching distance (margin, or
    margin - gap)."""
    n, x0 = plane()
    size, ty = np.asarray(tables()["geom_size"], dtype=np.float64), _flat("geom_type")
    out, clear = [], np.inf
    for g in floor_candidates((4, 5)):
        margin, incl = margin_of(g)
        c, R = geom_xpos[g], geom_xmat[g]
        if ty[g] == 4:
            every = plane_ellipsoid(n, x0, c, R, size[g], np.inf)
        else:
            every = plane_cylinder(n, x0, c, R, size[g, 0], size[g, 1], np.inf)
        for _, d in every:
            clear = min(clear, abs(d - margin), abs(d - incl))
        got = plane_ellipsoid(n, x0, c, R, size[g], margin) if ty[g] == 4 else plane_cylinder(n, x0, c, R, size[g, 0], size[g, 1], margin)
        out += [(g, p, d, d < incl) for p, d in got]
    return out, clear


def forward(qpos):
    """An OracleData of the shipped blob after mj_forward at `qpos` (zero velocity)."""
    from oracle import oracle as O

    d = O.OracleData(S.model())
    d.qpos[:] = qpos; d.qvel[:] = 0; d.act[:] = 0; d.ctrl[:] = 0
    d.forward()
    return d


def restated(qpos, d=None):
    d = d or forward(qpos)
    return restated_at(d.geom_xpos, d.geom_xmat)


def matter(contacts):
    """The restated contacts the kernel keeps: the active ones (no ellipsoid / cylinder of the fly sits on a body with an adhesion
    actuator, so one inside its margin but outside margin - gap takes part in nothing)."""
    body = _flat("geom_bodyid")
    assert not {int(body[g]) for g in floor_candidates((4, 5))} & S._adhesion_bodies()
    return [c for c in contacts if c[3]]


# ------------------------------------------------------------------------------------------------ witness spheres
PER_GEOM = ("geom_bodyid", "geom_type", "geom_size", "geom_pos", "geom_quat", "geom_condim", "geom_friction", "geom_margin", "geom_gap",
            "geom_solref", "geom_solimp", "geom_solmix", "geom_priority", "geom_contype", "geom_conaffinity")


def witness_tensors(qpos, contacts=None, d=None):
    """(blob tensors with one witness sphere per restated contact, the contacts).  A witness copies its geom's margin and gap, so that
    the oracle forms the same includemargin; its distance and position are the wanted ones whatever rho is."""
    d = d or forward(qpos)
    contacts = restated(qpos, d)[0] if contacts is None else contacts
    n, _ = plane()
    t = {k: np.array(v, copy=True) for k, v in tables().items()}
    ng = len(_flat("geom_type"))
    assert sorted(k for k in t if k.startswith("geom_")) == sorted(PER_GEOM) and all(len(t[k]) == ng for k in PER_GEOM)
    f = floor_geom()
    t["geom_contype"].reshape(-1)[f] |= 2
    rows = {k: [] for k in PER_GEOM}
    body = _flat("geom_bodyid")
    for g, p, dist, _ in contacts:
        b = int(body[g])
        cw = p + n * (RHO + dist / 2)
        w, x, y, z = d.xquat[b]
        Rb = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                       [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                       [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        for k in PER_GEOM:
            rows[k].append(np.array(t[k][g], copy=True))
        rows["geom_type"][-1] = np.asarray(2, dtype=t["geom_type"].dtype)
        rows["geom_size"][-1] = np.array([RHO, 0, 0], dtype=t["geom_size"].dtype)
        rows["geom_pos"][-1] = (Rb.T @ (cw - d.xpos[b])).astype(t["geom_pos"].dtype)
        rows["geom_quat"][-1] = np.array([1, 0, 0, 0], dtype=t["geom_quat"].dtype)
        rows["geom_contype"][-1] = np.asarray(0, dtype=t["geom_contype"].dtype)
        rows["geom_conaffinity"][-1] = np.asarray(2, dtype=t["geom_conaffinity"].dtype)
    if contacts:
        for k in PER_GEOM:
            t[k] = np.concatenate([t[k], np.stack(rows[k]).reshape((len(contacts),) + t[k].shape[1:])], axis=0)
    return t, contacts


def witness_model(qpos, contacts=None):
    """(OracleModel of the witness blob of this pose, the restated contacts)"""
    from flybody_amd.model.blob import write_blob
    from oracle import oracle as O

    t, contacts = witness_tensors(qpos, contacts)
    dr = tempfile.TemporaryDirectory(prefix="walk_floor_convex_")
    _keep.append(dr)
    path = os.path.join(dr.name, "fly_walk_witness.ffmb")
    write_blob(path, t)
    return O.OracleModel(path), contacts


def floor_rows(contacts_rows):
    """The rows of `OracleData.contacts()` with the floor plane on one side."""
    f = floor_geom()
    return [r for r in contacts_rows if int(r[0]) == f or int(r[1]) == f]


# ------------------------------------------------------------------------------------------------ state sets
def _quat_xyz(rx, ry, rz):
    """Rotation about x, then y, then z (world axes) as (w, x, y, z)."""
    def q(axis, a):
        out = np.zeros(4); out[0] = np.cos(a / 2); out[1 + axis] = np.sin(a / 2)
        return out

    def mul(a, b):
        return np.array([a[0] * b[0] - a[1:] @ b[1:], *(a[0] * b[1:] + b[0] * a[1:] + np.cross(a[1:], b[1:]))])

    return mul(q(2, rz), mul(q(1, ry), q(0, rx)))


@functools.lru_cache(maxsize=1)
def _hinges():
    t = tables()
    jt = _flat("jnt_type")
    hinge = [j for j in range(len(jt)) if jt[j] == 3]
    lo, hi = np.asarray(t["jnt_range"], dtype=np.float64)[hinge].T
    return hinge, _flat("jnt_qposadr")[hinge], lo, hi


LEGS = ("T1_left", "T1_right", "T2_left", "T2_right", "T3_left", "T3_right")


@functools.lru_cache(maxsize=4)
def tucked(up=(0.0, 0.0, 1.0), seed=1, tries=240):
    """qpos (root at the reset pose, lifted) whose six legs are drawn as far along `up` (root frame) as a random search over each leg's
    joints gets them: every try draws all legs at once, and each leg keeps the draw in which its lowest geom centre is highest."""
    _, names, jname = S.tables()
    hinge, qa, lo, hi = _hinges()
    rng = np.random.RandomState(seed)
    base = S.reset_pose().copy()
    base[:3] = [0, 0, 5.0]; base[3:7] = [1, 0, 0, 0]
    leg_j = {leg: np.array([leg in jname[j] for j in hinge]) for leg in LEGS}
    leg_g = {leg: [g for g in range(len(names)) if leg in names[g]] for leg in LEGS}
    best, best_q = {leg: -np.inf for leg in LEGS}, base.copy()
    up = np.asarray(up, dtype=np.float64)
    for k in range(tries):
        q = base.copy()
        q[qa] = np.where(np.any(list(leg_j.values()), axis=0), rng.uniform(lo, hi), q[qa])
        d = forward(q)
        touching = {int(g) for r in d.contacts() for g in r[:2]}
        for leg in LEGS:
            low = float((d.geom_xpos[leg_g[leg]] @ up).min())
            if low > best[leg] and not touching & set(leg_g[leg]):  # (a leg that touches anything in this draw is not taken)
                best[leg] = low
                best_q[qa[leg_j[leg]]] = q[qa[leg_j[leg]]]
    return best_q


def _settle(q, depth):
    """Moves the root along z so that the lowest restated candidate (contact or not) sits `depth` below the plane."""
    q = q.copy()
    n, x0 = plane()
    d = forward(q)
    size, ty = np.asarray(tables()["geom_size"], dtype=np.float64), _flat("geom_type")
    low = np.inf
    for g in floor_candidates((4, 5)):
        c, R = d.geom_xpos[g], d.geom_xmat[g]
        every = plane_ellipsoid(n, x0, c, R, size[g], np.inf) if ty[g] == 4 else plane_cylinder(n, x0, c, R, size[g, 0], size[g, 1], np.inf)
        low = min([low] + [dd for _, dd in every])
    q[2] -= low + depth
    return q


def _accept(q):
    """(state accepted?, restated contacts, info): inside the kernel's capacities and clear of every switching distance - the restated
    candidates by `restated_at`, the oracle's own (primitive floor pairs, fly-fly pairs) by its `contact_hist` over one substep."""
    d = forward(q)
    con, clear = restated(q, d)
    keep = matter(con)
    prim = floor_rows(d.contacts())
    total = d.ncon_matter + len(keep)
    # 48 rows in all (3 per floor contact, 1 per fly-fly contact, room for 6 joint limits), and 24 per block of the inertia - a block
    # is the subtree of one child of the thorax - with room for 3 joint limits
    body, rows = _flat("geom_bodyid"), {}
    for r in d.contacts():
        for g in (int(r[0]), int(r[1])):
            if g != floor_geom():
                rows[_block(body[g])] = rows.get(_block(body[g]), 0) + (3 if floor_geom() in (int(r[0]), int(r[1])) else 1)
    for c in keep:
        rows[_block(body[c[0]])] = rows.get(_block(body[c[0]]), 0) + 3
    rows.pop(1, None)  # (a geom of the thorax itself has no hinge: its rows take no column)
    ok = (len(keep) == len(con) and len(keep) >= 1 and total <= 16 and 3 * (len(prim) + len(keep)) + (d.ncon_matter - len(prim)) + 6 <= 48
          and max(list(rows.values()) + [0]) <= 21 and clear >= CLEAR)
    ok = ok and primitive_clearance(d) >= CLEAR
    if ok:
        m = S.model()
        ok = S.oracle_advance(m, (q, np.zeros(m.nv), np.zeros(m.na)), np.zeros(m.nu), 1, 0)[3] >= 10 * S.BAND
    return ok, keep, (total, len(prim), len(keep))


def _block(b):
    """The child of the thorax (body 1) whose subtree holds body `b`; 1 for the thorax itself."""
    par = _flat("body_parentid")
    b = int(b)
    while b != 1 and int(par[b]) != 1:
        b = int(par[b])
    return b


def primitive_clearance(d):
    """How far the 48 (floor, sphere / capsule) candidates stay from a switching distance (margin, or margin - gap) at the pose of `d`:
    mjc_PlaneSphere at the sphere's centre or at both ends of a capsule's segment.  (The oracle's `contact_hist` gives one figure over all
    candidate pairs, and one fly-fly pair that touches in every pose sits 5.05e-5 cm from its switch whatever the pose; the floor's
    candidates are held to CLEAR here and the fly-fly ones to the band of tests/walk_self_sets.py.)"""
    n, x0 = plane()
    size, ty = np.asarray(tables()["geom_size"], dtype=np.float64), _flat("geom_type")
    clear = np.inf
    for g in floor_candidates((2, 3)):
        margin, incl = pair_margin(g)
        half = size[g, 1] if ty[g] == 3 else 0.0
        for e in ((1.0, -1.0) if ty[g] == 3 else (1.0,)):
            dist = float(n @ (d.geom_xpos[g] + e * half * d.geom_xmat[g][:, 2] - x0)) - size[g, 0]
            clear = min(clear, abs(dist - margin), abs(dist - incl))
    return clear


def _cyl(keep):
    """Contacts per touching cylinder."""
    ty, per = _flat("geom_type"), {}
    for c in keep:
        if ty[c[0]] == 5:
            per[c[0]] = per.get(c[0], 0) + 1
    return sorted(per.values())


def _make(kind, n, seed):
    """`n` accepted states; the last ones are drawn from wider ranges until every quota of the kind is met."""
    _, names, _ = S.tables()
    rng = np.random.RandomState(seed)
    ty = _flat("geom_type")
    quota = {"A": {"cyl2": lambda k: 2 in _cyl(k), "cyl4": lambda k: 4 in _cyl(k)},
             "B": {"thorax alone": lambda k: all("thorax" in names[c[0]] for c in k), "wing": lambda k: any("wing" in names[c[0]] for c in k)},
             "C": {"coxa": lambda k: any("coxa" in names[c[0]] for c in k)}}[kind]
    out, met = [], set()
    for _ in range(1500):
        if len(out) >= n:
            break
        missing = [k for k in quota if k not in met]
        wide = len(out) >= n - len(missing)  # only the quota states are left
        if kind == "B":    # on its back: about x by pi +- up to 0.5 rad
            q = tucked().copy() if rng.rand() < 0.5 else S.reset_pose().copy()
            q[3:7] = _quat_xyz(np.pi + rng.uniform(-0.5, 0.5), rng.uniform(-0.15, 0.15), rng.uniform(-3, 3))
            want = lambda keep: True
        elif kind == "A":  # on its abdomen: legs tucked, pitched 10 .. 25 degrees (the quota states: up to 60, the abdomen bent at random)
            q = tucked().copy()
            if wide:
                _, _, jname = S.tables()
                hinge, qa, lo, hi = _hinges()
                q[qa] = np.where([("abdomen" in jname[j]) for j in hinge], rng.uniform(lo, hi), q[qa])
            q[3:7] = _quat_xyz(rng.uniform(-0.1, 0.1), -np.radians(rng.uniform(10, 60) if wide else rng.uniform(10, 25)), rng.uniform(-3, 3))
            want = lambda keep: any(ty[c[0]] == 5 for c in keep)
        else:              # coxae and mouth parts: legs tucked, pitched the other way (rolled too for the quota states)
            q = tucked().copy()
            q[3:7] = _quat_xyz(rng.uniform(-1.5, 1.5) if wide else rng.uniform(-0.1, 0.1), np.radians(rng.uniform(5, 30)), rng.uniform(-3, 3))
            want = lambda keep: any(ty[c[0]] == 4 for c in keep)
        q[:2] = rng.uniform(-1, 1, 2)
        q = _settle(q, rng.uniform(0.005, 0.03) if wide else rng.uniform(0.001, 0.012))
        ok, keep, info = _accept(q)
        fills = [k for k in missing if quota[k](keep)]
        if not ok or not want(keep) or (wide and not fills):
            continue
        met.update(k for k in quota if quota[k](keep))
        m = S.model()
        qv = rng.randn(m.nv) * 0.5
        qv[:6] *= 0.25
        out.append((q, qv, rng.uniform(-0.3, 0.3, m.na), info))
    assert len(out) >= n and not [k for k in quota if k not in met], (kind, len(out), met)
    return out


@functools.lru_cache(maxsize=1)
def set_a():
    return _make("A", 8, 21)


@functools.lru_cache(maxsize=1)
def set_b():
    return _make("B", 8, 22)


@functools.lru_cache(maxsize=1)
def set_c():
    return _make("C", 8, 23)


def get(which):
    return {"A": set_a, "B": set_b, "C": set_c}[which]()


def cylinder_counts(states):
    """Per state, the numbers of contacts its touching cylinders give."""
    return [_cyl(restated(s[0])[0]) for s in states]


def oracle_advance(state, ctrl, nsteps, flags, trace=None):
    """tests/walk_self_sets.py::oracle_advance on the witness blob of `state` (valid for ONE substep: the witness spheres belong to this
    pose).  `trace`, a list, receives a dict of the first substep: `ncon_matter` and `nefc` of the oracle on the witness blob, `nconvex`
    the restated contacts the kernel keeps, `mind` the smaller of the oracle's smallest active contact distance and the restatement's."""
    from oracle import oracle as O

    m, contacts = witness_model(state[0])
    tr = []
    ref = S.oracle_advance(m, state, ctrl, nsteps, flags, trace=tr)
    if trace is not None:
        d = O.OracleData(m)
        d.qpos[:], d.qvel[:], d.act[:] = state[:3]
        d.ctrl[:] = ctrl
        d.forward()
        active = [r[5] for r in d.contacts() if not int(r[3])]
        trace.append({"ncon_matter": tr[0][0], "nefc": tr[0][2], "nconvex": len(matter(contacts)),
                      "mind": min(active + [c[2] for c in matter(contacts)] + [np.inf])})
    return ref


def deepest_sixteen(qpos):
    """(plane-ellipsoid / plane-cylinder contacts among the 16 deepest floor contacts of both kinds at `qpos`, floor contacts of both
    kinds in all, the smallest distance): what the kernel must keep beyond its capacity (the oracle's floor rows and the restatement)."""
    d = forward(qpos)
    con = matter(restated(qpos, d)[0])
    both = sorted([(r[5], 0) for r in floor_rows(d.contacts())] + [(c[2], 1) for c in con])
    assert len(both) < 17 or both[15][0] < both[16][0] - CLEAR  # (the cut is clear of a tie)
    return sum(k for _, k in both[:16]), len(both), both[0][0]


def overflow_mixed():
    """Two belly-down states with tucked legs, level, whose 16 deepest floor contacts are of both kinds and leave out contacts of both
    kinds: at z = 0.05 cm the primitive pass alone stays inside the capacity (9 + 15), at z = 0.03 cm it overflows by itself (22 + 25)."""
    out = []
    for z in (0.05, 0.03):
        q = tucked().copy()
        q[3:7] = _quat_xyz(0.0, 0.0, 0.4)
        q[2] = z
        out.append((q, np.zeros(S.model().nv), np.zeros(S.model().na)))
    return out
