"""CPU-side checks of the floor plane against the walking fly's ellipsoids and cylinders (csrc/walk_full_env.hip `floor_full_step`,
FFE_WALK_FLOOR_CONVEX): the narrow phase (csrc/walk_floor_convex.hpp, in a stand-alone program under
AddressSanitizer and UBSan: tests/walk_floor_convex_host.cpp) against an independent float64 numpy restatement and against geometric
certificates that involve neither; the second floor table; the witness construction that lets the unchanged oracle check the new contacts
end to end (tests/walk_floor_convex_sets.py); the fallen state sets; the interface and the resource figures."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import walk_floor_convex_sets as F
import walk_self_sets as S

# Worst disagreement between the header and the numpy restatement over the random poses (cm), as measured; the bounds are 1e-12 (the
# same arithmetic in double, lengths below 1 cm) and 2e-6 (eps 6e-8 x coordinates <= 0.3 cm x a few dozen operations; also the project's
# switching band).
MEASURED = {"f64": 1.4e-16, "f32": 7.3e-8}
F64_BOUND, F32_BOUND = 1e-12, 2e-6
PER_GEOM = 14   # random poses per shipped geom: 22 x 14 = 308


def _rotation(rng):
    q = rng.randn(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _all(ty, n, x0, c, R, size, margin):
    return F.plane_ellipsoid(n, x0, c, R, size, margin) if ty == 4 else F.plane_cylinder(n, x0, c, R, size[0], size[1], margin)


@pytest.fixture(scope="module")
def poses():
    """[(type, n, x0, c, R, size, margin)]: every shipped candidate geom at random orientations over a random plane, the lowest point
    between 0.8 x the smallest size below the plane and 0.1 x above it, every contact distance at least 1e-4 cm from the margin, a
    cylinder's axis at least 1 degree from the normal; then the exactly parallel cylinders."""
    rng = np.random.RandomState(7)
    t = F.tables()
    size, ty = np.asarray(t["geom_size"], dtype=np.float64), F._flat("geom_type")
    out = []
    for g in F.floor_candidates((4, 5)):
        margin = F.pair_margin(g)[0]
        k = 0
        while k < PER_GEOM:
            n = rng.randn(3); n /= np.linalg.norm(n)
            x0, R = rng.uniform(-0.1, 0.1, 3), _rotation(rng)
            smallest = size[g][size[g] > 0].min()
            if ty[g] == 5:  # half of a cylinder's poses with the axis within 15 degrees of the normal, where all four contacts occur
                th = np.radians(rng.uniform(1.0, 15.0) if k % 2 else rng.uniform(1.0, 90.0))
                perp = np.cross(n, rng.randn(3)); perp /= np.linalg.norm(perp)
                R[:, 2] = (np.cos(th) * n + np.sin(th) * perp) * rng.choice([-1.0, 1.0])
                R[:, 0] = np.cross(R[:, 2], rng.randn(3)); R[:, 0] /= np.linalg.norm(R[:, 0])
                R[:, 1] = np.cross(R[:, 2], R[:, 0])
                assert abs(n @ R[:, 2]) <= np.cos(np.radians(1.0)) + 1e-12
                smallest = max(1.5 * size[g, 0] * np.sin(th), 2 * size[g, 1] * np.cos(th)) * 1.5  # (what separates one contact from four)
            low = min(d for _, d in _all(ty[g], n, x0, np.zeros(3), R, size[g], np.inf))
            c = n * (rng.uniform(-0.8, 0.1) * smallest - low)
            if min(abs(d - margin) for _, d in _all(ty[g], n, x0, c, R, size[g], np.inf)) < 1e-4:
                continue
            out.append((int(ty[g]), n, x0, c, R, size[g].copy(), margin))
            k += 1
    nrandom = len(out)
    z = np.array([0.0, 0.0, 1.0])
    for flip in (1.0, -1.0):  # the disk exactly parallel to the plane, axis along and against the normal, shallow and deep
        for depth in (0.3, 2.5):
            R = np.diag([1.0, flip, flip])
            out.append((5, z, np.zeros(3), z * (0.0142 - depth * 0.0142), R, np.array([0.0367, 0.0142, 0.0]), 0.0))
    return out, nrandom


@pytest.fixture(scope="module")
def host(tmp_path_factory, poses):
    """tests/walk_floor_convex_host.cpp built with -fsanitize=address,undefined and run on its own (never loaded into Python)."""
    tmp = tmp_path_factory.mktemp("walk_floor_convex")
    exe, pin, pout = str(tmp / "walk_floor_convex_host"), str(tmp / "poses.bin"), str(tmp / "out.bin")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "walk_floor_convex_host.cpp")])
    rows = [np.concatenate([[float(ty)], n, x0, c, R.ravel(), size, [margin]]) for ty, n, x0, c, R, size, margin in poses[0]]
    np.concatenate([[float(len(rows))]] + rows).tofile(pin)
    r = subprocess.run([exe, S.WALK_BLOB, pin, pout], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr  # a sanitizer report ends the program with a non-zero status
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    rep = dict(line.split(None, 1) for line in r.stdout.splitlines())
    out = np.fromfile(pout).reshape(len(rows), 2, 17)
    return rep, out


def _contacts(rec):
    """[(pos, dist)] of one record of out.bin, in slot order."""
    mask = int(rec[0])
    return [(rec[1 + 4 * e: 4 + 4 * e], float(rec[4 + 4 * e])) for e in range(4) if (mask >> e) & 1]


@pytest.mark.parametrize("tag,bound", [("f64", F64_BOUND), ("f32", F32_BOUND)])
def test_header_equals_the_restatement(host, poses, tag, bound):
    (all_poses, nrandom), (_, out) = poses, host
    worst, counts = 0.0, {}
    for i in range(nrandom):
        ty, n, x0, c, R, size, margin = all_poses[i]
        want, got = _all(ty, n, x0, c, R, size, margin), _contacts(out[i, 0 if tag == "f64" else 1])
        assert len(want) == len(got), (i, ty, len(want), len(got))
        counts[(ty, len(want))] = counts.get((ty, len(want)), 0) + 1
        for (pw, dw), (pg, dg) in zip(want, got):
            worst = max(worst, abs(dw - dg), float(np.abs(pw - pg).max()))
    print(f"{tag}: worst difference {worst:.3e} cm over {nrandom} poses (recorded: {MEASURED[tag]:.1e}); (type, contacts) -> poses {counts}")
    assert nrandom == 22 * PER_GEOM
    assert all(counts.get(k, 0) >= 5 for k in ((4, 0), (4, 1), (5, 0), (5, 1), (5, 2), (5, 3), (5, 4))), counts
    assert worst <= bound


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_the_parallel_disk(host, poses, tag):
    """Axis exactly along or against the normal: checked by counts, equal distances and rim membership only (the direction of the first
    rim point is a convention there)."""
    (all_poses, nrandom), (_, out) = poses, host
    tol = 1e-12 if tag == "f64" else 2e-6
    for i in range(nrandom, len(all_poses)):
        ty, n, x0, c, R, size, margin = all_poses[i]
        got = _contacts(out[i, 0 if tag == "f64" else 1])
        deep = (c @ n) + size[1] <= 0  # the upper disk is below the plane too
        assert len(got) == (4 if deep else 3), (i, len(got))
        lower = [g for k, g in enumerate(got) if not (deep and k == 1)]
        assert max(abs(d - lower[0][1]) for _, d in lower) <= tol
        for p, d in got:
            s = p + n * d / 2 - c
            assert abs(np.hypot(s[0], s[1]) - size[0]) <= tol and abs(abs(s[2]) - size[1]) <= tol and abs((p + n * d / 2 - x0) @ n - d) <= tol


def _dense_sphere(k=200):
    u = np.linspace(0, np.pi, k)[:, None]
    v = np.linspace(0, 2 * np.pi, 2 * k)[None, :]
    return np.stack([np.sin(u) * np.cos(v), np.sin(u) * np.sin(v), np.cos(u) * np.ones_like(v)], axis=-1).reshape(-1, 3)


@pytest.mark.parametrize("source", ["header", "restatement"])
def test_certificates(host, poses, source):
    """What a correct answer must satisfy, whoever computed it.  Ellipsoid: the surface point pos + n dist / 2 lies on the surface, the
    surface gradient there is antiparallel to n, no point of a dense surface sample is lower.  Cylinder: every surface point lies on a
    rim (radial distance r, axial +-h), its dist is its plane distance, contact 1 is the minimum over a dense rim sample, contacts 3 and
    4 are mirror images across the plane spanned by n and the axis."""
    (all_poses, nrandom), (_, out) = poses, host
    sphere = _dense_sphere()
    ang = np.linspace(0, 2 * np.pi, 20000, endpoint=False)
    checked = {4: 0, 5: 0, "pair": 0}
    for i in range(nrandom):
        ty, n, x0, c, R, size, margin = all_poses[i]
        got = _contacts(out[i, 0]) if source == "header" else _all(ty, n, x0, c, R, size, margin)
        if not got:
            continue
        if ty == 4:
            (p, d), = got
            s = p + n * d / 2
            loc = R.T @ (s - c)
            assert abs(np.linalg.norm(loc / size) - 1.0) <= 1e-12
            grad = R @ (loc / size ** 2)
            assert np.linalg.norm(np.cross(grad / np.linalg.norm(grad), n)) <= 1e-9 and grad @ n < 0
            assert abs((s - x0) @ n - d) <= 1e-14
            sample = c + (sphere * size) @ R.T
            assert ((sample - x0) @ n).min() >= d - 1e-12  # (the sample lies on the surface: none of it may be below the support point)
            assert ((sample - x0) @ n).min() <= d + 1e-3 * size.max()
        else:
            r, h, a = size[0], size[1], R[:, 2]
            rim = lambda sgn: c + sgn * h * a + r * (np.cos(ang)[:, None] * R[:, 0] + np.sin(ang)[:, None] * R[:, 1])
            lowest = min(((rim(1.0) - x0) @ n).min(), ((rim(-1.0) - x0) @ n).min())
            for k, (p, d) in enumerate(got):
                s = p + n * d / 2
                loc = R.T @ (s - c)
                assert abs(np.hypot(loc[0], loc[1]) - r) <= 1e-12 and abs(abs(loc[2]) - h) <= 1e-12
                assert abs((s - x0) @ n - d) <= 1e-14
            assert got[0][1] <= lowest + 1e-14 and lowest <= got[0][1] + r * (2 * np.pi / len(ang)) ** 2
            if len(got) >= 3:
                s3, s4 = got[-2][0] + n * got[-2][1] / 2, got[-1][0] + n * got[-1][1] / 2
                m = np.cross(n, a); m /= np.linalg.norm(m)  # the normal of the plane spanned by n and the axis
                assert np.abs((s3 - c) - 2 * ((s3 - c) @ m) * m - (s4 - c)).max() <= 1e-12 and abs(got[-2][1] - got[-1][1]) <= 1e-14
                checked["pair"] += 1
        checked[ty] += 1
    print(source, checked)
    assert checked[4] >= 50 and checked[5] >= 30 and checked["pair"] >= 10


def test_second_floor_table(host):
    """Exactly the 22 ellipsoids and cylinders that pass MuJoCo's pair filter against the floor, in model order; the two thorax
    ellipsoids have no link; WalkExtra's bytes and the 48 rows of the first table are untouched."""
    rep, _ = host
    t, names, _ = S.tables()
    want = F.floor_candidates((4, 5))
    assert len(want) == 22 and int(rep["table_rows"]) == 22 and rep["table_ok"] == "1" and rep["params_ok"] == "1"
    rows = [list(map(int, rep[f"row{s}"].split())) for s in range(22)]
    ty, body = F._flat("geom_type"), F._flat("geom_bodyid")
    assert [r[0] for r in rows] == want and [r[1] for r in rows] == [int(ty[g]) for g in want]
    assert sorted(ty[want].tolist()) == [4] * 16 + [5] * 6
    for g, kind, link, adh, blk, amask in rows:
        if body[g] == 1:
            assert "thorax" in names[g] and (link, adh, blk, amask) == (-1, -1, 255, 0)
        else:
            assert 0 <= link < 64 and 0 <= blk < 12 and amask > 0 and adh == -1
    assert sum(1 for r in rows if r[2] < 0) == 2
    # rows of one body subtree share a block, rows of different subtrees do not
    blocks = {}
    for g, kind, link, adh, blk, amask in rows:
        if link >= 0:
            blocks.setdefault(F._block(body[g]), set()).add(blk)
    assert all(len(v) == 1 for v in blocks.values()) and len({next(iter(v)) for v in blocks.values()}) == len(blocks)
    assert rep["extra_untouched"] == "1" and int(rep["first_table_rows"]) == 48
    assert [int(rep[f"first{s}"].split()[0]) for s in range(48)] == F.floor_candidates((2, 3))


@pytest.mark.parametrize("which", ["A", "B", "C"])
def test_state_sets_and_witness_construction(which):
    """Every state: at most 16 contacts in all (the oracle's `ncon_matter` on the shipped blob plus the restated contacts), clear of every
    switching distance.  The oracle on the witness blob reports each wanted contact with dist / pos within 1e-12, its fly-fly contact list
    is the shipped blob's, and its `ncon_matter` is the sum."""
    from oracle import oracle as O

    states = F.get(which)
    assert len(states) >= 8
    names = S.tables()[1]
    seen = set()
    for s in states:
        d0 = F.forward(s[0])
        con, clear = F.restated(s[0], d0)
        keep = F.matter(con)
        assert len(keep) == len(con) >= 1 and d0.ncon_matter + len(con) <= 16 and clear >= F.CLEAR and F.primitive_clearance(d0) >= F.CLEAR
        seen |= {names[c[0]].replace("_collision", "") for c in con}
        m, _ = F.witness_model(s[0], con)
        assert m.ngeom == 71 + len(con)
        d = O.OracleData(m)
        d.qpos[:] = s[0]; d.qvel[:] = 0; d.act[:] = 0; d.ctrl[:] = 0
        d.forward()
        rows, rows0 = d.contacts(), d0.contacts()
        wit = [r for r in rows if max(int(r[0]), int(r[1])) >= 71]
        assert [max(int(r[0]), int(r[1])) for r in wit] == list(range(71, 71 + len(con)))
        for r, (g, p, dist, _) in zip(wit, con):
            assert abs(r[5] - dist) <= 1e-12 and np.abs(r[6:9] - p).max() <= 1e-12 and int(r[2]) == 3 and not int(r[3])
        rest = [r for r in rows if max(int(r[0]), int(r[1])) < 71]
        assert len(rest) == len(rows0) and all(np.array_equal(a[[0, 1, 2, 3, 5]], b[[0, 1, 2, 3, 5]]) for a, b in zip(rest, rows0))
        assert d.ncon_matter == d0.ncon_matter + len(con)
        ref = F.oracle_advance(s, np.zeros(59), 1, 0)
        assert ref[3] >= 10 * S.BAND  # (the fly-fly candidates: one pair that always touches sits 5.05e-5 cm from its switch)
    print(which, sorted(seen), F.cylinder_counts(states))
    if which == "A":
        cyl = [k for c in F.cylinder_counts(states) for k in c]
        assert 2 in cyl and 4 in cyl
    if which == "B":
        assert any("thorax" in x for x in seen) and any("wing" in x for x in seen)
    if which == "C":
        assert any("coxa" in x for x in seen) and any(x.startswith(("labrum", "rostrum")) for x in seen)


def test_standing_and_lifted_sets_have_no_plane_convex_contact():
    for s in S.r10() + S.x_lifted() + S.x_standing():
        assert not F.restated(s[0])[0]


def test_interface():
    from flybody_amd import batched_env, build, fly_envs

    hdr = open(os.path.join(ROOT, "include", "flybody_env.h")).read()
    assert re.search(r"\bFFE_WALK_FLOOR_CONVEX\s*=\s*32768\b", hdr) and batched_env.FFE_WALK_FLOOR_CONVEX == 32768 == F.WALK_FLOOR_CONVEX
    assert "FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS | FFE_WALK_FLOOR | FFE_WALK_SELF | FFE_WALK_FLOOR_CONVEX\n" in hdr
    assert "created with FFE_WALK_FLOOR_CONVEX reports" in hdr and "real 2" in hdr and "tasks/base.py:331-364" in hdr
    p = inspect.signature(batched_env.BatchedWalkPhysics.__init__).parameters["floor_convex"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    for kw in ({}, {"floor_contacts": True}):  # before any device call
        with pytest.raises(ValueError, match="floor_convex"):
            batched_env.BatchedWalkPhysics(batch_size=1, floor_convex=True, **kw)
    assert "floor_convex=True" in batched_env.BatchedWalkPhysics.__doc__
    unit = "walk_full_env.hip"
    assert unit in build.SOURCES and build.PER_SOURCE_FLAGS[unit] == build.PER_SOURCE_FLAGS["walk_self_env.hip"]
    assert "walk_floor_convex.hpp" in build.HEADERS
    # nothing else changes: the default factory call and floor_contacts=True keep raising, "all" stays a ValueError
    with pytest.raises(NotImplementedError, match="floor contacts"):
        fly_envs.walk_imitation()
    with pytest.raises(NotImplementedError, match="floor contacts"):
        fly_envs.walk_imitation(floor_contacts=True)
    with pytest.raises(ValueError):
        fly_envs.walk_imitation(floor_contacts="all")


def _tiles(src):
    from flybody_amd import build

    return {k: u for k, u in build.kernel_resource_usage(src, "").items() if u.get("LDS Size", 0) > 0}


def test_kernel_inside_the_resource_targets():
    """One kernel with an LDS tile in the new unit, with a name the older tests do not count: tile <= 20 480 B, two waves per SIMD, no
    VGPR spill."""
    use = _tiles("walk_full_env.hip")
    assert len(use) == 1, sorted(use)
    (name, u), = use.items()
    print(name, u)
    assert "floor_full_step" in name and "walk_" not in name and "_kernel" not in name and not re.search(r"\dfloor_stepE", name), name
    assert u["LDS Size"] <= 20480 and u["Occupancy"] == 2 and u["VGPRs Spill"] == 0


def test_the_seven_kernels_before_it_keep_the_parents_figures():
    """The figures each step recorded in DESIGN.md section 12, as the tests of those steps pin them."""
    from test_walk_self_cpu import PARENT
    from test_walk_self_env_cpu import NEW, PARENT_SELF

    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "20 176 B LDS" in design and "20 416 B" in design
    use = {**_tiles("walk_env.hip"), **_tiles("walk_floor_env.hip")}
    assert len(use) == 5, sorted(use)
    for name, ref in PARENT.items():
        (u,) = [u for k, u in use.items() if re.search(r"\d" + name + "E", k)]
        assert {k: u[k] for k in ref} == ref, (name, u)
    (u,) = _tiles("walk_self_env.hip").values()
    assert {k: u[k] for k in PARENT_SELF} == PARENT_SELF, u
    (u,) = _tiles("walk_imit_self_env.hip").values()
    assert {k: u[k] for k in NEW} == NEW, u
