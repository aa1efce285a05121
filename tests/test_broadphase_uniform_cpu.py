"""The flight broad phase's uniform support function (flybody_amd/csrc/convex.hpp: ushape, GeomU, hsupport_u, overlap_u,
separation_bound_u, compiled for the host with -DCVX_HOST by tests/cvx_uniform_host.cpp) against the per-type originals the narrow
phase and walk_on_ball keep using, and its separating-direction bound against the float64 oracle.  Runs without a GPU.

 * support value and core segment of all 70 flight geoms over random directions, directions along a cylinder's axis included:
   the per-type `support` / `core_segment` and the float64 support value to float32 rounding;
 * on states of an oracle rollout of the flight task: `separation_bound_u` never exceeds the oracle's distance (it never culls a
   touching pair), and it and `overlap_u` agree with the originals to float32 rounding.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle.oracle import _dp
from test_convex_f32_cpu import _rec, _rollout

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HERE = os.path.dirname(os.path.abspath(__file__))
fp = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cvxu") / "libcvx_uniform_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", out, os.path.join(HERE, "cvx_uniform_host.cpp")])
    L = C.CDLL(out)
    for f in ("cvxu_hsupport", "cvxu_overlap", "cvxu_overlap_ref", "cvxu_separation_bound", "cvxu_separation_bound_ref"):
        getattr(L, f).restype = C.c_float
    return L


@pytest.fixture(scope="module")
def geoms():
    from flybody_amd.model.blob import read_blob

    t = read_blob(os.path.join(ROOT, "flybody_amd", "assets", "fly_flight.ffmb"))
    return np.asarray(t["geom_type"]).astype(int), np.asarray(t["geom_size"]).reshape(-1, 3)


def _ptr(a):
    return a.ctypes.data_as(fp)


def _rot(q):
    w, x, y, z = q
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def test_ushape_constants(lib, geoms):
    """The per-geom table: radii, segment half-length and core segment of each type (the kernel's cg_ush rows)."""
    gt, gs = geoms
    assert len(gt) == 70 and set(gt) == {2, 3, 4, 5}
    out = np.zeros(8, np.float32)
    for t, s in zip(gt, gs.astype(np.float32)):
        lib.cvxu_ushape(int(t), C.c_float(s[0]), C.c_float(s[1]), C.c_float(s[2]), _ptr(out))
        r = s[0]
        if t == 4:
            k = int(np.argmax(s))
            want = [s[0], s[1], s[2], 0, k == 0, k == 1, k == 2, s.max() - np.sort(s)[1]]
        else:
            want = [r, r, 0 if t == 5 else r, s[1] if t in (3, 5) else 0, 0, 0, 1, s[1] if t in (3, 5) else 0]
        np.testing.assert_allclose(out, np.asarray(want, np.float32), rtol=0, atol=1e-8, err_msg=str((t, s)))


def _hsupport64(rec, t, s, n):
    """float64 support value of the geom record in the direction n"""
    q = rec[3:7].astype(np.float64)
    l = _rot(q / np.linalg.norm(q)).T @ n
    e = {2: (s[0], s[0], s[0], 0.0), 3: (s[0], s[0], s[0], s[1]), 4: (s[0], s[1], s[2], 0.0), 5: (s[0], s[0], 0.0, s[1])}[t]
    return n @ rec[:3].astype(np.float64) + np.linalg.norm(np.asarray(e[:3]) * l) + e[3] * abs(l[2])


def test_support_matches_per_type(lib, geoms):
    gt, gs = geoms
    rng = np.random.RandomState(7)
    sr, cu = np.zeros(3, np.float32), np.zeros(8, np.float32)
    worst_r = worst_h = worst_k = 0.0
    ncyl_axis = 0
    for g in range(len(gt)):
        for _ in range(40):
            q = rng.normal(size=4)
            q /= np.linalg.norm(q)
            rec = _rec(rng.uniform(-0.3, 0.3, 3), _rot(q), gs[g], gt[g])  # (cm: the size of the fly's world coordinates)
            R = _rot(rec[3:7].astype(np.float64))
            dirs = [rng.normal(size=3) for _ in range(30)]
            dirs += [R[:, 2], -R[:, 2]]  # along the local z axis: a cylinder's flat face, a capsule's cap
            dirs += [R[:, 2] + 1e-7 * rng.normal(size=3) for _ in range(3)]  # and within float32 rounding of it
            for n in dirs:
                n = np.asarray(n / np.linalg.norm(n), np.float32)
                n64 = n.astype(np.float64)
                lib.cvxu_support_ref(_ptr(rec), _ptr(n), _ptr(sr))
                h64 = _hsupport64(rec, int(gt[g]), gs[g], n64)
                h = lib.cvxu_hsupport(_ptr(rec), _ptr(n)) + n64 @ rec[:3].astype(np.float64)
                worst_h = max(worst_h, abs(h - h64))
                # n within rounding of a cylinder's axis: the per-type path takes a point on the rim in the direction of the rounding
                # noise, up to 1e-6 cm above the support value (still a rigorous bound; the uniform form has the whole face)
                on_axis = gt[g] == 5 and abs(abs(float(n64 @ R[:, 2])) - 1.0) < 1e-6
                ncyl_axis += on_axis
                if not on_axis:
                    worst_r = max(worst_r, abs(h - n64 @ sr.astype(np.float64)))
                else:
                    assert h <= n64 @ sr.astype(np.float64) + 1e-7
            lib.cvxu_core(_ptr(rec), _ptr(cu))
            worst_k = max(worst_k, np.abs(cu[:3] - cu[4:7]).max(), abs(cu[3] - cu[7]))
    assert ncyl_axis > 100
    assert worst_r < 1.5e-7 and worst_h < 1.5e-7 and worst_k < 1e-7, (worst_r, worst_h, worst_k)


def test_bound_on_flight_rollout(lib):
    from flybody_amd.model.blob import read_blob

    m, env, draw = _rollout("flight")
    t = read_blob(os.path.join(ROOT, "flybody_amd", "assets", "fly_flight.ffmb"))
    gt, gs, gm = np.asarray(t["geom_type"]), np.asarray(t["geom_size"]).reshape(-1, 3), np.asarray(t["geom_margin"])
    g1s, g2s, gl = np.asarray(t["cand_g1"]), np.asarray(t["cand_g2"]), np.asarray(t["cgeom_link"])
    pairs = [(int(a), int(b)) if gt[a] <= gt[b] else (int(b), int(a)) for a, b in zip(g1s, g2s) if gl[a] != gl[b]]
    env.reset()
    d = env.data
    ng = len(gt)
    n, p = np.zeros(3), np.zeros(3)
    rng = np.random.RandomState(1)
    nbound = nnear = 0
    worst_b = worst_o = 0.0
    for step in range(40):
        env.step(draw())
        xp = np.ctypeslib.as_array(m.L.fo_geom_xpos(d.ptr), (3 * ng,)).reshape(ng, 3).copy()
        xm = np.ctypeslib.as_array(m.L.fo_geom_xmat(d.ptr), (9 * ng,)).reshape(ng, 3, 3).copy()
        for a, b in pairs:
            if np.linalg.norm(xp[a] - xp[b]) > 0.12:
                continue
            ra, rb = _rec(xp[a], xm[a], gs[a], gt[a]), _rec(xp[b], xm[b], gs[b], gt[b])
            bound = lib.cvxu_separation_bound(_ptr(ra), _ptr(rb))
            d64 = m.L.fo_convex_distance(m.ptr, d.ptr, a, b, _dp(n), _dp(p))
            assert bound <= d64 + 1e-6, (a, b, bound, d64)  # a lower bound: it never culls a touching pair
            nbound += 1
            nnear += d64 <= max(gm[a], gm[b]) + 1e-3
            worst_b = max(worst_b, abs(bound - lib.cvxu_separation_bound_ref(_ptr(ra), _ptr(rb))))
            u = np.asarray(rng.normal(size=3), np.float32)
            u /= np.linalg.norm(u)
            worst_o = max(worst_o, abs(lib.cvxu_overlap(_ptr(ra), _ptr(rb), _ptr(u)) - lib.cvxu_overlap_ref(_ptr(ra), _ptr(rb), _ptr(u))))
    assert nbound > 2000 and nnear > 30, (nbound, nnear)
    assert worst_b < 2e-7 and worst_o < 2e-7, (worst_b, worst_o)
    print(f"flight: {nbound} bounds ({nnear} pairs within 1e-3 of their margin), worst |bound - per-type bound| {worst_b:.1e}, |overlap - per-type| {worst_o:.1e}")
