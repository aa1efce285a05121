"""CPU-side checks of the floor contacts of the free-root walking-fly physics (csrc/walk_env.hip `floor_step`; DESIGN.md section 12 step
3b): the opt-in bit and the keyword exist, the fourth step kernel sits inside its resource targets under a name the older tests do not
count, and the formulas behind it (csrc/walk_floor.hpp) and the floor tables of the walk builder agree with the float64 oracle's contacts
and constraint rows.  The formulas run in a stand-alone program under AddressSanitizer and UBSan (tests/walk_floor_host.cpp)."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import walk_floor_sets as S

QUANTITIES = ("dist", "pos", "normal", "includemargin", "friction", "D", "aref", "J", "G", "y0")
# Worst float32 errors the host program measured on F06 + F10 (48 states, 196 contacts, 543 rows), each relative to the largest
# |reference| of its quantity (dist: 7e-4 cm, so 2.5e-5 of it is 2e-8 cm).  Asserted at 3x.  In float64 the same program stays below
# 1e-10 on every quantity.
F32_MEASURED = {"dist": 2.6e-5, "pos": 2.7e-7, "normal": 2.4e-7, "includemargin": 0.0, "friction": 0.0, "D": 4.5e-7, "aref": 7.9e-6, "J": 2.4e-7,
                "G": 6.8e-7, "y0": 2.1e-6}


def test_header_bit_and_keyword():
    from flybody_amd import batched_env

    hdr = open(os.path.join(ROOT, "include", "flybody_env.h")).read()
    assert re.search(r"\bFFE_WALK_FLOOR\s*=\s*2048\b", hdr)
    assert batched_env.FFE_WALK_FLOOR == 2048
    sig = inspect.signature(batched_env.BatchedWalkPhysics.__init__)
    assert sig.parameters["floor_contacts"].default is False and sig.parameters["joint_limits"].default is False
    from flybody_amd import build

    assert "walk_floor.hpp" in build.HEADERS


def test_walk_imitation_keeps_raising():
    from flybody_amd import fly_envs

    with pytest.raises(NotImplementedError, match="floor contacts"):
        fly_envs.walk_imitation()


@pytest.fixture(scope="module")
def tile_kernels():
    from flybody_amd import build

    use = build.kernel_resource_usage("walk_env.hip", "")
    return {k: u for k, u in use.items() if u.get("LDS Size", 0) > 0}


def test_floor_kernel_inside_the_resource_targets(tile_kernels):
    """The fourth kernel with an LDS tile: tile <= 20 480 B, two waves per SIMD, no VGPR spill."""
    assert len(tile_kernels) == 4, sorted(tile_kernels)
    (name, u), = [(k, u) for k, u in tile_kernels.items() if "floor_step" in k]
    print(name, u)
    assert u["LDS Size"] <= 20480 and u["Occupancy"] == 2 and u["VGPRs Spill"] == 0


def test_floor_kernel_name_is_not_counted_by_the_older_tests(tile_kernels):
    """tests/test_walk_limits_cpu.py and tests/test_walk_episode_cpu.py count the tile-owning kernels of walk_env.hip by `walk_` and
    `_kernel` in the mangled name, argument types included."""
    (name,) = [k for k in tile_kernels if "floor_step" in k]
    assert "walk_" not in name and "_kernel" not in name, name
    assert len([k for k in tile_kernels if "walk_" in k]) == 2 and len([k for k in tile_kernels if "_kernel" in k]) == 3


@pytest.fixture(scope="module")
def host_report(tmp_path_factory):
    """tests/walk_floor_host.cpp built with -fsanitize=address,undefined and run on its own (never loaded into Python) on F06 + F10."""
    from oracle import oracle as O
    from flybody_amd.model.blob import read_blob

    tmp = tmp_path_factory.mktemp("walk_floor")
    exe, states = str(tmp / "walk_floor_host"), str(tmp / "states.bin")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "walk_floor_host.cpp")])
    m, F06, F10 = S.sets()
    t = read_blob(S.floor_only_blob())
    ty, body = np.asarray(t["geom_type"]).ravel(), np.asarray(t["geom_bodyid"]).ravel()
    d = O.OracleData(m)
    buf, ncons, nefcs = [], [], []
    for s in F06 + F10:
        d.qpos[:], d.qvel[:], d.act[:] = s
        d.ctrl[:] = 0
        d.forward()
        cons, (J, aref, D, _), M = d.contacts(), d.efc(), d.dense_M()
        ncons.append(d.ncon)
        nefcs.append(d.nefc)
        rec = [d.qpos.copy(), d.qvel.copy(), M.ravel(), d.qacc_smooth.copy(), d.xpos.ravel().copy(), d.xquat.ravel().copy(), [float(d.ncon)]]
        rows = []
        for c in cons:  # rows: geom1, geom2, dim, exclude, efc_adr, dist, pos[3], normal[3], mu, friction, includemargin, normal force
            g1, g2 = int(c[0]), int(c[1])
            assert body[g1] == 0 and ty[g1] == 0 and body[g2] > 1 and ty[g2] in (2, 3) and int(c[2]) == 3  # floor against sphere / capsule only
            rec.append([c[4], c[5], *c[6:9], *c[9:12], c[14], c[13]])
            if c[4] >= 0:
                rows += [int(c[4]), int(c[4]) + 1, int(c[4]) + 2]
        for r in rows:
            rec += [J[r], [aref[r], D[r]]]
        Jc = J[rows]
        rec.append((Jc @ np.linalg.solve(M, Jc.T)).ravel())
        buf.append(np.concatenate([np.asarray(x, dtype=np.float64).ravel() for x in rec]))
    assert 2 <= min(ncons) and max(ncons) <= 6 and 7 <= min(nefcs) and max(nefcs) <= 18, (ncons, nefcs)
    np.concatenate([[float(len(buf))]] + buf).tofile(states)
    r = subprocess.run([exe, S.floor_only_blob(), states], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr  # a sanitizer report ends the program with a non-zero status
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    print(r.stdout)
    rep = dict(line.split(None, 1) for line in r.stdout.splitlines())
    rep["oracle_contacts"] = sum(ncons)
    return rep


def test_floor_tables_are_the_48_pairs_the_oracle_collides(host_report):
    assert S.model().npair == 48 and int(host_report["floor_geoms"]) == 48 and host_report["floor_tables_ok"] == "1"
    from oracle import oracle as O

    assert O.OracleModel(S.WALK_BLOB).npair == 2336  # the committed blob: the fly's own pairs too


def test_reach_bound_covers_every_geom(host_report):
    """`f_reach`, above which a floor substep runs the limits kernel's code, is a bound over all joint angles: on the rollout states no
    geom's surface + margin comes near it, and it stays below the 1 cm of the no-floor-in-reach test and above the standing height."""
    reach, far = float(host_report["floor_reach"]), float(host_report["f64_farthest"])
    print(f"reach bound {reach:.4f} cm, farthest geom surface + margin on F06 + F10 {far:.4f} cm")
    assert 0.14 < far <= reach < 1.0


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_every_contact_and_row_is_found(host_report, tag):
    rep = host_report
    assert int(rep[tag + "_states"]) == 48 and int(rep[tag + "_contacts"]) == rep["oracle_contacts"]
    assert rep[tag + "_count_match"] == "1" and rep[tag + "_unmatched"] == "0"
    assert int(rep[tag + "_rows"]) >= 3 * 48 * 2 and int(rep[tag + "_most_contacts"]) == 6


def test_formulas_equal_the_oracle_in_float64(host_report):
    for k in QUANTITIES:
        print(f"{k}: float64 relative error {float(host_report['f64_' + k]):.3e}")
    for k in QUANTITIES:
        assert float(host_report["f64_" + k]) <= 1e-10, (k, host_report["f64_" + k])


def test_formulas_in_float32(host_report):
    for k in QUANTITIES:
        e = float(host_report["f32_" + k])
        print(f"{k}: float32 relative error {e:.3e} (measured {F32_MEASURED[k]:.1e})")
        assert e <= 3 * F32_MEASURED[k], (k, e)
