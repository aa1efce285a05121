"""CPU-side checks of the walk_imitation environment with every contact of the reference's task (csrc/walk_imit_full_env.hip
`imitation_full_step`, FFE_WALK_EPISODES | FFE_WALK_FLOOR | FFE_WALK_SELF | FFE_WALK_SELF_EPISODES | FFE_WALK_FLOOR_CONVEX; DESIGN.md
section 12 step 4e): the keyword exists on the env and on the factory, the ninth free-root step kernel fits its tile in a translation
unit of its own while the eight before it keep the parent commit's resource figures, the fixtures of tests/test_gpu_walk_full_env.py are
what they claim to be (with the float64 oracle alone), and the sensor pass with plane-ellipsoid contacts among the floor's slots agrees
with the oracle (tests/walk_full_sense_host.cpp, a stand-alone program under AddressSanitizer and UBSan)."""
import functools
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import walk_floor_convex_sets as F
import walk_full_env_samples as X
import walk_self_sets as S
from test_walk_self_env_cpu import _sensor_record

UNIT = "walk_imit_full_env.hip"
# The eight older tile kernels as the parent commit compiles them (`build.kernel_resource_usage(unit, "")` run on the parent before
# anything was edited), by the kernel's name in its mangled form
PARENT8 = {
    ("walk_env.hip", "16walk_step_kernelE"): {"VGPRs": 168, "SGPRs Spill": 26, "VGPRs Spill": 0, "ScratchSize": 0, "LDS Size": 18240, "Occupancy": 2},
    ("walk_env.hip", "18walk_limits_kernelE"): {"VGPRs": 256, "SGPRs Spill": 57, "VGPRs Spill": 0, "ScratchSize": 112, "LDS Size": 18800, "Occupancy": 2},
    ("walk_env.hip", "10floor_stepE"): {"VGPRs": 256, "SGPRs Spill": 125, "VGPRs Spill": 0, "ScratchSize": 368, "LDS Size": 19872, "Occupancy": 2},
    ("walk_env.hip", "21imitation_step_kernelE"): {"VGPRs": 256, "SGPRs Spill": 109, "VGPRs Spill": 0, "ScratchSize": 112, "LDS Size": 19712, "Occupancy": 2},
    ("walk_floor_env.hip", "20imitation_floor_stepE"): {"VGPRs": 256, "SGPRs Spill": 180, "VGPRs Spill": 0, "ScratchSize": 368, "LDS Size": 20304, "Occupancy": 2},
    ("walk_self_env.hip", "15floor_self_stepE"): {"VGPRs": 256, "SGPRs Spill": 151, "VGPRs Spill": 0, "ScratchSize": 368, "LDS Size": 20176, "Occupancy": 2},
    ("walk_imit_self_env.hip", "19imitation_self_stepE"): {"VGPRs": 256, "SGPRs Spill": 204, "VGPRs Spill": 0, "ScratchSize": 368, "LDS Size": 20416, "Occupancy": 2},
    ("walk_full_env.hip", "15floor_full_stepE"): {"VGPRs": 256, "SGPRs Spill": 170, "VGPRs Spill": 0, "ScratchSize": 368, "LDS Size": 20176, "Occupancy": 2},
}
# the figures the build reaches for the new kernel: recorded; the test bounds LDS, VGPR spill and occupancy
NEW = {"VGPRs": 256, "SGPRs Spill": 222, "VGPRs Spill": 0, "ScratchSize": 368, "LDS Size": 20416, "Occupancy": 2}
# Worst float32 errors the host program measured on the 28 round samples, relative to max(1, largest |reference|); the bound is 3 x these
F32_MEASURED = {"force": 9.5e-8, "touch": 1.3e-9}  # (measured 9.403e-8 and 1.235e-9)


# ------------------------------------------------------------------------------------------------ interface
def test_interface():
    from flybody_amd import batched_env, build, fly_envs

    for fn in (batched_env.BatchedWalkEnv.__init__, fly_envs.walk_imitation):
        p = inspect.signature(fn).parameters["floor_convex"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    view, refs = X.world()
    for kw in ({}, {"floor_contacts": True}):  # before any device call
        with pytest.raises(ValueError, match="floor_convex"):
            batched_env.BatchedWalkEnv(refs, view, batch_size=1, floor_convex=True, **kw)
    for kw in ({}, {"floor_contacts": False}, {"floor_contacts": "primitives"}, {"floor_contacts": False, "self_contacts": True}, {"self_contacts": True}):
        with pytest.raises(ValueError, match="floor_convex"):
            fly_envs.walk_imitation(floor_convex=True, **kw)
    with pytest.raises(OSError):  # the keywords pass the factory's validation: the next thing on the way is the reference file
        fly_envs.walk_imitation(os.path.join(ROOT, "tests", "no_such_clips.npz"), floor_contacts="primitives", self_contacts=True, floor_convex=True)
    # the default call still raises, with every pinned word and with the opt-in and the two reasons
    doc = " ".join(fly_envs.walk_imitation.__doc__.split())
    for kw in ({}, {"floor_contacts": True}):
        with pytest.raises(NotImplementedError) as e:
            fly_envs.walk_imitation(**kw)
        for text in ("floor contacts", '"primitives"', "own contacts", "ellipsoid", "self_contacts=True", "free-root smooth dynamics", "task layer",
                     "limits", "sensors", "episode protocol", "floor_convex=True", "follow-up", "NC = 16", "40 %"):
            assert text in str(e.value), text
    for word in ("free-root smooth dynamics", "task layer", "limits", "floor contacts", "sensors", "episode protocol", "floor_convex=True", "NC = 16"):
        assert word in doc, word
    with pytest.raises(ValueError):
        fly_envs.walk_imitation(floor_contacts="all")
    assert UNIT in build.SOURCES and build.PER_SOURCE_FLAGS[UNIT] == build.PER_SOURCE_FLAGS["walk_env.hip"]
    bdoc = batched_env.BatchedWalkEnv.__doc__
    assert "floor_convex=True" in bdoc and "reals[:, 3]" in bdoc
    hdr = open(os.path.join(ROOT, "include", "flybody_env.h")).read()
    assert ("FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS | FFE_WALK_EPISODES | FFE_WALK_FLOOR | FFE_WALK_SELF | FFE_WALK_SELF_EPISODES |\n"
            "   *   FFE_WALK_FLOOR_CONVEX ") in hdr
    assert "real 3 = the" in hdr and "plane-ellipsoid / plane-cylinder contacts among int 5 (real 3 is zero on every other handle)" in hdr
    assert "csrc/walk_imit_full_env.hip" in hdr
    src = open(os.path.join(ROOT, "flybody_amd", "csrc", "walk_env.hip")).read()
    assert "under the environment (FFE_WALK_EPISODES) it is not built yet" not in src


# ------------------------------------------------------------------------------------------------ resources
@functools.lru_cache(maxsize=None)
def _tiles(src):
    from flybody_amd import build

    return {k: u for k, u in build.kernel_resource_usage(src, "").items() if u.get("LDS Size", 0) > 0}


def test_kernel_inside_the_resource_targets():
    """One kernel with an LDS tile in the new unit, with a name the older tests do not count: tile <= 20 480 B, two waves per SIMD, no VGPR
    spill."""
    use = _tiles(UNIT)
    assert len(use) == 1, sorted(use)
    (name, u), = use.items()
    print(name, u, "recorded", NEW)
    assert "imitation_full_step" in name and "walk_" not in name and "_kernel" not in name and not re.search(r"\dfloor_stepE", name), name
    assert u["LDS Size"] <= 20480 and u["VGPRs Spill"] == 0 and u["Occupancy"] == 2
    src = open(os.path.join(ROOT, "flybody_amd", "csrc", UNIT)).read()
    assert "__launch_bounds__(64, 2)" in src and "WTileSXC" in src


def test_the_eight_kernels_before_it_keep_the_parents_figures():
    units = sorted({u for u, _ in PARENT8})
    assert sum(len(_tiles(u)) for u in units) == 8
    for (unit, key), ref in PARENT8.items():
        (u,) = [v for k, v in _tiles(unit).items() if key in k]
        assert {k: u[k] for k in ref} == ref, (unit, key, u)


# ------------------------------------------------------------------------------------------------ fixtures, with the oracle alone
def test_round_blobs():
    """2 352 pairs on the oracle blob; its floor contacts on the retyped geoms equal `plane_ellipsoid` on the round sizes; the two blobs
    count the same contacts at qpos0."""
    from flybody_amd.model.blob import read_blob
    from oracle import oracle as O

    dev, ora = X.round_blobs()
    assert os.path.exists(os.path.splitext(dev)[0] + ".json")
    ell, r = X.ellipsoids()
    assert len(ell) == 16
    td, to = read_blob(dev), read_blob(ora)
    assert (np.asarray(td["geom_type"]).ravel()[ell] == 4).all() and (np.asarray(to["geom_type"]).ravel()[ell] == 2).all()
    assert np.array_equal(np.asarray(td["geom_size"])[ell], np.repeat(np.asarray(to["geom_size"])[ell, :1], 3, axis=1))
    m = X.round_model()
    assert m.npair == 2352
    n, x0 = F.plane()
    samples, _ = X.round_samples(0)
    worst, seen = 0.0, 0
    d = O.OracleData(m)
    for s in samples:
        d.qpos[:], d.qvel[:], d.act[:] = s["state"]
        d.ctrl[:] = 0
        d.forward()
        got = {g: (dist, pos) for g, dist, pos, _ in X.round_floor(d)}
        for g, rr in zip(ell, r):
            margin, _ = F.pair_margin(g)
            want = F.plane_ellipsoid(n, x0, d.geom_xpos[g], d.geom_xmat[g], [rr, rr, rr], margin)
            assert (g in got) == bool(want), (g, got.get(g), want)
            if want:
                worst = max(worst, abs(got[g][0] - want[0][1]), float(np.abs(got[g][1] - want[0][0]).max()))
                seen += 1
    print(f"round blobs: {seen} floor contacts on retyped geoms over {len(samples)} states, worst difference from plane_ellipsoid {worst:.2e} cm")
    assert seen >= 20 and worst <= 1e-12
    counts = []
    for path in (S.WALK_BLOB, ora):
        mm = O.OracleModel(path)
        dd = O.OracleData(mm)
        dd.forward()
        counts.append(dd.ncon_matter)
    assert counts == [6, 6], counts


@pytest.mark.parametrize("flags,name", X.FLAG_SETS)
def test_round_samples(flags, name):
    """Every compared step has a round geom on the floor in at least one substep and no cylinder candidate inside margin + CLEAR in any;
    thorax and head contacts occur among the kept ones; the band leaves out no more than a quarter."""
    _, names, _ = S.tables()
    samples, _ = X.round_samples(flags)
    keep = X.kept(samples)
    print(f"{name} seed {X.SEEDS[flags]}: {len(samples) - len(keep)} of {len(samples)} left out; contacts {[s['ncon'] for s in samples]}, plane-round "
          f"{[s['nconvex'] for s in samples]}, cylinder clearance {min(s['cyl'] for s in samples):.4f} cm")
    assert len(samples) == 28 and len(samples) - len(keep) <= X.LEFT_OUT_CAP == len(samples) // 4
    assert all(s["cyl"] >= X.CLEAR for s in samples)
    assert all(s["st"] == 1 for s in samples) and max(max(t[0] for t in s["trace"]) for s in samples) <= 9
    assert all(s["geoms"] for s in samples)
    touched = [{names[g] for g in samples[i]["geoms"]} for i in keep]
    assert any(any("thorax" in x for x in t) for t in touched)
    assert any(any(k in x for k in X.HEAD_KINDS for x in t) for t in touched)
    if flags == 0:
        runs = X.open_loop(0)
        assert all(r["cyl"] >= X.CLEAR and r["gap"] >= S.BAND and r["st"] == 1 for run in runs for r in run)
        assert all(any(r["nconvex"] for r in run) for run in runs)


def test_static_clips_and_their_witnesses():
    """The pose each reset builds is inside every capacity and CLEAR (`_accept`), and a reset of the oracle env on its witness blob
    reproduces the restated contacts to 1e-12 cm, with `ncon_matter` the sum."""
    refs, info = X.static_clips()
    ty = F._flat("geom_type")
    assert [c["set"] for c in info] == ["A", "A", "B", "B", "C", "C"] and refs.ntraj == 6
    assert (np.diff(refs.off) == X.CLIP_ROWS).all() and X.CLIP_ROWS > 64 + 1
    nconvex = []
    for k, c in enumerate(info):
        pose = X.reset_pose(refs, k)
        assert np.abs(pose - c["pose"]).max() <= 1e-12  # the reset builds the pose that was settled and accepted
        ok, keep, (total, nprim, nkeep) = F._accept(pose)
        assert ok and total <= 16 and nkeep == len(c["contacts"]) >= 1
        d0 = F.forward(pose)
        st, r, disc, obs, ncon, nself, con, layout, o = X.witness_reset(refs, k, False)
        assert (st, r, disc) == (0, 0.0, 1.0) and ncon == d0.ncon_matter + len(con)
        wit = [row for row in o.data.contacts() if max(int(row[0]), int(row[1])) >= 71]
        assert len(wit) == len(con)
        for row, (g, p, dist, _) in zip(wit, con):
            assert abs(row[5] - dist) <= 1e-12 and np.abs(row[6:9] - p).max() <= 1e-12 and not int(row[3])
        nconvex.append((len(con), sum(1 for x in con if ty[x[0]] == 5)))
    print("static clips: (plane-convex contacts, of them plane-cylinder)", nconvex)
    assert max(n for n, _ in nconvex) >= 2 and any(c for _, c in nconvex)


def test_bridge_states():
    st = X.bridge_states()
    assert len(st) == 24 and [s[0] for s in st] == ["A"] * 8 + ["B"] * 8 + ["C"] * 8
    a = X.actions(77, 1, 0.5)[0]
    ctrl = X.applied_ctrl(a)
    assert ctrl.shape == (59,) and np.isfinite(ctrl).all() and np.abs(ctrl).max() > 0


# ------------------------------------------------------------------------------------------------ the sense pass on the host
@pytest.fixture(scope="module")
def host_report(tmp_path_factory):
    """tests/walk_full_sense_host.cpp built with -fsanitize=address,undefined and run on its own (never loaded into Python) on the 28
    round samples: the device's tables of the round device blob, the oracle's states and contacts on the round oracle blob."""
    from oracle import oracle as O

    tmp = tmp_path_factory.mktemp("walk_full_sense")
    exe, states = str(tmp / "walk_full_sense_host"), str(tmp / "states.bin")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "walk_full_sense_host.cpp")])
    m = X.round_model()
    body = np.asarray(S.tables()[0]["geom_bodyid"]).ravel()
    ell = set(X.ellipsoids()[0].tolist())
    d = O.OracleData(m)
    buf, ncons, nself, nround, nroot = [], 0, 0, 0, 0
    samples, _ = X.round_samples(0)
    for s in samples:
        d.qpos[:], d.qvel[:], d.act[:] = s["state"]
        d.ctrl[:] = 0
        rec, cons = _sensor_record(d, body)
        buf.append(rec)
        ncons += len(cons)
        nself += len(S.fly_fly(cons))
        rnd = [int(c[1]) for c in cons if int(c[0]) == 0 and int(c[1]) in ell]
        nround += len(rnd)
        nroot += sum(1 for g in rnd if body[g] == 1)
    np.concatenate([[float(len(buf))]] + buf).tofile(states)
    r = subprocess.run([exe, X.round_blobs()[0], states], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr  # a sanitizer report ends the program with a non-zero status
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    print(r.stdout)
    rep = dict(line.split(None, 1) for line in r.stdout.splitlines())
    rep.update(oracle_contacts=ncons, oracle_flyfly=nself, oracle_round=nround, oracle_root=nroot, nstates=len(samples))
    return rep


def test_host_program_sees_slots_with_link_255_and_geoms_past_the_first_table(host_report):
    rep = host_report
    for tag in ("f64", "f32"):
        assert int(rep[tag + "_states"]) == rep["nstates"] and int(rep[tag + "_contacts"]) == rep["oracle_contacts"] and rep[tag + "_unmatched"] == "0"
        assert int(rep[tag + "_most_contacts"]) <= 16
        assert int(rep[tag + "_convex"]) == rep["oracle_round"] >= 20 and int(rep[tag + "_convex_root"]) == rep["oracle_root"] >= 5
        # coxae, head, wings and thorax are not below a tarsus, and none is a claw: such a slot adds to no sensor of the shipped model
        assert rep[tag + "_convex_sensed"] == "0" and rep[tag + "_convex_touch"] == "0"


def test_force_and_touch_equal_the_oracle_in_float64(host_report):
    for k in ("force", "touch"):
        print(f"{k}: float64 error {float(host_report['f64_' + k]):.3e} relative to max(1, {float(host_report['f64_' + k + '_scale']):.4f})")
    for k in ("force", "touch"):
        assert float(host_report["f64_" + k]) <= 1e-12, (k, host_report["f64_" + k])


def test_force_and_touch_in_float32(host_report):
    for k in ("force", "touch"):
        print(f"{k}: float32 error {float(host_report['f32_' + k]):.3e} (recorded {F32_MEASURED[k]})")
    for k in ("force", "touch"):
        assert F32_MEASURED[k] is not None, "the measured float32 error has not been recorded"
        assert float(host_report["f32_" + k]) <= 3 * F32_MEASURED[k], (k, host_report["f32_" + k])
