"""CPU-side checks of the walk_imitation environment on the floor with the fly's own contacts (csrc/walk_imit_self_env.hip
`imitation_self_step`, FFE_WALK_EPISODES | FFE_WALK_FLOOR | FFE_WALK_SELF): the keyword exists on the env
and on the factory, the seventh free-root step kernel fits its tile in a translation unit of its own while the six before it keep the
parent's resource figures, what a fly-fly contact adds to the force and touch sensors (csrc/walk_self_sense.hpp) agrees with the float64
oracle, the oracle's touch sensors equal the shortcut the kernel uses, and the teacher-forced samples of the GPU tests stay inside the
band cap.  Everything runs on the shipped blob.  The formulas run in a stand-alone program under AddressSanitizer and UBSan
(tests/walk_self_sense_host.cpp)."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import walk_self_env_samples as E
import walk_self_sets as S
from test_walk_self_cpu import PARENT

UNIT = "walk_imit_self_env.hip"
# `floor_self_step` as the parent commit compiles it; SGPRs Spill was 153 before `self_forces` and
# `floor_forces` became one `contact_forces`
PARENT_SELF = {"VGPRs": 256, "ScratchSize": 368, "LDS Size": 20176, "SGPRs Spill": 151, "VGPRs Spill": 0, "Occupancy": 2}
# the figures the build reaches for the new kernel
NEW = {"VGPRs": 256, "ScratchSize": 368, "LDS Size": 20416, "VGPRs Spill": 0, "Occupancy": 2}
# Worst float32 errors the host program measured on R10 + XL + XS (48 states), relative to max(1, largest |reference|): recorded (DESIGN.md
# section 7), printed next to each run's figure, not asserted (the float64 instantiation alone is bounded).
F32_MEASURED = {"force": 1.5e-7, "touch": 2.1e-8}


def test_interface():
    from flybody_amd import batched_env, build, fly_envs

    for fn in (batched_env.BatchedWalkEnv.__init__, fly_envs.walk_imitation):
        p = inspect.signature(fn).parameters["self_contacts"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    view_refs = E.world()
    with pytest.raises(ValueError, match="floor_contacts"):  # before any device call
        batched_env.BatchedWalkEnv(view_refs[1], view_refs[0], batch_size=1, self_contacts=True)
    with pytest.raises(ValueError, match="floor_contacts"):
        fly_envs.walk_imitation(floor_contacts=False, self_contacts=True)
    with pytest.raises(NotImplementedError) as e:
        fly_envs.walk_imitation()
    for text in ("floor contacts", '"primitives"', "own contacts", "ellipsoid", "self_contacts=True"):
        assert text in str(e.value), text
    with pytest.raises(OSError):  # the keyword passes the factory's validation: the next thing on the way is the reference file
        fly_envs.walk_imitation(os.path.join(ROOT, "tests", "no_such_clips.npz"), floor_contacts="primitives", self_contacts=True)
    assert UNIT in build.SOURCES and build.PER_SOURCE_FLAGS[UNIT] == build.PER_SOURCE_FLAGS["walk_env.hip"]
    assert "walk_self_sense.hpp" in build.HEADERS
    assert "self_contacts=True" in batched_env.BatchedWalkEnv.__doc__ and "reals[:, 2]" in batched_env.BatchedWalkEnv.__doc__
    hdr = open(os.path.join(ROOT, "include", "flybody_env.h")).read()
    assert "FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS | FFE_WALK_EPISODES | FFE_WALK_FLOOR | FFE_WALK_SELF | FFE_WALK_SELF_EPISODES\n" in hdr
    assert re.search(r"\bFFE_WALK_SELF_EPISODES\s*=\s*8192\b", hdr) and batched_env.FFE_WALK_SELF_EPISODES == 8192
    assert "real 2 = the fly-fly contacts among them" in hdr


def _tiles(src):
    from flybody_amd import build

    return {k: u for k, u in build.kernel_resource_usage(src, "").items() if u.get("LDS Size", 0) > 0}


def test_kernel_inside_the_resource_targets():
    """One kernel with an LDS tile in the new unit, with a name the older tests do not count: tile <= 20 480 B, two waves per SIMD, and the
    figures the build reaches (no VGPR spill, as both parents)."""
    use = _tiles(UNIT)
    assert len(use) == 1, sorted(use)
    (name, u), = use.items()
    print(name, u)
    assert "imitation_self_step" in name and "walk_" not in name and "_kernel" not in name and not re.search(r"\dfloor_stepE", name), name
    assert u["LDS Size"] <= 20480 and u["Occupancy"] == 2
    assert {k: u[k] for k in NEW} == NEW, u


def test_the_six_kernels_before_it_keep_the_parents_figures():
    use = {**_tiles("walk_env.hip"), **_tiles("walk_floor_env.hip")}
    assert len(use) == 5, sorted(use)
    for name, ref in PARENT.items():
        (u,) = [u for k, u in use.items() if re.search(r"\d" + name + "E", k)]
        assert {k: u[k] for k in ref} == ref, (name, u)
    (u,) = _tiles("walk_self_env.hip").values()
    assert {k: u[k] for k in PARENT_SELF} == PARENT_SELF, u


def _sensor_record(d, body):
    """One state of states.bin from the oracle (tests/walk_self_sense_host.cpp has the layout): `d` holds (qpos, qvel, act, ctrl)."""
    d.step1()
    qpos, qvel = d.qpos.copy(), d.qvel.copy()
    xpos, xquat = d.xpos.ravel().copy(), d.xquat.ravel().copy()
    d.step2()
    cons = d.contacts()  # (the collision of step1 with the rows step2 gave it: step2 integrates the state, the contact list stays)
    rec = [qpos, qvel, d.qacc.copy(), xpos, xquat, [float(len(cons))]]
    force = d.efc_force.copy()
    for c in cons:  # rows: geom1, geom2, dim, exclude, efc_adr, dist, pos[3], normal[3], mu, friction, includemargin, normal force
        adr, dim = int(c[4]), int(c[2])
        f = np.zeros(3)
        if adr >= 0:
            f[:dim] = force[adr:adr + dim]
        rec.append([c[4], c[0], c[1], body[int(c[0])], body[int(c[1])], *c[9:12], *f])
    rec += [d.sens_force.ravel().copy(), d.sens_touch.copy()]
    return np.concatenate([np.asarray(x, dtype=np.float64).ravel() for x in rec]), cons


@pytest.fixture(scope="module")
def host_report(tmp_path_factory):
    """tests/walk_self_sense_host.cpp built with -fsanitize=address,undefined and run on its own (never loaded into Python) on R10 + XL +
    XS: per state qpos, qvel before the integration, and qacc, the contacts with their efc_force and the sensors after step1; step2."""
    from oracle import oracle as O

    tmp = tmp_path_factory.mktemp("walk_self_sense")
    exe, states = str(tmp / "walk_self_sense_host"), str(tmp / "states.bin")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "walk_self_sense_host.cpp")])
    m = S.model()
    body = np.asarray(S.tables()[0]["geom_bodyid"]).ravel()
    d = O.OracleData(m)
    buf, ncons, nself = [], 0, 0
    for s in S.r10() + S.x_lifted() + S.x_standing():
        d.qpos[:], d.qvel[:], d.act[:] = s[:3]
        d.ctrl[:] = 0
        rec, cons = _sensor_record(d, body)
        buf.append(rec)
        ncons += len(cons)
        nself += len(S.fly_fly(cons))
    np.concatenate([[float(len(buf))]] + buf).tofile(states)
    r = subprocess.run([exe, S.WALK_BLOB, states], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr  # a sanitizer report ends the program with a non-zero status
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    print(r.stdout)
    rep = dict(line.split(None, 1) for line in r.stdout.splitlines())
    rep["oracle_contacts"], rep["oracle_flyfly"] = ncons, nself
    return rep


def test_host_program_sees_the_oracle_states(host_report):
    rep = host_report
    for tag in ("f64", "f32"):
        assert int(rep[tag + "_states"]) == 24 + 2 * S.NX and int(rep[tag + "_contacts"]) == rep["oracle_contacts"] and rep[tag + "_unmatched"] == "0"
        assert int(rep[tag + "_flyfly"]) == rep["oracle_flyfly"] >= 80 and int(rep[tag + "_most_contacts"]) <= 16
        # fly-fly contacts with a row under a force sensor on the side of geom2 (c_link) and of geom1 (c_link1), and rows against a
        # geom of the thorax (that side has no link and adds to no sensor)
        assert int(rep[tag + "_flyfly_pos"]) >= 1 and int(rep[tag + "_flyfly_neg"]) >= 1 and int(rep[tag + "_flyfly_thorax"]) >= 1, rep
    assert float(rep["f64_force_scale"]) > 0.1 and float(rep["f64_touch_scale"]) > 0.1


def test_force_and_touch_equal_the_oracle_in_float64(host_report):
    for k in ("force", "touch"):
        print(f"{k}: float64 error {float(host_report['f64_' + k]):.3e} relative to max(1, {float(host_report['f64_' + k + '_scale']):.4f})")
    for k in ("force", "touch"):
        assert float(host_report["f64_" + k]) <= 1e-12, (k, host_report["f64_" + k])


def test_force_and_touch_in_float32_are_recorded(host_report):
    for k in ("force", "touch"):
        e = float(host_report["f32_" + k])
        print(f"{k}: float32 error {e:.3e} (recorded {F32_MEASURED[k]:.1e})")
        assert np.isfinite(e)


def test_touch_is_the_sum_of_positive_normal_forces_in_the_oracle():
    """tests/test_walk_floor_env_cpu.py's check on the shipped blob: the oracle's touch (mj_sensorAcc's ray test against the touch site)
    equals the sum of the positive normal forces of all contacts with rows on the claw's body, on either side of the pair - on the rollout
    of that test (72 steps at amplitudes 0 / 0.6 / 1.0) and on the crafted poses XS and XL.  0 mismatches in 1 440 checks; the sum over the
    floor's contacts alone differs somewhere (a claw touched by the fly itself)."""
    from flybody_amd.tasks import walking as W
    from oracle import oracle as O

    t = S.tables()[0]
    gbody = np.asarray(t["geom_bodyid"]).ravel()
    site_body = np.asarray(t["sites_bodyid"]).ravel()[np.asarray(t["touch_site"]).ravel()]
    view = W.WalkModelView()
    refs = W.WalkRefSet(W.synthetic_snippets(view, n=1, length=200))
    m = S.model()
    count = dict(checks=0, live=0, most=0, floor_only_differs=0)

    def check(state, ctrl, what):
        d = O.OracleData(m)
        d.qpos[:], d.qvel[:], d.act[:] = state[:3]
        d.ctrl[:] = ctrl
        d.step1()
        d.step2()
        cons = d.contacts()
        force = d.efc_force.copy()
        count["most"] = max(count["most"], len(cons))
        for k, body in enumerate(site_body):
            rows = [c for c in cons if int(c[4]) >= 0 and body in (gbody[int(c[0])], gbody[int(c[1])])]
            want = sum(max(0.0, force[int(c[4])]) for c in rows)
            floor = sum(max(0.0, force[int(c[4])]) for c in rows if int(c[0]) == 0)
            got = float(d.sens_touch[k])
            count["checks"] += 1
            count["live"] += got > 0
            count["floor_only_differs"] += abs(got - floor) > 1e-12 * max(1.0, got)
            assert abs(got - want) <= 1e-12 * max(1.0, want), (what, k, got, want)

    for amp in (0.0, 0.6, 1.0):
        env = O.OracleWalkEnv(m, refs, view.mocap_jnt, view.mocap_site, (view.retract_qadr, view.retract_val), terminal_com_dist=float("inf"))
        env.force_next(0)
        env.reset()
        rs = np.random.RandomState(5)
        for step in range(72):
            st, _, _, _ = env.step(rs.uniform(-amp, amp, env.naction))
            assert st == 1
            check((env.data.qpos, env.data.qvel, env.data.act), env.data.ctrl, (amp, step))
    for i, s in enumerate(S.x_standing() + S.x_lifted()):
        check(s, 0.0, ("crafted", i))
    print(count)
    assert count["checks"] == (3 * 72 + 2 * S.NX) * 6 == 1440 and count["live"] > count["checks"] // 2
    assert count["floor_only_differs"] >= 1 and count["most"] <= 16


@pytest.mark.parametrize("which,flags", sorted(E.SEEDS))
def test_the_band_leaves_out_no_more_than_the_cap(which, flags):
    """The teacher-forced samples the GPU tests compare (walk_self_env_samples.forced_samples): how many come within BAND = 2e-6 cm of
    a switching distance during the control step, with the oracle alone, so that the seeds hold on any machine.  Every sample is a step
    inside its episode, and fly-fly rows occur among the kept ones."""
    samples, _ = E.forced_samples(which, flags)
    keep = E.kept(samples)
    print(f"{which} flags {flags} seed {E.SEEDS[(which, flags)]}: {len(samples) - len(keep)} of {len(samples)} left out; contacts "
          f"{[s['ncon'] for s in samples]}, fly-fly {[s['nself'] for s in samples]}")
    assert len(samples) == (24 if which == "R10" else S.NX)
    assert len(samples) - len(keep) <= E.LEFT_OUT_CAP[which]
    assert any(samples[i]["self_rows"] > 0 for i in keep)
    assert max(s["ncon"] for s in samples) <= 16
