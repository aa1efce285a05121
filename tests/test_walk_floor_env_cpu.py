"""CPU-side checks of the walk_imitation environment on the floor (csrc/walk_floor_env.hip `imitation_floor_step`; DESIGN.md section 12
step 4c): the keyword and the factory option exist, the fifth free-root step kernel sits inside its resource targets in a translation
unit of its own, the force / touch formulas behind it (csrc/walk_sense.hpp) agree with the float64 oracle, and the oracle's touch
sensors on the floor equal the shortcut the kernel uses.  The formulas run in a stand-alone program under AddressSanitizer and UBSan
(tests/walk_sense_host.cpp)."""
import inspect
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import walk_floor_sets as S

UNIT = "walk_floor_env.hip"
# Worst float32 errors the host program measured on F06 + F10 (48 states, 196 contacts, 543 rows), relative to max(1, largest
# |reference|): recorded, printed next to each run's figure, not asserted (the issue bounds the float64 instantiation only).
F32_MEASURED = {"force": 2.5e-7, "touch": 4.9e-8}


def test_interface():
    from flybody_amd import batched_env, build, fly_envs

    sig = inspect.signature(batched_env.BatchedWalkEnv.__init__)
    assert sig.parameters["floor_contacts"].default is False and sig.parameters["floor_contacts"].kind is inspect.Parameter.KEYWORD_ONLY
    with pytest.raises(NotImplementedError, match="floor contacts") as e:
        fly_envs.walk_imitation(floor_contacts=True)
    assert '"primitives"' in str(e.value)  # the text names the option and says what is missing
    assert "own contacts" in str(e.value) and "ellipsoid" in str(e.value)
    with pytest.raises(ValueError, match="primitives"):
        fly_envs.walk_imitation(floor_contacts="all")  # validated before anything touches a GPU
    with pytest.raises(OSError):  # "primitives" passes that validation: the next thing on the way is the reference file, which is not there
        fly_envs.walk_imitation(os.path.join(ROOT, "tests", "no_such_clips.npz"), floor_contacts="primitives")
    assert UNIT in build.SOURCES and build.PER_SOURCE_FLAGS[UNIT] == build.PER_SOURCE_FLAGS["walk_env.hip"]
    assert "walk_substeps.hpp" in build.HEADERS and "walk_sense.hpp" in build.HEADERS


@pytest.fixture(scope="module")
def tile_kernels():
    from flybody_amd import build

    use = build.kernel_resource_usage(UNIT, "")
    return {k: u for k, u in use.items() if u.get("LDS Size", 0) > 0}


def test_kernel_inside_the_resource_targets(tile_kernels):
    """One kernel with an LDS tile in the new unit: tile <= 20 480 B, two waves per SIMD, no VGPR spill; a name the older tests do not count."""
    assert len(tile_kernels) == 1, sorted(tile_kernels)
    (name, u), = tile_kernels.items()
    print(name, u)
    assert "imitation_floor_step" in name and "walk_" not in name and "_kernel" not in name, name
    assert u["LDS Size"] <= 20480 and u["Occupancy"] == 2 and u["VGPRs Spill"] == 0


@pytest.fixture(scope="module")
def host_report(tmp_path_factory):
    """tests/walk_sense_host.cpp built with -fsanitize=address,undefined and run on its own (never loaded into Python) on F06 + F10: per
    state qpos, qvel before the integration, and qacc, the contacts with their efc_force and the sensors after step1; step2."""
    from oracle import oracle as O

    tmp = tmp_path_factory.mktemp("walk_sense")
    exe, states = str(tmp / "walk_sense_host"), str(tmp / "states.bin")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "walk_sense_host.cpp")])
    m, F06, F10 = S.sets()
    d = O.OracleData(m)
    buf, ncons = [], []
    for s in F06 + F10:
        d.qpos[:], d.qvel[:], d.act[:] = s
        d.ctrl[:] = 0
        d.step1()
        qpos, qvel = d.qpos.copy(), d.qvel.copy()
        xpos, xquat = d.xpos.ravel().copy(), d.xquat.ravel().copy()
        d.step2()
        cons = d.contacts()  # (the collision of step1 with the rows step2 gave it: step2 integrates the state, the contact list stays)
        ncons.append(len(cons))
        rec = [qpos, qvel, d.qacc.copy(), xpos, xquat, [float(len(cons))]]
        force = d.efc_force.copy()
        for c in cons:  # rows: geom1, geom2, dim, exclude, efc_adr, dist, pos[3], normal[3], mu, friction, includemargin, normal force
            adr = int(c[4])
            rec.append([c[4], c[1], *(force[adr:adr + 3] if adr >= 0 else (0.0, 0.0, 0.0))])
        rec += [d.sens_force.ravel().copy(), d.sens_touch.copy()]
        buf.append(np.concatenate([np.asarray(x, dtype=np.float64).ravel() for x in rec]))
    np.concatenate([[float(len(buf))]] + buf).tofile(states)
    r = subprocess.run([exe, S.floor_only_blob(), states], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr  # a sanitizer report ends the program with a non-zero status
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    print(r.stdout)
    rep = dict(line.split(None, 1) for line in r.stdout.splitlines())
    rep["oracle_contacts"] = sum(ncons)
    return rep


def test_host_program_sees_the_oracle_states(host_report):
    rep = host_report
    for tag in ("f64", "f32"):
        assert int(rep[tag + "_states"]) == 48 and int(rep[tag + "_contacts"]) == rep["oracle_contacts"] and rep[tag + "_unmatched"] == "0"
        assert int(rep[tag + "_rows"]) >= 3 * 48 * 2 and int(rep[tag + "_touching"]) > 48
    # the sensors are live: forces of the order of the fly's weight, and an inertial reading on legs in the air
    assert float(rep["f64_force_scale"]) > 0.1 and float(rep["f64_touch_scale"]) > 0.1 and float(rep["f64_free_force"]) > 1e-4


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
    """The kernel's touch is the sum of the positive normal forces of the contacts on the claw's link; the oracle's is mj_sensorAcc's ray
    test against the touch site.  On the floor-only blob the two are the same number: 72-step rollouts at three action amplitudes, every
    state copied into a fresh OracleData and advanced by step1; step2.  The condition is 0 mismatches - a mismatch means the kernel needs
    the ray test, and the assertion names the state."""
    from flybody_amd.model.blob import read_blob
    from flybody_amd.tasks import walking as W
    from oracle import oracle as O

    t = read_blob(S.floor_only_blob())
    gbody = np.asarray(t["geom_bodyid"]).ravel()
    site_body = np.asarray(t["sites_bodyid"]).ravel()[np.asarray(t["touch_site"]).ravel()]
    view = W.WalkModelView()
    refs = W.WalkRefSet(W.synthetic_snippets(view, n=1, length=200))
    m = S.model()
    checks = live = most = 0
    for amp in (0.0, 0.6, 1.0):
        env = O.OracleWalkEnv(m, refs, view.mocap_jnt, view.mocap_site, (view.retract_qadr, view.retract_val), terminal_com_dist=float("inf"))
        env.force_next(0)
        env.reset()
        rs = np.random.RandomState(5)
        for step in range(72):
            st, _, _, _ = env.step(rs.uniform(-amp, amp, env.naction))
            assert st == 1
            d = O.OracleData(m)
            d.qpos[:], d.qvel[:], d.act[:] = env.data.qpos, env.data.qvel, env.data.act
            d.ctrl[:] = env.data.ctrl
            d.step1()
            d.step2()
            cons = d.contacts()
            force = d.efc_force.copy()
            most = max(most, len(cons))
            for k, body in enumerate(site_body):
                want = sum(max(0.0, force[int(c[4])]) for c in cons if int(c[4]) >= 0 and gbody[int(c[1])] == body)
                got = float(d.sens_touch[k])
                checks += 1
                live += got > 0
                assert abs(got - want) <= 1e-12 * max(1.0, want), (amp, step, k, got, want)
    print(f"{checks} checks, {live} with touch > 0, at most {most} contacts at once")
    assert checks == 3 * 72 * 6 and live > checks // 2 and most <= 16
