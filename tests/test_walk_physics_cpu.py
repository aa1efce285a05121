"""CPU-side checks of the free-root walking-fly physics (csrc/walk_env.hip, walk_model.hpp): the C ABI
entry is declared and exported, the free-root kernel sits in its own translation unit inside its resource targets while the tethered
kernel keeps its figures, and the host table builder - as a stand-alone program under AddressSanitizer and UBSan - gives the tethered
fly's tables on the walk blob and unchanged tables on the ball blob."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

ASSETS = os.path.join(ROOT, "flybody_amd", "assets")
WALK_BLOB, BALL_BLOB = os.path.join(ASSETS, "fly_walk.ffmb"), os.path.join(ASSETS, "fly_ball.ffmb")


def test_create_walk_physics_is_declared_and_exported():
    from flybody_amd import _capi, build

    hdr = open(os.path.join(ROOT, "include", "flybody_env.h")).read()
    assert re.search(r"\bint\s+ffe_create_walk_physics\s*\(", hdr) and "ffe_walk_physics_task" in hdr
    assert "ffe_create_walk_physics" in _capi.SYMBOLS
    build.build()
    assert hasattr(_capi.lib(), "ffe_create_walk_physics")
    assert "walk_env.hip" in build.SOURCES and {"leg_dyn.hpp", "leg_stage1.inc", "row_newton.hpp", "walk_model.hpp", "walk_env.hpp"} <= set(build.HEADERS)


def test_free_root_kernel_meets_its_resource_targets():
    """tile <= 20 480 B (8 waves per CU), two waves per SIMD; with the constraint code compiled out VGPRs and scratch
    stay below the tethered kernel's 256 / 492 B.  The figures are printed for the record."""
    from flybody_amd import build

    use = build.kernel_resource_usage("walk_env.hip", "walk_step")
    assert len(use) == 1, use
    (name, u), = use.items()
    print(name, u)
    assert u["LDS Size"] <= 20480 and u["Occupancy"] == 2
    assert u["VGPRs"] <= 256 and u["ScratchSize"] <= 492 and u["VGPRs Spill"] == 0


def test_tethered_kernel_keeps_its_resource_figures():
    from flybody_amd import build

    use = build.kernel_resource_usage("ball_env.hip", "ball_step")
    assert len(use) == 1, use
    (name, u), = use.items()
    print(name, u)
    assert (u["VGPRs"], u["ScratchSize"], u["LDS Size"], u["Occupancy"]) == (256, 492, 20128, 2)
    # as the commit before its collision passes moved to self_pairs.hpp compiles it
    assert (u["SGPRs Spill"], u["VGPRs Spill"]) == (130, 76)


def test_the_step_kernels_live_in_separate_translation_units():
    csrc = os.path.join(ROOT, "flybody_amd", "csrc")
    ball, walk = open(os.path.join(csrc, "ball_env.hip")).read(), open(os.path.join(csrc, "walk_env.hip")).read()
    assert "ball_step_kernel" in ball and "walk_step_kernel" not in ball and "FREE_ROOT = false" in ball
    assert "walk_step_kernel" in walk and "ball_step_kernel" not in walk and "FREE_ROOT = true" in walk
    for src in (ball, walk):  # both compile the same leg code and the same constraint solve
        assert '#include "leg_dyn.hpp"' in src and '#include "leg_stage1.inc"' in src and '#include "row_newton.hpp"' in src
        assert "row_newton<" in src
    for name in sorted(os.listdir(csrc)):  # and no source defines a Newton of its own
        if name.endswith(".hip"):
            src = open(os.path.join(csrc, name)).read()
            assert "dense_newton(" not in src and "limits_newton(" not in src, name


@pytest.fixture(scope="module")
def builder_report(tmp_path_factory):
    """tests/walk_model_host.cpp built with -fsanitize=address,undefined and run on its own (never loaded into Python)."""
    exe = str(tmp_path_factory.mktemp("walk_model") / "walk_model_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "walk_model_host.cpp")])
    r = subprocess.run([exe, WALK_BLOB, BALL_BLOB], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr  # a sanitizer report ends the program with a non-zero status
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    return dict(line.split(None, 1) for line in r.stdout.splitlines()), r.stderr


def test_walk_builder_gives_the_tethered_tables_plus_the_root(builder_report):
    from oracle import oracle as O

    rep, err = builder_report
    m = O.OracleModel(WALK_BLOB)
    assert (int(rep["links"]), int(rep["halteres"]), int(rep["hinge_dofs"]), int(rep["blocks"]), int(rep["actuators"])) == (64, 2, 102, 12, 59)
    assert int(rep["hinge_dofs"]) + 6 == m.nv == 108 and int(rep["actuators"]) == m.nu and m.nq == 109
    assert int(rep["links"]) + int(rep["halteres"]) + 2 == m.nbody  # + world + thorax
    from flybody_amd.model.blob import read_blob

    t = read_blob(WALK_BLOB)
    assert float(rep["root_mass"]) == float(t["body_mass"][1]) and float(rep["root_mass"]) > 0
    assert abs(float(rep["total_mass"]) - float(sum(t["body_mass"]))) < 1e-15
    assert float(rep["timestep"]) == pytest.approx(m.timestep, rel=1e-7) and float(rep["gravity_z"]) == -981.0
    # the hinge order of the two models is the same, so every table the leg code reads equals the ball builder's
    for key in ("same_tree", "same_dofs", "same_schedules", "same_actuators", "same_link_inertia"):
        assert rep[key] == "1", key
    assert int(rep["floor_geom"]) >= 0 and int(rep["limited_hinges"]) > 0
    # a blob that is not the walk model is refused with a text, not a crash
    assert rep["ball_blob_refused"] == "1" and "walk model" in err


def test_ball_builder_results_are_unchanged(builder_report):
    """Fingerprint (FNV-1a over the BallModel bytes) of build_ball_model on fly_ball.ffmb, recorded before the builder learned about the
    walk blob."""
    rep, _ = builder_report
    assert rep["ball_model_bytes"] == "112328" and rep["ball_model_fnv"] == "ba12b18360ef4491"


def test_json_hinge_order_is_shared():
    import json

    names = [json.load(open(os.path.join(ASSETS, f)))["jnt_name"] for f in ("fly_ball.json", "fly_walk.json")]
    assert names[0][1:] == names[1][1:] and len(names[1]) == 103


def test_walk_imitation_says_what_exists_and_what_is_missing():
    from flybody_amd import batched_env, fly_envs

    with pytest.raises(NotImplementedError) as e:
        fly_envs.walk_imitation()
    doc = " ".join(fly_envs.walk_imitation.__doc__.split())
    for word in ("free-root smooth dynamics", "task layer", "limits", "floor contacts", "sensors", "episode protocol"):
        assert word in str(e.value) and word in doc, word
    assert hasattr(batched_env, "BatchedWalkPhysics")
