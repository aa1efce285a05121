"""CPU-side checks of the walking fly's own contacts (csrc/walk_self_env.hip `floor_self_step`, FFE_WALK_SELF; DESIGN.md section 12 step
3c): the opt-in bit and the keyword exist, the sixth step kernel fits its tile while the five before it keep the parent's resource
figures, the collision tables of the walk builder hold the pairs the float64 oracle collides, and the formulas behind the new rows
(csrc/walk_self.hpp) agree with the oracle's constraint rows on the shipped blob.  The formulas run in a stand-alone program under
AddressSanitizer and UBSan (tests/walk_self_host.cpp)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import walk_self_sets as S

QUANTITIES = ("J", "aref", "D", "y0", "G", "qacc")
# the bound of tests/test_walk_floor_cpu.py::test_formulas_equal_the_oracle_in_float64
F64_BOUND = 1e-10
# The five step kernels with an LDS tile as the parent commit compiles them (`build.kernel_resource_usage`): the new code of
# walk_substeps.hpp sits under `if constexpr` on a trait of the new tile and must not change them.
PARENT = {
    "floor_step": {"VGPRs": 256, "ScratchSize": 368, "LDS Size": 19872, "SGPRs Spill": 125, "VGPRs Spill": 0, "Occupancy": 2},
    "walk_step_kernel": {"VGPRs": 168, "ScratchSize": 0, "LDS Size": 18240, "SGPRs Spill": 26, "VGPRs Spill": 0, "Occupancy": 2},
    "walk_limits_kernel": {"VGPRs": 256, "ScratchSize": 112, "LDS Size": 18800, "SGPRs Spill": 57, "VGPRs Spill": 0, "Occupancy": 2},
    "imitation_step_kernel": {"VGPRs": 256, "ScratchSize": 112, "LDS Size": 19712, "SGPRs Spill": 109, "VGPRs Spill": 0, "Occupancy": 2},
    "imitation_floor_step": {"VGPRs": 256, "ScratchSize": 368, "LDS Size": 20304, "SGPRs Spill": 180, "VGPRs Spill": 0, "Occupancy": 2},
}


def test_header_bit_mirror_and_keyword():
    from flybody_amd import batched_env, build

    hdr = open(os.path.join(ROOT, "include", "flybody_env.h")).read()
    assert re.search(r"\bFFE_WALK_SELF\s*=\s*4096\b", hdr)
    assert batched_env.FFE_WALK_SELF == 4096 == S.WALK_SELF
    # the accepted set is in the header's table, and the columns the handle adds are documented
    assert "FFE_NO_CONTACT | FFE_WALK_JOINT_LIMITS | FFE_WALK_FLOOR | FFE_WALK_SELF " in hdr
    assert re.search(r"created with FFE_WALK_SELF reports", hdr) and "int 3 = the fly-fly contacts among them" in hdr and "bit value 8" in hdr
    sig = inspect.signature(batched_env.BatchedWalkPhysics.__init__)
    assert sig.parameters["self_contacts"].default is False and sig.parameters["floor_contacts"].default is False
    doc = batched_env.BatchedWalkPhysics.__doc__
    assert "self_contacts=True" in doc and "int 3" in doc
    assert "walk_self_env.hip" in build.SOURCES and build.PER_SOURCE_FLAGS["walk_self_env.hip"] == build.PER_SOURCE_FLAGS["walk_env.hip"]
    assert {"walk_self.hpp", "walk_self_model.hpp"} <= set(build.HEADERS)


def test_self_contacts_need_the_floor():
    """Checked before anything touches the device."""
    from flybody_amd.batched_env import BatchedWalkPhysics

    with pytest.raises(ValueError, match="floor_contacts"):
        BatchedWalkPhysics(batch_size=1, self_contacts=True)


def test_walk_imitation_keeps_raising():
    from flybody_amd import fly_envs

    with pytest.raises(NotImplementedError, match="floor contacts"):
        fly_envs.walk_imitation()


def _tiles(src):
    from flybody_amd import build

    return {k: u for k, u in build.kernel_resource_usage(src, "").items() if u.get("LDS Size", 0) > 0}


def test_the_five_kernels_before_it_keep_the_parents_figures():
    use = {**_tiles("walk_env.hip"), **_tiles("walk_floor_env.hip")}
    assert len(use) == 5, sorted(use)
    for name, ref in PARENT.items():
        (u,) = [u for k, u in use.items() if re.search(r"\d" + name + "E", k)]
        assert {k: u[k] for k in ref} == ref, (name, u)


def test_self_kernel_fits_its_tile():
    """The sixth kernel with an LDS tile, in a translation unit of its own: tile <= 20 480 B (8 waves per CU); the other figures are
    printed and recorded in DESIGN.md section 12."""
    use = _tiles("walk_self_env.hip")
    ((name, u),) = use.items()
    print(name, u)
    assert "floor_self_step" in name and "walk_" not in name and "_kernel" not in name
    assert u["LDS Size"] <= 20480


@pytest.fixture(scope="module")
def oracle_pairs():
    """The pairs the oracle collides on the shipped blob, as (geom1, geom2) in mj_collision's order."""
    m = S.model()
    L = m.L
    L.fo_pair_g1.restype = L.fo_pair_g2.restype = C.POINTER(C.c_int)
    L.fo_pair_g1.argtypes = L.fo_pair_g2.argtypes = [C.c_void_p]
    g1 = np.ctypeslib.as_array(L.fo_pair_g1(m.ptr), shape=(m.npair,)).copy()
    g2 = np.ctypeslib.as_array(L.fo_pair_g2(m.ptr), shape=(m.npair,)).copy()
    return list(zip(g1.tolist(), g2.tolist()))


def _record(d, body):
    """One state of states.bin from the oracle after `forward` (tests/walk_self_host.cpp has the layout)."""
    cons, (J, aref, D, _), M = d.contacts(), d.efc(), d.dense_M()
    ff = S.fly_fly(cons)
    rec = [d.qpos.copy(), d.qvel.copy(), M.ravel(), d.qacc_smooth.copy(), d.xpos.ravel().copy(), d.xquat.ravel().copy(), [float(len(ff))]]
    rows = []
    for c in ff:
        assert int(c[2]) == 1  # condim 1
        rec.append([body[int(c[0])], body[int(c[1])], c[4], c[5], *c[6:9], *c[9:12], c[14]])
        if c[4] >= 0:
            rows.append(int(c[4]))
    f = d.efc_force[: d.nefc].copy()
    for r in rows:
        rec += [J[r], [aref[r], D[r], f[r]]]
    Jc = J[rows]
    rec.append((Jc @ np.linalg.solve(M, Jc.T)).ravel())
    rec.append(np.linalg.solve(M, Jc.T @ f[rows]) if rows else np.zeros(M.shape[0]))
    return np.concatenate([np.asarray(x, dtype=np.float64).ravel() for x in rec]), ff


@pytest.fixture(scope="module")
def host_report(tmp_path_factory):
    """tests/walk_self_host.cpp built with -fsanitize=address,undefined and run on its own (never loaded into Python) on R10 + XL + XS."""
    from oracle import oracle as O

    tmp = tmp_path_factory.mktemp("walk_self")
    exe, states, pairs = str(tmp / "walk_self_host"), str(tmp / "states.bin"), str(tmp / "pairs.txt")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "walk_self_host.cpp")])
    m = S.model()
    body = np.asarray(S.tables()[0]["geom_bodyid"]).ravel()
    d = O.OracleData(m)
    buf, seen, nrows = [], [], 0
    for s in S.r10() + S.x_lifted() + S.x_standing():
        d.qpos[:], d.qvel[:], d.act[:] = s[:3]
        d.ctrl[:] = 0
        d.forward()
        rec, ff = _record(d, body)
        buf.append(rec)
        seen += [(int(c[0]), int(c[1])) for c in ff]
        nrows += sum(1 for c in ff if c[4] >= 0)
    np.concatenate([[float(len(buf))]] + buf).tofile(states)
    r = subprocess.run([exe, S.WALK_BLOB, states, pairs], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr  # a sanitizer report ends the program with a non-zero status
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    print(r.stdout)
    rep = dict(line.split(None, 1) for line in r.stdout.splitlines())
    rep["oracle_pairs_seen"], rep["oracle_rows"], rep["oracle_contacts"] = seen, nrows, len(seen)
    sp, cp = set(), set()
    for line in open(pairs):
        k, a, b = line.split()
        (sp if k == "sp" else cp).add((int(a), int(b)))
    rep["sp"], rep["cp"] = sp, cp
    return rep


def test_primitive_pair_table_is_the_oracles_pair_list(host_report, oracle_pairs):
    """The sphere / capsule half of the oracle's 2 336 pairs, the floor plane's pairs left out, is `sp_mask` pair for pair."""
    ty = np.asarray(S.tables()[0]["geom_type"]).ravel()
    want = {(min(a, b), max(a, b)) for a, b in oracle_pairs if ty[a] in (2, 3) and ty[b] in (2, 3)}
    assert len(oracle_pairs) == 2336 and sum(1 for a, b in oracle_pairs if ty[a] == 0) == 48
    assert host_report["sp"] == want and int(host_report["sp_pairs"]) == len(want)
    assert int(host_report["slots"]) == 48 and int(host_report["geoms"]) == 70 and host_report["extra_untouched"] == "1"


def test_convex_candidates_are_pairs_the_oracle_collides(host_report, oracle_pairs):
    """1 058 candidates with an ellipsoid or a cylinder on one side, every one of them a pair of the oracle's list in its geom order,
    none with the floor plane."""
    ty = np.asarray(S.tables()[0]["geom_type"]).ravel()
    cp = host_report["cp"]
    assert len(cp) == int(host_report["cp_pairs"]) == 1058
    assert cp <= set(oracle_pairs)
    assert all(ty[a] >= 2 and ty[b] >= 4 for a, b in cp)


def test_every_contact_the_oracle_reports_is_a_candidate(host_report):
    """On R10, XL and XS every fly-fly contact of the oracle is a pair of `sp_mask` or of the convex candidate list (the static list of
    flybody_amd/model/reach.py prunes the oracle's 2 288 fly-fly pairs to the ones that can touch)."""
    seen = host_report["oracle_pairs_seen"]
    missing = [p for p in seen if (min(p), max(p)) not in host_report["sp"] and p not in host_report["cp"]]
    print(f"{len(seen)} fly-fly contacts, {len(set(seen))} distinct pairs")
    assert len(seen) >= 80 and not missing, missing


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_every_row_is_built(host_report, tag):
    rep = host_report
    assert int(rep[tag + "_states"]) == 24 + 2 * S.NX and int(rep[tag + "_contacts"]) == rep["oracle_contacts"]
    assert int(rep[tag + "_rows"]) == rep["oracle_rows"] >= 60
    # rows whose two chains lie in two blocks of M, and rows against a geom of the thorax (one chain), both occur
    assert int(rep[tag + "_two_block_rows"]) >= 5 and int(rep[tag + "_thorax_rows"]) >= 1


def test_formulas_equal_the_oracle_in_float64(host_report):
    for k in QUANTITIES:
        print(f"{k}: float64 relative error {float(host_report['f64_' + k]):.3e}")
    for k in QUANTITIES:
        assert float(host_report["f64_" + k]) <= F64_BOUND, (k, host_report["f64_" + k])


def test_formulas_in_float32_are_reported(host_report):
    for k in QUANTITIES:
        print(f"{k}: float32 relative error {float(host_report['f32_' + k]):.3e}")
        assert np.isfinite(float(host_report["f32_" + k]))


def _ctrls(n, seed):
    """tests/test_gpu_walk_floor.py::_ctrls, as the oracle is shown them"""
    rs = np.random.RandomState(seed)
    return [rs.uniform(-0.5, 0.5, 59).astype(np.float32).astype(np.float64) for _ in range(n)]


@pytest.mark.parametrize("which", ["R10", "XL", "XS"])
def test_the_band_leaves_out_at_most_three_states(which):
    """The 2e-6 cm band of `contact_hist` (a candidate pair that close to a switching distance) over one substep under the three flag
    sets of the GPU tests, and over ten substeps on R10: asserted here with the oracle alone, so that the seeds hold on any machine."""
    m = S.model()
    states = {"R10": S.r10, "XL": S.x_lifted, "XS": S.x_standing}[which]()
    ctrls = _ctrls(len(states), 11)
    for extra in (0, S.NO_NOSLIP, S.NO_FLUID | S.NO_ADHESION):
        out = [S.oracle_advance(m, s, c, 1, extra) for s, c in zip(states, ctrls)]
        assert sum(o[3] < S.BAND for o in out) <= 3, (which, extra)
    if which == "R10":
        ctrls = _ctrls(len(states), 3)
        out = [S.oracle_advance(m, s, c, 10, 0) for s, c in zip(states, ctrls)]
        assert sum(o[3] < S.BAND for o in out) <= 3
