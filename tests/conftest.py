import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")
BLOB = os.path.join(ROOT, "flybody_amd", "assets", "fly_flight.ffmb")
MODEL_FIXTURE = os.path.join(GOLDEN, "fly_model")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden_quat():
    with np.load(os.path.join(GOLDEN, "quaternions.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="session")
def golden_wbpg():
    with np.load(os.path.join(GOLDEN, "wbpg.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="session")
def oracle_model():
    from oracle.oracle import OracleModel

    return OracleModel(BLOB)


@pytest.fixture(scope="session")
def wb_tables():
    from flybody_amd.tasks.synthetic import base_wing_pattern
    from flybody_amd.tasks.wbpg import build_tables

    return build_tables(base_wing_pattern())


@pytest.fixture(scope="session")
def ref_traj():
    from flybody_amd.tasks.synthetic import flight_trajectories
    from flybody_amd.tasks.trajectories import preprocess

    return preprocess(*flight_trajectories(8, 3006))


@pytest.fixture(scope="session")
def flight_model():
    """`build_flight_model()` -> (model, welded links) from the reference's MJCF and the mesh mass properties recorded from
    its meshes (tests/golden/fly_model, tools/gen_model_fixtures.py); `head_red` is still rebuilt from the stored head mesh."""
    from flybody_amd.model import compiler

    with np.load(os.path.join(MODEL_FIXTURE, "mesh_props.npz")) as f:
        st = {k: f[k] for k in f.files}
    props = {str(n): (float(v), c, i) for n, v, c, i in zip(st["names"], st["vol"], st["com"], st["inertia"])}
    raw = {str(n): (st[f"raw_verts_{n}"].astype(np.float64), st[f"raw_faces_{n}"].astype(np.int64)) for n in st["donors"]}

    class StoredMeshBank(compiler._MeshBank):
        def raw(self, name):
            return raw.get(name)

        def props(self, name):
            if name in self.reconstructed:
                return super().props(name)
            assert self.rule == str(st["rule"]), self.rule
            return props[name]

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(compiler, "_MeshBank", StoredMeshBank)
        return compiler.build_flight_model(MODEL_FIXTURE, MODEL_FIXTURE)
