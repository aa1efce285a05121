"""Writes tests/golden/fly_model/: what the model-compiler tests need to recompile the flight model without the reference
checkout, whose meshes (tens of MB) cannot be committed.

    python tools/gen_model_fixtures.py <reference checkout>

* `fruitfly.xml` - the reference's MJCF model (`fruitfly/assets/fruitfly.xml`), unchanged;
* `mesh_props.npz` - per mesh the unit-density volume / centre of mass / inertia about it (scaled mesh coordinates) that
  `build_flight_model()` integrates from the meshes, and the raw triangles of the one mesh the compiler reconstructs
  another from (`head_red` from `head`), so that reconstruction still runs in the tests.

tests/conftest.py::flight_model rebuilds the model from these through a mesh bank that serves the stored values.
"""
import os
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "fly_model")
DONORS = ("head",)


def main(ref_root):
    from flybody_amd.model import compiler

    assets = os.path.join(ref_root, "vnl_ray", "fruitfly", "assets")
    msh = os.path.join(ref_root, "vnl_ray", "fruitfly", "build_fruitfly", "assets")
    banks = []

    class RecordingMeshBank(compiler._MeshBank):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            banks.append(self)

    compiler._MeshBank = RecordingMeshBank
    compiler.build_flight_model(assets, msh)
    (bank,) = banks
    names = sorted(n for n in bank.cache if n not in bank.reconstructed)
    out = {"names": np.array(names), "rule": np.array(bank.rule),
           "vol": np.array([bank.cache[n][0] for n in names]),
           "com": np.array([bank.cache[n][1] for n in names]),
           "inertia": np.array([bank.cache[n][2] for n in names]),
           "donors": np.array(DONORS)}
    for n in DONORS:
        v, f = bank.raw(n)
        v32 = v.astype(np.float32)
        assert np.array_equal(v32.astype(np.float64), v), f"{n}: vertices are not float32-exact"  # (.msh twins are float32)
        out[f"raw_verts_{n}"], out[f"raw_faces_{n}"] = v32, f.astype(np.int32)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "mesh_props.npz"), **out)
    shutil.copyfile(os.path.join(assets, "fruitfly.xml"), os.path.join(OUT, "fruitfly.xml"))
    print(f"{len(names)} meshes, donors {DONORS} -> {OUT}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
