"""The flight kernels read their model tables at fixed offsets of one base, not through a pointer fetched from the struct ahead of
every read: counted on the assembly by tools/isa_waits.py (one compile of the flight source with the library's own flags, about 20 s,
no GPU).  The bounds are fractions of what the same count gave for the commit before the fixed-offset arena: 69 64-bit scalar loads
in the capacity-6 step kernel, 104 global memory operations within twelve instructions of the s_load that fetched their base pair."""
import os
import sys

import pytest

from conftest import ROOT

PARENT_S_LOAD_DWORDX2 = 69
PARENT_G_SBASE_NEAR = 104


@pytest.fixture(scope="module")
def report():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import isa_waits
    finally:
        sys.path.pop(0)
    rep = {isa_waits.short(k): v for k, v in isa_waits.report(os.path.join(ROOT, "flybody_amd", "csrc")).items()}
    for k, v in rep.items():
        print(k, v)
    assert sorted(rep) == sorted(f"{f}<{c}>" for f in ("flight_step_kernel", "flight_collide_a", "flight_collide_b") for c in (6, 12)), sorted(rep)
    return rep


@pytest.mark.parametrize("capacity", [6, 12])
def test_step_kernel_fetches_no_table_pointers(report, capacity):
    r = report[f"flight_step_kernel<{capacity}>"]
    # what remains: kernel arguments, the task's table pointers (TaskDev) and pairs of neighbouring scalars of the model struct
    assert r["s_load_dwordx2"] <= PARENT_S_LOAD_DWORDX2 // 2, r
    assert r["g_sbase_near"] <= PARENT_G_SBASE_NEAR // 4, r


@pytest.mark.parametrize("capacity", [6, 12])
@pytest.mark.parametrize("fn", ["flight_collide_a", "flight_collide_b"])
def test_collision_functions_chain_no_loads(report, fn, capacity):
    """No vector load whose only use is the address of another load (the parent: 13 in flight_collide_a, 5 in flight_collide_b), and
    the struct's scalars come by s_load off the pointer made uniform at entry."""
    r = report[f"{fn}<{capacity}>"]
    assert r["v_chained"] == 0, r
    assert r["s_load"] > 0, r
