"""The selectable contact capacity of flight handles (6, the default, or 12), as far as it can be checked without a GPU: the option
is there at every layer, and the library carries one instantiation of the flight step kernel per capacity."""
import ctypes as C
import inspect
import os
import re

from conftest import ROOT


def test_option_is_declared_at_every_layer():
    from flybody_amd import _capi
    from flybody_amd.batched_env import BatchedFlyEnv

    p = inspect.signature(BatchedFlyEnv.__init__).parameters
    assert "contact_capacity" in p and p["contact_capacity"].default == 6
    assert _capi.FlightTask._fields_[-1] == ("contact_capacity", C.c_int32)
    hdr = open(os.path.join(ROOT, "include", "flybody_env.h")).read()
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\}\s*ffe_flight_task;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    assert fields[-1] == "int32_t contact_capacity", fields[-1]
    # same size and field order on both sides of the ABI
    names = [n for f in fields for n in re.sub(r"^(const\s+)?\w+\s*", "", f).replace("*", "").split(",")]
    assert [n.strip() for n in names] == [n for n, _ in _capi.FlightTask._fields_]


def test_library_carries_one_step_kernel_per_capacity():
    """`hipcc -Rpass-analysis=kernel-resource-usage` on the flight source with the library's flags: two instantiations of the step
    kernel; the default one keeps its 10 128-byte tile (16 waves of 10 240 B fill a CU's 160 KB exactly).  The figures of the
    capacity-12 kernel are printed for the record."""
    from flybody_amd import build

    build.build()
    use = build.kernel_resource_usage()
    for k, v in use.items():
        print(k, v)
    by_cap = {int(re.search(r"flight_step_kernelILi(\d+)E", k).group(1)): v for k, v in use.items()}
    assert sorted(by_cap) == [6, 12], sorted(by_cap)
    assert by_cap[6]["LDS Size"] == 10128
