"""What the compiler reports for the two instantiations of the flight step kernel (`hipcc -Rpass-analysis=kernel-resource-usage` with
the library's own flags; one compile of the flight source, about 20 s, no GPU): the kernel keeps its occupancy and its tile, and its
own frame holds no spill - the private segment is what the two collision functions it calls need for theirs."""
import re

import pytest

# bytes per lane: flight_collide_b's frame (its callee-saved registers), the larger of the two callees'.  The step kernel's own frame
# is empty.  (Before the stages took their lane id and flag word afresh: 268 B at capacity 6, 316 B at capacity 12.)
SCRATCH_BYTES = 124
# registers the step kernel itself spills to that frame.  (Before: 54 at capacity 6, 64 at capacity 12.)
VGPR_SPILLS = 0
# wave-uniform values parked in lanes of a VGPR (task values and kernel arguments the epilogue needs), capacity 6 / 12.  (Before: 123 / 176.)
SGPR_SPILLS = {6: 62, 12: 119}


@pytest.fixture(scope="module")
def usage():
    from flybody_amd import build

    use = build.kernel_resource_usage()
    for k, v in use.items():
        print(k, v)
    by_cap = {int(re.search(r"flight_step_kernelILi(\d+)E", k).group(1)): v for k, v in use.items()}
    assert sorted(by_cap) == [6, 12], sorted(by_cap)
    return by_cap


@pytest.mark.parametrize("capacity", [6, 12])
def test_step_kernel_keeps_occupancy_and_tile(usage, capacity):
    u = usage[capacity]
    assert u["VGPRs"] <= 128 and u["Occupancy"] == 4, u
    assert u["LDS Size"] == 10128, u


@pytest.mark.parametrize("capacity", [6, 12])
def test_step_kernel_has_no_frame_of_its_own(usage, capacity):
    u = usage[capacity]
    assert u["ScratchSize"] <= SCRATCH_BYTES, u
    assert u["VGPRs Spill"] <= VGPR_SPILLS, u
    assert u["SGPRs Spill"] <= SGPR_SPILLS[capacity], u
