"""Validity reporting (ffe_get_validity, the n-step writer's taint column, the actor loop's flagged totals): everything that needs
no device - the declared and exported entry points, a pure-Python restatement of the taint rule on hand-made sequences (the GPU
test compares the device writer against the same restatement), and the argument checks of the Python layer."""
import os
import re

import pytest

from conftest import ROOT
from nstep_restatement import taint_restatement  # noqa: F401  (tests/test_gpu_validity.py imports it from here)

NEW_SYMBOLS = ("ffe_get_validity", "ffe_validity_stats", "ffe_nstep_create_tracked", "ffe_nstep_observe_flagged", "ffe_nstep_taint_buffer")


def test_header_declares_and_library_exports_the_validity_entry_points():
    from flybody_amd import _capi, build

    build.build()
    L = _capi.lib()
    hdr = open(os.path.join(ROOT, "include", "flybody_env.h")).read()
    declared = set(re.findall(r"\b(ffe_[a-z_]+)\s*\(", hdr))
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in _capi.SYMBOLS, s
        assert hasattr(L, s), s
    # the signatures the issue fixes
    flat = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert "int ffe_get_validity(ffe_handle h, int32_t *info_dev, void *stream);" in flat
    assert "int ffe_nstep_taint_buffer(ffe_nstep_handle h, uint8_t **taint );" in flat
    assert "int ffe_validity_stats(const int32_t *step_type_dev, const int32_t *info_dev, long long *totals_dev, int batch, void *stream);" in flat
    assert re.search(r"int ffe_nstep_observe_flagged\(ffe_nstep_handle h, const float \*action_dev, const int32_t \*step_type_dev, const float \*reward_dev, "
                     r"const float \*discount_dev, const float \*obs_dev, const int32_t \*step_bits_dev, int stride_ints, void \*stream\);", flat)


def test_flag_on_a_first_call_taints_the_first_entry():
    assert taint_restatement([0, 1, 1, 1], [1, 0, 0, 0], 1) == [1, 0, 0]
    assert taint_restatement([0, 1, 1, 1], [2, 0, 0, 0], 1) == [1, 0, 0]       # any bit counts
    # a FIRST in the middle: the flag of the LAST row before it does not cross the episode boundary, the FIRST row's own does
    assert taint_restatement([0, 1, 2, 0, 1, 1], [0, 0, 1, 0, 0, 0], 1) == [0, 1, 0, 0]
    assert taint_restatement([0, 1, 2, 0, 1, 1], [0, 0, 0, 1, 0, 0], 1) == [0, 0, 1, 0]


def test_flag_at_step_t_taints_entries_t_and_t_plus_one():
    assert taint_restatement([0, 1, 1, 1, 1], [0, 0, 1, 0, 0], 1) == [0, 1, 1, 0]
    assert taint_restatement([0, 1, 1, 1, 1, 1], [0, 0, 1, 1, 0, 0], 1) == [0, 1, 1, 1, 0]


def test_taint_leaves_a_five_step_window_after_the_expected_number_of_steps():
    T, t_flag, n = 16, 3, 5
    st, bits = [0] + [1] * (T - 1), [0] * T
    bits[t_flag] = 1
    got = taint_restatement(st, bits, n)   # got[t - 1] = the transition written at step t, spanning entries max(1, t - n + 1) .. t
    # marked entries: t_flag and t_flag + 1; the last window that holds entry t_flag + 1 is the one written at step t_flag + 1 + n - 1
    want = [int(t_flag <= t <= t_flag + n) for t in range(1, T)]
    assert got == want and sum(got) == n + 1
    assert got == [0, 0, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]


def test_last_tails_get_the_suffix_or():
    # entries 1 .. 4 marked [0, 1, 1, 0]; steps 1 .. 3 write one transition each, LAST writes the four suffixes
    assert taint_restatement([0, 1, 1, 1, 2], [0, 0, 1, 0, 0], 5) == [0, 1, 1] + [1, 1, 1, 0]
    # with a window of 2 the LAST step holds entries 3, 4 (marks [1, 0])
    assert taint_restatement([0, 1, 1, 1, 2], [0, 0, 1, 0, 0], 2) == [0, 1, 1] + [1, 0]
    # flag on the LAST row itself: every tail ends in the marked entry
    assert taint_restatement([0, 1, 1, 2], [0, 0, 0, 4], 5) == [0, 0] + [1, 1, 1]


def test_env_classes_name_their_task_kind():
    from flybody_amd.batched_env import BatchedBallEnv, BatchedFlyEnv, Validity

    assert BatchedFlyEnv.task_kind == "flight_imitation" and BatchedBallEnv.task_kind == "walk_on_ball"
    assert Validity._fields == ("step_bits", "episode_flagged_steps", "episode_bits", "episode_steps")
    assert callable(BatchedFlyEnv.validity) and BatchedBallEnv.validity is BatchedFlyEnv.validity


def test_writer_and_loop_argument_checks_need_no_device():
    import torch

    from flybody_amd.actor_loop import BatchedActorLoop, GroupedActorLoop, NStepTransitionWriter, _step_bits_arg

    with pytest.raises(TypeError, match="track_validity"):
        NStepTransitionWriter(4, 8, 2, track_validity="yes")
    with pytest.raises(ValueError, match="n_step"):
        NStepTransitionWriter(4, 8, 2, n_step=0, track_validity=True)
    dev = torch.device("cuda", 0)
    with pytest.raises(TypeError, match="int32"):
        _step_bits_arg(torch.zeros(4), 4, dev)
    with pytest.raises(TypeError, match="int32"):
        _step_bits_arg([0, 0, 0, 0], 4, dev)
    with pytest.raises(ValueError, match="device"):
        _step_bits_arg(torch.zeros(4, dtype=torch.int32), 4, dev)      # a host tensor
    with pytest.raises(TypeError, match="track_validity"):
        BatchedActorLoop(object(), None, track_validity=1)

    class _Adder:
        track_validity = False

    with pytest.raises(ValueError, match="agree"):
        BatchedActorLoop(object(), None, adder=_Adder(), track_validity=True)
    import inspect

    assert list(inspect.signature(BatchedActorLoop.__init__).parameters)[1:] == ["env", "policy", "adder", "track_validity"]
    assert "track_validity" in inspect.signature(GroupedActorLoop.__init__).parameters
    assert inspect.signature(NStepTransitionWriter.observe).parameters["step_bits"].default is None
    assert inspect.signature(NStepTransitionWriter.transitions).parameters["with_taint"].default is False
