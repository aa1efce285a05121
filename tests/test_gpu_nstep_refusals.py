"""The n-step writer's argument refusals on the smallest legal ring (batch 2, obs_dim 3, act_dim 2, n_step 2, capacity 4): a refused
call says which function refused it - on the handle, or in `ffe_nstep_last_error(NULL)` when there is no handle - launches nothing,
and leaves the writer usable.  Only arguments are refused here: no bad pointers, no exhausted memory."""
import ctypes as C

import pytest

from test_gpu_parity import torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu


def test_nstep_refusals_have_texts_and_launch_nothing(torch_mod):
    torch = torch_mod
    from flybody_amd.actor_loop import NStepTransitionWriter
    from flybody_amd.dm_types import StepType, TimeStep

    B, O, A = 2, 3, 2
    w = NStepTransitionWriter(B, O, A, n_step=2, discount=0.5, capacity=4)
    L, h, dev = w._L, w._h, w.device
    act = torch.ones(B, A, device=dev)
    obs = torch.arange(B * O, dtype=torch.float32, device=dev).reshape(B, O)
    rew, disc = torch.ones(B, device=dev), torch.ones(B, device=dev)
    first = torch.full((B,), int(StepType.FIRST), dtype=torch.int32, device=dev)
    mid = torch.tensor([int(StepType.MID), int(StepType.FIRST)], dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    args = [act.data_ptr(), first.data_ptr(), rew.data_ptr(), disc.data_ptr(), obs.data_ptr()]

    # no handle: the text is the family's
    assert L.ffe_nstep_observe(None, *args, stream) == -1
    assert L.ffe_nstep_last_error(None).decode() == "ffe_nstep_observe: null handle"
    # one NULL input at a time: the text is the handle's and names the function
    for k in range(len(args)):
        bad = list(args)
        bad[k] = None
        assert L.ffe_nstep_observe(h, *bad, stream) == -1, k
        text = L.ffe_nstep_last_error(h).decode()
        print(k, repr(text))
        assert text and "ffe_nstep_observe" in text, (k, text)
    assert w.num_written() == 0
    # an untracked writer has no taint column
    p = C.c_void_p()
    assert L.ffe_nstep_taint_buffer(h, C.byref(p)) == -1 and p.value is None
    assert "without validity tracking" in L.ffe_nstep_last_error(h).decode()
    assert L.ffe_nstep_observe_flagged(h, *args, first.data_ptr(), 1, stream) == -1
    assert "without validity tracking" in L.ffe_nstep_last_error(h).decode()
    assert w.num_written() == 0

    # the writer is as it was: FIRST for both envs, then MID for env 0 (env 1 starts over) writes env 0's one-step transition
    w.observe(act, TimeStep(first, rew, disc, None), obs)
    assert w.num_written() == 0
    w.observe(act, TimeStep(mid, rew, disc, None), obs + 1)
    assert w.num_written() == 1
    o, a, r, d, o2 = (x.cpu() for x in w.transitions())
    assert o.tolist() == [[0.0, 1.0, 2.0]] and o2.tolist() == [[1.0, 2.0, 3.0]] and a.tolist() == [[1.0, 1.0]]
    assert r.tolist() == [1.0] and d.tolist() == [1.0]

    w._h = None  # destroyed by hand below
    assert L.ffe_nstep_destroy(h) == 0
    assert L.ffe_nstep_destroy(None) == -1
    assert L.ffe_nstep_last_error(None).decode() == "ffe_nstep_destroy: null handle"
