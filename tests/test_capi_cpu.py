"""CPU-side checks of the drop-in boundary: the C ABI library builds for gfx950, loads, and exports every
symbol include/flybody_env.h declares; the Python host mirrors the reference's factory names."""
import os
import re

import pytest

from conftest import ROOT


def test_library_exports_every_declared_symbol():
    from flybody_amd import _capi, build

    build.build()
    L = _capi.lib()
    hdr = open(os.path.join(ROOT, "include", "flybody_env.h")).read()
    declared = set(re.findall(r"\b(ffe_[a-z_]+)\s*\(", hdr))
    assert declared == set(_capi.SYMBOLS)
    for s in declared:
        assert hasattr(L, s), s
    assert b"gfx950" in L.ffe_version()


def test_create_fails_loudly_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from flybody_amd import fly_envs

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fly_envs.flight_imitation(batch_size=4)


def test_factory_surface_matches_reference_names():
    from flybody_amd import fly_envs

    for name in ("flight_imitation", "walk_imitation", "walk_on_ball", "vision_guided_flight", "template_task"):
        assert callable(getattr(fly_envs, name))
    import inspect

    params = list(inspect.signature(fly_envs.flight_imitation).parameters)
    assert params[:4] == ["wpg_pattern_path", "ref_path", "random_state", "terminal_com_dist"]


def test_product_path_does_not_touch_the_oracle():
    bad = []
    for dp, _, fs in os.walk(os.path.join(ROOT, "flybody_amd")):
        for f in fs:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                txt = open(os.path.join(dp, f)).read()
                if re.search(r"(from|import)\s+oracle|fly_oracle|oracle/", txt):
                    bad.append(f)
    assert not bad, bad


def test_hdf5_converter_keeps_individual_lengths(tmp_path):
    """tools/convert_hdf5_to_npz.py (h5py is absent here, so its layout logic is driven with an in-memory stand-in for the
    HDF5 groups): every trajectory keeps its own length, as the reference serves them (trajectory_loaders.py:98-100)."""
    import sys

    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import convert_hdf5_to_npz as conv
    from flybody_amd.tasks import trajectories as T

    rng = np.random.RandomState(0)
    lens = [40, 7, 25, 3006]
    data = {}
    for i, n in enumerate(lens):
        q = rng.randn(n, 7); q[:, 3:] /= np.linalg.norm(q[:, 3:], axis=1, keepdims=True)
        data[str(i)] = (q, rng.randn(n, 6))
    dst = str(tmp_path / "set.npz")
    kept, lo, hi = conv.convert(lambda k: data[k], [str(i) for i in range(len(lens))], 2e-4, dst, min_len=8)
    assert (kept, lo, hi) == (3, 25, 3006)   # the 7-step trajectory cannot host an episode (future_steps + 2 = 7 < 8)
    qs, vs, dt = T.load_npz(dst)
    assert [len(q) for q in qs] == [40, 25, 3006] and dt == 2e-4
    assert np.array_equal(qs[1], data["2"][0]) and np.array_equal(vs[2], data["3"][1])
    refs = T.preprocess_ragged(qs, vs)
    assert refs.ntraj == 3 and refs.lengths().tolist() == [40, 25, 3006] and refs.off.tolist() == [0, 40, 65, 3071]
    # per-trajectory preprocessing == the stacked one on a trajectory of its own (xy re-centred on its first sample)
    rq, rv = T.preprocess(qs[1][None], vs[1][None])
    assert np.array_equal(refs.trajectory(1)[0], rq[0]) and np.array_equal(refs.trajectory(1)[1], rv[0])
    assert np.abs(T.root2com(refs.trajectory(2)[0])[0, :2]).max() < 1e-12


def test_env_entry_points_live_in_capi_hip():
    """Every declared `ffe_*` function is defined in exactly one file of csrc/, the env-handle ones in capi.hip."""
    from flybody_amd import build

    csrc = os.path.join(ROOT, "flybody_amd", "csrc")
    hdr = open(os.path.join(ROOT, "include", "flybody_env.h")).read()
    declared = set(re.findall(r"\b(ffe_[a-z_]+)\s*\(", hdr))
    defined = {}
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".hpp", ".inc")):
            txt = open(os.path.join(csrc, f)).read()
            # a definition: return type at the start of a line, the name, a parameter list, an opening brace
            for name in re.findall(r"^(?:const char \*|int )(ffe_[a-z_]+)\s*\([^;{]*\)\s*\{", txt, re.M):
                defined.setdefault(name, []).append(f)
    assert set(defined) >= declared, declared - set(defined)
    assert all(len(defined[n]) == 1 for n in declared), {n: defined[n] for n in declared if len(defined[n]) != 1}
    other = ("ffe_nstep_", "ffe_sampler_", "ffe_eplog_", "ffe_walktask_")
    alone = {"ffe_pack_timestep", "ffe_episode_stats", "ffe_validity_stats", "ffe_test_quat"}
    env_calls = {n for n in declared if not n.startswith(other) and n not in alone}
    assert len(env_calls) == 21 and {"ffe_create_flight", "ffe_step", "ffe_time_kernel", "ffe_destroy", "ffe_last_error"} <= env_calls
    assert {n: defined[n] for n in env_calls} == {n: ["capi.hip"] for n in env_calls}
    assert all(defined[n] != ["capi.hip"] for n in declared - env_calls)
    assert "capi.hip" in build.SOURCES and {"env_backend.hpp", "fly_env.hpp", "ball_env.hpp", "walk_env.hpp"} <= set(build.HEADERS)


def test_python_handles_share_one_base():
    import inspect

    from flybody_amd._capi import LibHandle
    from flybody_amd.batched_env import BatchedBallEnv, BatchedFlyEnv, BatchedWalkPhysics, EnvHandle

    assert inspect.getmro(BatchedFlyEnv)[1] is EnvHandle and inspect.getmro(BatchedWalkPhysics)[1] is EnvHandle
    assert inspect.getmro(BatchedBallEnv)[1] is BatchedFlyEnv and inspect.getmro(EnvHandle)[1] is LibHandle
    owns_handle = ("_check", "close", "__del__")  # what every handle family shares, envs or not
    for name in owns_handle + ("_stream", "raw_action_bounds", "get_state", "set_state", "physics_step", "get_task_state", "get_act", "set_act"):
        owners = [c for c in (LibHandle, EnvHandle, BatchedFlyEnv, BatchedBallEnv, BatchedWalkPhysics) if name in vars(c)]
        assert owners == [LibHandle if name in owns_handle else EnvHandle], (name, owners)
        assert getattr(BatchedWalkPhysics, name) is getattr(BatchedFlyEnv, name) is getattr(BatchedBallEnv, name)
    assert (BatchedFlyEnv.task_kind, BatchedBallEnv.task_kind, BatchedWalkPhysics.task_kind) == ("flight_imitation", "walk_on_ball", "walk_physics")


def test_every_handle_family_shares_the_owning_base():
    """`close`, `__del__` and `_check` exist once, in `_capi.LibHandle`; a family may extend `close` (the tracker synchronises first, the
    log drops its views) and names its own destroy / last_error symbols, which the library exports."""
    from flybody_amd import _capi
    from flybody_amd.actor_loop import EpisodeLog, NStepTransitionWriter, ReplaySampler
    from flybody_amd.batched_env import EnvHandle
    from flybody_amd.tasks.walk_tracker import WalkTracker

    for cls in (NStepTransitionWriter, ReplaySampler, EpisodeLog, WalkTracker, EnvHandle):
        assert issubclass(cls, _capi.LibHandle)
        assert "__del__" not in vars(cls) and "_check" not in vars(cls), cls
        assert cls._destroy in _capi.SYMBOLS and cls._last_error in _capi.SYMBOLS, cls
    assert [c.__name__ for c in (NStepTransitionWriter, ReplaySampler, EpisodeLog, WalkTracker, EnvHandle) if "close" in vars(c)] == ["EpisodeLog", "WalkTracker"]
