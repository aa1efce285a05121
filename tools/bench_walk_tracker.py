"""The walk_imitation task layer on the device (flybody_amd/csrc/walk_task.hip, `tasks/walk_tracker.py`):

 * float64 `walking.featurize` on 65 536 raw pose rows - end to end (host packing, upload, kernel, download) and the features kernel
   alone - against numpy `walking.walker_features`, measured in the same run over 200 rows;
 * float32 `WalkTracker.evaluate` with all outputs at N = 4 096 and 8 192.

Timing: device events around 200 calls of the C entry point (outputs allocated once) per window, every shape warmed first
(20 calls), 5 windows; the spread is max - min over the windows.  The bytes a state needs are computed from the handle's dimensions: its own qpos / qvel / clip / step, the reference
rows it reads (one row of qvel, root2site, joint_quat and 65 rows of the compact root table) and what it writes; the model tables
(shared by all rows, cache-resident) are left out.  Nobody has measured these before: there is no threshold, the log reports.
Needs an MI355X; fails without one.    python tools/bench_walk_tracker.py [--out profiles/walk_tracker_bench.log]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch

from flybody_amd.tasks import walking as W
from flybody_amd.tasks.walk_tracker import WalkTracker

WARMUP, CALLS, WINDOWS = 20, 200, 5
FEATURIZE_ROWS, NUMPY_ROWS = 65536, 200
HBM_PEAK = 8.0e12  # bytes/s, MI355X data sheet (about 6.3e12 is reachable by a plain copy)


def windows(fn):
    """us per call in each of WINDOWS windows of CALLS calls"""
    for _ in range(WARMUP):
        fn()
    out = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / CALLS)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "profiles", "walk_tracker_bench.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_walk_tracker: no GPU - this measurement has no CPU fallback")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    med = lambda x: sorted(x)[len(x) // 2]  # noqa: E731
    view = W.WalkModelView()
    refs = W.WalkRefSet(W.synthetic_snippets(view, n=3, length=100))
    J, S = len(view.mocap_jnt), len(view.mocap_site)
    say(f"walk task layer; device: {torch.cuda.get_device_name(0)}; {WARMUP} warm-up + {CALLS} timed calls per window, {WINDOWS} windows")

    # ---- featurize, float64
    rng = np.random.RandomState(0)
    reps = -(-FEATURIZE_ROWS // len(refs.qpos))
    qrows = np.tile(refs.qpos, (reps, 1))[:FEATURIZE_ROWS].copy()
    vrows = np.tile(refs.qvel, (reps, 1))[:FEATURIZE_ROWS].copy()
    qrows[:, 7:] += rng.normal(0, 0.02, qrows[:, 7:].shape)
    off = np.array([0, FEATURIZE_ROWS])
    W.featurize(view, qrows[:1024], vrows[:1024], [0, 1024])  # warm: library load, first launch
    t0 = time.perf_counter()
    out = W.featurize(view, qrows, vrows, off)
    wall = time.perf_counter() - t0
    t0 = time.perf_counter()
    want = [W.walker_features(view, view.full_qpos(qrows[i]), np.zeros(view.nv)) for i in range(NUMPY_ROWS)]
    wall_np = time.perf_counter() - t0
    err = max(np.abs(out.root2site[i] - want[i]["root2site"]).max() for i in range(NUMPY_ROWS))
    errq = max(np.abs(out.joint_quat[i] - want[i]["joint_quat"][1:]).max() for i in range(NUMPY_ROWS))
    say(f"featurize float64, {FEATURIZE_ROWS} rows end to end: {wall * 1e3:.1f} ms = {FEATURIZE_ROWS / wall:,.0f} rows/s | numpy walker_features, "
        f"{NUMPY_ROWS} rows: {wall_np * 1e3:.1f} ms = {NUMPY_ROWS / wall_np:,.0f} rows/s | ratio {FEATURIZE_ROWS / wall / (NUMPY_ROWS / wall_np):,.0f} | "
        f"max |difference| on those rows: root2site {err:.1e}, joint_quat {errq:.1e}")
    tr = WalkTracker(None, view, dtype="float64")
    full = np.tile(view.m.qpos0.astype(np.float64), (FEATURIZE_ROWS, 1))
    full[:, :7], full[:, view.mocap_qadr], full[:, view.retract_qadr] = qrows[:, :7], qrows[:, 7:], view.retract_val
    q, v = torch.as_tensor(full, device="cuda"), torch.zeros((FEATURIZE_ROWS, view.nv), dtype=torch.float64, device="cuda")
    ft = tr.features(q, v)
    call = (tr._h, q.data_ptr(), v.data_ptr(), FEATURIZE_ROWS, ft.com.data_ptr(), ft.qvel.data_ptr(), ft.root2site.data_ptr(), ft.joint_quat.data_ptr(), tr._stream())
    w = windows(lambda: tr._L.ffe_walktask_features(*call))
    say(f"features kernel float64 alone, N {FEATURIZE_ROWS}: {med(w):.1f} us/call (windows {', '.join(f'{x:.1f}' for x in w)}; spread {max(w) - min(w):.1f} us) = "
        f"{FEATURIZE_ROWS / med(w) * 1e6:,.0f} rows/s")
    tr.close()

    # ---- evaluate, float32, all outputs
    tr = WalkTracker(refs, view, dtype="float32")
    F1 = tr.future_steps + 1
    kin = sum(wd for _, wd in tr.obs_layout.values())
    read = tr.nq * 8 + tr.nv * 8 + 8 + (6 + J) * 4 + 3 * S * 4 + 4 * J * 4 + F1 * 7 * 8
    write = 4 * 4 + 4 + 4 + kin * 4
    say(f"bytes a state needs: read {read} (qpos {tr.nq * 8}, qvel {tr.nv * 8}, clip + step 8, reference row {(6 + J) * 4 + 3 * S * 4 + 4 * J * 4}, "
        f"{F1} preview rows {F1 * 56}) + written {write} (factors 16, reward 4, term_bits 4, {kin} observation columns {kin * 4}) = {read + write}")
    for N in (4096, 8192):
        idx = rng.randint(len(refs.qpos), size=N)
        clip = (np.searchsorted(refs.off, idx, side="right") - 1).astype(np.int32)
        step = np.minimum(idx - refs.off[clip], tr.episode_steps[clip]).astype(np.int32)
        qp = np.array([view.full_qpos(refs.qpos[refs.off[c] + k]) for c, k in zip(clip, step)])
        qp[:, view.mocap_qadr] += rng.normal(0, 0.05, (N, J))
        q, v = torch.as_tensor(qp, device="cuda"), torch.as_tensor(rng.normal(0, 5, (N, view.nv)), device="cuda")
        c, k = torch.as_tensor(clip, device="cuda"), torch.as_tensor(step, device="cuda")
        obs = torch.zeros((N, tr.obs_dim), device="cuda")
        ev = tr.evaluate(q, v, c, k, obs=obs)  # the outputs of the timed calls: allocated once, so a window times the launches alone
        stream, L = tr._stream(), tr._L
        call = (tr._h, q.data_ptr(), v.data_ptr(), c.data_ptr(), k.data_ptr(), N, ev.factors.data_ptr(), ev.reward.data_ptr(), ev.term_bits.data_ptr(),
                obs.data_ptr(), tr.obs_dim, stream)
        w = windows(lambda: L.ffe_walktask_evaluate(*call))
        bps = N * (read + write) / (med(w) * 1e-6)
        say(f"evaluate float32, all outputs, N {N}: {med(w):.1f} us/call (windows {', '.join(f'{x:.1f}' for x in w)}; spread {max(w) - min(w):.1f} us) = "
            f"{med(w) * 1e3 / N:.2f} ns/state, {bps * 1e-9:.1f} GB/s achieved on {N * (read + write)} bytes = {100 * bps / HBM_PEAK:.1f} % of the {HBM_PEAK * 1e-12:.0f} TB/s peak")
        say(f"    -> bound by {'memory traffic' if bps > 0.5 * HBM_PEAK else 'the latency of the 9-level kinematic chain (one wave per state, at most 12 lanes busy per level), not by memory'}")
    tr.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
