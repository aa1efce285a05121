// capi.hip - the env-handle entry points of include/flybody_env.h (host code only): argument checks, the handle's device, and the
// mapping of the backends' exceptions to the ABI's return codes (the table in the header).  What a handle does lives behind EnvBackend
// (env_backend.hpp): fly_env.hip, ball_env.hip, walk_env.hip.
#include <memory>
#include <string>

#include "env_backend.hpp"
#include "fly_env.hpp"
#include "ball_env.hpp"
#include "walk_env.hpp"

using ffe::EnvBackend;
using ffe::need;
using ffe::Refused;

struct ffe_env {
  std::unique_ptr<EnvBackend> be;
  int device = 0;
  std::string err;
};

static thread_local std::string g_err;  // of the create functions

// Every call on a handle goes through the handle layer (handle.hpp): on the handle's device, -1 when the backend (or `body` itself)
// refuses, -2 on any other failure, the text in the handle.  A NULL handle has nowhere to put one, and this family writes none.
template <class F>
static int on_handle(ffe_handle h, F &&body) {
  return ffe::on_handle(h, "", nullptr, [&](ffe_env &e) { body(*e.be); });
}

// Every create: `make` runs on `device`; whatever it throws is a refusal (-1) with the text in ffe_last_error(NULL).
template <class F>
static int create(const char *who, bool args_ok, int device, ffe_handle *out, F &&make) {
  return ffe::create(out, nullptr, g_err, [&](ffe_env &e) {
    if (!args_ok) throw Refused(std::string(who) + ": bad arguments");
    ffe::check_device(device, who);
    ffe::DeviceGuard guard(device);
    e.device = device;
    e.be = make();
  });
}

static int launch_step(ffe_handle h, const float *act, float *obs, float *rew, float *disc, int32_t *st, void *stream, int mode,
                       const uint8_t *mask = nullptr) {
  return on_handle(h, [&](EnvBackend &be) {
    need(mode != 3 || mask, "null reset mask");
    be.launch(act, obs, rew, disc, st, stream, mode, 0, mask);
  });
}

extern "C" {

const char *ffe_version(void) { return "flybody_amd 0.1 (gfx950, wave-per-env)"; }
const char *ffe_last_error(ffe_handle h) { return h ? h->err.c_str() : g_err.c_str(); }

int ffe_create_flight(const void *model_blob, size_t blob_size, const ffe_flight_task *task, int batch, int device, uint64_t seed,
                      uint64_t env_id_base, ffe_handle *out) {
  return create("ffe_create_flight", model_blob && task && batch > 0, device, out,
                [&] { return ffe::flight_create(model_blob, blob_size, *task, batch, device, seed, env_id_base); });
}
int ffe_create_walk_on_ball(const void *model_blob, size_t blob_size, const ffe_ball_task *task, int batch, int device, ffe_handle *out) {
  return create("ffe_create_walk_on_ball", task != nullptr, device, out, [&] {
    const ffb::BallTaskHost t{task->time_limit_steps, task->pad_first_obs, task->physics_flags, task->canonical_actions, task->clip_actions,
                              task->control_timestep};
    return ffb::ball_create(model_blob, blob_size, t, batch, device);
  });
}
int ffe_create_walk_physics(const void *model_blob, size_t blob_size, const ffe_walk_physics_task *task, int batch, int device, ffe_handle *out) {
  return create("ffe_create_walk_physics", task != nullptr, device, out,
                [&] { return ffw::walk_create(model_blob, blob_size, *task, batch, device); });
}

int ffe_destroy(ffe_handle h) { return ffe::destroy(h, "", nullptr); }

int ffe_spec(ffe_handle h, ffe_spec_t *s) {
  return on_handle(h, [&](EnvBackend &be) { need(s, "ffe_spec: null spec"); be.spec(*s); });
}
int ffe_action_bounds(ffe_handle h, float *mn, float *mx) {
  return on_handle(h, [&](EnvBackend &be) { need(mn && mx, "ffe_action_bounds: null buffer"); be.action_bounds(mn, mx); });
}

int ffe_reset(ffe_handle h, float *obs, float *rew, float *disc, int32_t *st, void *stream) { return launch_step(h, nullptr, obs, rew, disc, st, stream, 1); }
int ffe_reset_envs(ffe_handle h, const uint8_t *mask, float *obs, float *rew, float *disc, int32_t *st, void *stream) {
  return launch_step(h, nullptr, obs, rew, disc, st, stream, 3, mask);
}
int ffe_step(ffe_handle h, const float *act, float *obs, float *rew, float *disc, int32_t *st, void *stream) {
  return launch_step(h, act, obs, rew, disc, st, stream, 0);
}
int ffe_physics_step(ffe_handle h, const float *ctrl, int nsteps, void *stream) {
  return on_handle(h, [&](EnvBackend &be) {
    need(ctrl && nsteps > 0, "ffe_physics_step: null ctrl or nsteps < 1");
    be.launch(ctrl, nullptr, nullptr, nullptr, nullptr, stream, 2, nsteps, nullptr);
  });
}

int ffe_force_next_episode(ffe_handle h, const int32_t *traj, const double *phase, void *stream) {
  return on_handle(h, [&](EnvBackend &be) { need(traj && phase, "ffe_force_next_episode: null array"); be.force_next_episode(traj, phase, stream); });
}

int ffe_get_state(ffe_handle h, double *qpos, double *qvel, void *stream) {
  return on_handle(h, [&](EnvBackend &be) { need(qpos && qvel, "ffe_get_state: null buffer"); be.get_state(qpos, qvel, stream); });
}
int ffe_set_state(ffe_handle h, const double *qpos, const double *qvel, void *stream) {
  return on_handle(h, [&](EnvBackend &be) { need(qpos && qvel, "ffe_set_state: null buffer"); be.set_state(qpos, qvel, stream); });
}
int ffe_get_act(ffe_handle h, double *act_dev, void *stream) {
  return on_handle(h, [&](EnvBackend &be) { need(act_dev, "ffe_get_act: null buffer"); be.get_act(act_dev, stream); });
}
int ffe_set_act(ffe_handle h, const double *act_dev, void *stream) {
  return on_handle(h, [&](EnvBackend &be) { need(act_dev, "ffe_set_act: null buffer"); be.set_act(act_dev, stream); });
}
int ffe_get_validity(ffe_handle h, int32_t *info, void *stream) {
  return on_handle(h, [&](EnvBackend &be) {
    need(info && !(reinterpret_cast<uintptr_t>(info) & 15), "ffe_get_validity: info_dev must be a 16-byte aligned device buffer");
    be.get_validity(info, stream);
  });
}
int ffe_get_task_state(ffe_handle h, int32_t *ints, double *reals, void *stream) {
  return on_handle(h, [&](EnvBackend &be) { need(ints && reals, "ffe_get_task_state: null buffer"); be.get_task_state(ints, reals, stream); });
}

// mean milliseconds per step launch, by the backend's event pair around all `iters` launches
int ffe_time_steps(ffe_handle h, const float *act, float *obs, float *rew, float *disc, int32_t *st, int iters, void *stream, float *ms) {
  return on_handle(h, [&](EnvBackend &be) {
    need(ms && iters > 0, "ffe_time_steps: null ms or iters < 1");
    ffe::KernelTimer *t = be.timer();
    if (!t) be.refuse("ffe_time_steps");
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_OK(hipEventRecord(t->ev0, s));
    for (int i = 0; i < iters; i++) be.launch(act, obs, rew, disc, st, stream, 0, 0, nullptr);
    HIP_OK(hipEventRecord(t->ev1, s));
    HIP_OK(hipEventSynchronize(t->ev1));
    float total = 0.f;
    HIP_OK(hipEventElapsedTime(&total, t->ev0, t->ev1));
    *ms = total / (float)iters;
  });
}

// ... and of the step kernel alone: the backend's launch brackets it while the timer is armed
int ffe_time_kernel(ffe_handle h, const float *act, float *obs, float *rew, float *disc, int32_t *st, int iters, void *stream, float *ms) {
  return on_handle(h, [&](EnvBackend &be) {
    need(ms && iters > 0, "ffe_time_kernel: null ms or iters < 1");
    ffe::KernelTimer *t = be.timer();
    if (!t) be.refuse("ffe_time_kernel");
    ffe::KernelTimer::Armed armed(*t);
    for (int i = 0; i < iters; i++) be.launch(act, obs, rew, disc, st, stream, 0, 0, nullptr);
    *ms = (float)(t->ms / iters);
  });
}

}  // extern "C"
