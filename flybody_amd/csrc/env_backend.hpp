// env_backend.hpp - host-only: the interface between the C ABI (capi.hip) and the three kinds of env handle - flight (fly_env.hip),
// walk_on_ball (ball_env.hip), free-root walk physics (walk_env.hip).  A backend throws (`Refused`, HIP_OK: handle.hpp); capi.hip turns
// that into the ABI's codes through the handle layer every family shares.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "../../include/flybody_env.h"
#include "handle.hpp"

namespace ffe {

// ffe_time_kernel: events around the step kernel alone.  A launch calls start() before the step kernel, stop() right after it and
// collect() once everything else of the launch (the launch-order kernel) is queued; all three do nothing unless armed.
struct KernelTimer {
  hipEvent_t ev0 = nullptr, ev1 = nullptr;  // also the pair ffe_time_steps brackets its launches with
  bool armed = false;
  double ms = 0.0;
  KernelTimer() = default;
  KernelTimer(const KernelTimer &) = delete;
  KernelTimer &operator=(const KernelTimer &) = delete;
  ~KernelTimer() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
  void create() { HIP_OK(hipEventCreate(&ev0)); HIP_OK(hipEventCreate(&ev1)); }
  struct Armed {  // armed, from zero, for the life of this object
    KernelTimer &t;
    explicit Armed(KernelTimer &timer) : t(timer) { t.armed = true; t.ms = 0.0; }
    ~Armed() { t.armed = false; }
  };
  void start(hipStream_t s) { if (armed) HIP_OK(hipEventRecord(ev0, s)); }
  void stop(hipStream_t s) { if (armed) HIP_OK(hipEventRecord(ev1, s)); }
  void collect() {
    if (!armed) return;
    float t = 0.f;
    HIP_OK(hipEventSynchronize(ev1));
    HIP_OK(hipEventElapsedTime(&t, ev0, ev1));
    ms += t;
  }
};

// One handle kind.  The caller has made `device` current (creation, every method, the destructor).  The capabilities every kind has are
// pure; the base implementation of an optional one refuses.
struct EnvBackend {
  int device = 0, batch = 0;
  virtual ~EnvBackend() = default;  // frees what the backend owns

  virtual void spec(ffe_spec_t &s) const = 0;  // every field, offsets included (-1: not in this kind's observation row)
  virtual void action_bounds(float *mn, float *mx) const = 0;
  // mode 0 step, 1 reset all, 2 bare physics (nphys steps, act = ctrl), 3 reset the envs whose mask byte is set
  virtual void launch(const float *act, float *obs, float *rew, float *disc, int32_t *st, void *stream, int mode, int nphys, const uint8_t *mask) = 0;
  virtual void get_state(double *qpos, double *qvel, void *stream) = 0;
  virtual void set_state(const double *qpos, const double *qvel, void *stream) = 0;
  virtual void get_task_state(int32_t *ints, double *reals, void *stream) = 0;
  virtual void get_validity(int32_t *info, void *stream) = 0;  // int32[B][4], 16-byte aligned

  virtual void get_act(double *, void *) { refuse("ffe_get_act"); }
  virtual void set_act(const double *, void *) { refuse("ffe_set_act"); }
  virtual void force_next_episode(const int32_t *, const double *, void *) { refuse("ffe_force_next_episode"); }
  virtual KernelTimer *timer() { return nullptr; }  // none: ffe_time_steps / ffe_time_kernel are refused

  [[noreturn]] virtual void refuse(const char *what) const { throw Refused(std::string(what) + ": not available on this kind of handle"); }
};

}  // namespace ffe
