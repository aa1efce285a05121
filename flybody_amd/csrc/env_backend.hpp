// env_backend.hpp - host-only: the interface between the C ABI (capi.hip) and the three kinds of env handle - flight (fly_env.hip),
// walk_on_ball (ball_env.hip), free-root walk physics (walk_env.hip) - and the host helpers every handle in csrc/ shares.
//
// Errors travel as exceptions and become the ABI's codes in one place (capi.hip): `Refused` = -1, the call was refused or its arguments
// were bad and nothing was launched; every other std::exception (HIP_OK throws std::runtime_error) = -2.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "../../include/flybody_env.h"

#define HIP_OK(expr)                                                                              \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess) throw std::runtime_error(std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

namespace ffe {

struct Refused : std::runtime_error {
  using std::runtime_error::runtime_error;
};

// Every entry point runs on the handle's device and leaves the caller's current device untouched.
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != device) { switched = (hipSetDevice(device) == hipSuccess); }
  }
  ~DeviceGuard() { if (switched && prev >= 0) (void)hipSetDevice(prev); }
  DeviceGuard(const DeviceGuard &) = delete;
  DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// `who`: the create function, for the text
inline void check_device(int device, const char *who) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) throw Refused("no HIP device: the MI355X path has no CPU fallback");
  if (device < 0 || device >= ndev) throw Refused(std::string(who) + ": no such device");
}

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
