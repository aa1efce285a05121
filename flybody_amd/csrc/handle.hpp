// handle.hpp - host-only: what every handle family of include/flybody_env.h shares (env handles in capi.hip, the n-step writer in
// nstep.hip, the sampler in replay.hip, the episode log in episode_log.hip, the walk task in walk_task.hip).
//
// Errors travel as exceptions and become the ABI's codes in one place (on_handle / create below): `Refused` = -1, the call was refused
// or its arguments were bad and nothing was launched; every other std::exception (HIP_OK throws std::runtime_error) = -2.  Nothing
// crosses extern "C".  A handle type has `int device` and `std::string err`; a family has one thread-local string for the texts of its
// create function and of calls on a NULL handle.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#define HIP_OK(expr)                                                                              \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess) throw std::runtime_error(std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

namespace ffe {

struct Refused : std::runtime_error {
  using std::runtime_error::runtime_error;
};

// a bad argument is a refusal with a text
inline void need(bool ok, const char *text) {
  if (!ok) throw Refused(text);
}

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

// `who`: the create function, for the text.  The env creates tell a machine without devices from a bad index; the four small
// families say `one_text` for both.
inline void check_device(int device, const char *who, bool one_text = false) {
  int ndev = 0;
  const bool none = hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0, bad = none || device < 0 || device >= ndev;
  if (one_text && bad) throw Refused(std::string(who) + ": no such HIP device: the MI355X path has no CPU fallback");
  if (none) throw Refused("no HIP device: the MI355X path has no CPU fallback");
  if (bad) throw Refused(std::string(who) + ": no such device");
}

// The device memory a handle owns: zero-filled when made, on the device that is current then, freed with the holder.
struct DeviceBuffers {
  const char *who;  // the create function that fills it, for the text
  int device = -1;
  std::vector<void *> ptrs;
  explicit DeviceBuffers(const char *create_function) : who(create_function) {}
  DeviceBuffers(const DeviceBuffers &) = delete;
  DeviceBuffers &operator=(const DeviceBuffers &) = delete;
  ~DeviceBuffers() {
    if (ptrs.empty()) return;
    DeviceGuard guard(device);
    for (void *p : ptrs) (void)hipFree(p);
  }
  template <class T>
  T *zeroed(size_t count) {
    const size_t bytes = count * sizeof(T);
    void *p = nullptr;
    ptrs.reserve(ptrs.size() + 1);
    if (ptrs.empty()) HIP_OK(hipGetDevice(&device));
    if (hipMalloc(&p, bytes) != hipSuccess) throw Refused(std::string(who) + ": out of device memory");
    ptrs.push_back(p);
    if (hipMemset(p, 0, bytes) != hipSuccess) throw Refused(std::string(who) + ": out of device memory");
    return static_cast<T *>(p);
  }
  // the fills have landed: whatever stream reads the memory next finds the zeros
  void ready() {
    if (hipDeviceSynchronize() != hipSuccess) throw Refused(std::string(who) + ": out of device memory");
  }
};

// After a kernel launch: the text of the error if it was not accepted, else null.
inline const char *launch_error() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}
inline void launched(const char *who) {
  if (const char *text = launch_error()) throw std::runtime_error(std::string(who) + ": " + text);
}

// the text of `e` into `*err` (null: nowhere to put one), `rc` back
inline int failed(std::string *err, const std::exception &e, int rc) noexcept {
  try {
    if (err) *err = e.what();
  } catch (...) {
  }
  return rc;
}

// Every call on a handle: `body(*h)` on the handle's device, -1 when it refuses, -2 on any other failure; both leave the text in the
// handle.  A NULL handle is refused with "<who>: null handle" in `*null_err`, the family's string (null: the family writes none).
template <class H, class F>
int on_handle(H *h, const char *who, std::string *null_err, F &&body) {
  std::string *err = h ? &h->err : null_err;
  try {
    if (!h) throw Refused(std::string(who) + ": null handle");
    DeviceGuard guard(h->device);
    body(*h);
  } catch (const Refused &e) {
    return failed(err, e, -1);
  } catch (const std::exception &e) {
    return failed(err, e, -2);
  }
  return 0;
}

// ... and the one that ends it
template <class H>
int destroy(H *h, const char *who, std::string *null_err) {
  if (!h) return on_handle(h, who, null_err, [](H &) {});
  DeviceGuard guard(h->device);
  delete h;
  return 0;
}

// Every create: `fill(h)` on a fresh handle checks the arguments, then the device (check_device), makes it current (DeviceGuard) and
// builds what the handle owns.  Whatever it throws is a refusal (-1) with the text in `err`, the family's string, and *out stays NULL.
// A NULL `out` is refused with `null_out` (null: no text).
template <class H, class F>
int create(H **out, const char *null_out, std::string &err, F &&fill) {
  try {
    if (!out) throw Refused(null_out ? null_out : "");
    *out = nullptr;
    std::unique_ptr<H> h(new H());
    fill(*h);
    *out = h.release();
  } catch (const std::exception &e) {
    return failed(out || null_out ? &err : nullptr, e, -1);
  }
  return 0;
}

}  // namespace ffe
