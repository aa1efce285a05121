// walk_task.hip - kernels and C ABI of the walk_imitation task layer (ffe_walktask_*, include/flybody_env.h).  The maths lives in
// walk_task.hpp, shared with the host harness of the tests; here: one wavefront (one 64-thread workgroup) per state row, its body
// poses and joint axes in LDS (float32: 3.1 KB, float64: 6.3 KB per wave), the tables in one HBM arena built at create.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>

#include "../../include/flybody_env.h"
#include "handle.hpp"
#include "walk_task.hpp"

namespace wt {

constexpr int kMaxBody = 72, kMaxJnt = 104;  // LDS capacity (walk model: 68 bodies, 103 joints); create refuses larger models

template <class T>
__global__ __launch_bounds__(64) void walk_features_kernel(const Tables<T> t, const double *__restrict__ qpos, const double *__restrict__ qvel,
                                                           double *__restrict__ com, T *__restrict__ qv, T *__restrict__ r2s, T *__restrict__ jq) {
  __shared__ T P[7 * kMaxBody], AX[3 * kMaxJnt];
  const size_t n = blockIdx.x;
  RowOut<T> o;
  o.com = com ? com + 3 * n : nullptr;
  o.qvel = qv ? qv + n * (6 + t.J) : nullptr;
  o.r2s = r2s ? r2s + n * 3 * t.S : nullptr;
  o.jq = jq ? jq + n * 4 * (1 + t.J) : nullptr;
  o.factors = nullptr; o.reward = nullptr; o.term = nullptr; o.obs = nullptr;
  row_task<T, false>(t, qpos + n * t.nq, qvel ? qvel + n * t.nv : nullptr, 0, 0, o, P, AX);
}

template <class T>
__global__ __launch_bounds__(64) void walk_evaluate_kernel(const Tables<T> t, const double *__restrict__ qpos, const double *__restrict__ qvel,
                                                           const int *__restrict__ clip, const int *__restrict__ step, T *__restrict__ factors,
                                                           T *__restrict__ reward, int *__restrict__ term, T *__restrict__ obs, long long obs_stride) {
  __shared__ T P[7 * kMaxBody], AX[3 * kMaxJnt];
  const size_t n = blockIdx.x;
  RowOut<T> o;
  o.com = nullptr; o.qvel = nullptr; o.r2s = nullptr; o.jq = nullptr;
  o.factors = factors ? factors + 4 * n : nullptr;
  o.reward = reward ? reward + n : nullptr;
  o.term = term ? term + n : nullptr;
  o.obs = obs ? obs + n * (size_t)obs_stride : nullptr;
  row_task<T, true>(t, qpos + n * t.nq, qvel + n * t.nv, clip[n], step[n], o, P, AX);
}

template <class T>
__global__ __launch_bounds__(64) void walk_reference_pose_kernel(const Tables<T> t, const int *__restrict__ clip, const int *__restrict__ step,
                                                                 double *__restrict__ qpos, double *__restrict__ qvel) {
  const size_t n = blockIdx.x;
  row_reference_pose<T>(t, clip[n], step[n], qpos ? qpos + n * t.nq : nullptr, qvel ? qvel + n * t.nv : nullptr);
}

}  // namespace wt

struct ffe_walktask {
  int device = 0;
  bool f64 = false;
  wt::Packed<float> pf;
  wt::Packed<double> pd;
  wt::Tables<float> tf;
  wt::Tables<double> td;
  ffe::DeviceBuffers mem{"ffe_walktask_create"};  // the arena
  std::string err;
};

static thread_local std::string g_werr;  // of ffe_walktask_create and of calls on a NULL handle

using ffe::need;
using ffe::Refused;

extern "C" {

int ffe_walktask_create(const void *model_blob, size_t blob_size, const ffe_walk_task *task, int flags, int device, ffe_walktask_handle *out) {
  return ffe::create(out, "ffe_walktask_create: a null required pointer (out)", g_werr, [&](ffe_walktask &p) {
    auto must = [](bool ok, const std::string &text) { if (!ok) throw Refused("ffe_walktask_create: " + text); };
    must(!(flags & ~FFE_WALKTASK_FLOAT64), "unknown flags " + std::to_string(flags));
    p.device = device; p.f64 = (flags & FFE_WALKTASK_FLOAT64) != 0;
    std::string e;
    if (!(p.f64 ? p.pd.build(model_blob, blob_size, task, e) : p.pf.build(model_blob, blob_size, task, e))) throw Refused(e);
    const int nbody = p.f64 ? p.pd.tab.nbody : p.pf.tab.nbody, njnt = p.f64 ? p.pd.tab.njnt : p.pf.tab.njnt;
    must(nbody <= wt::kMaxBody && njnt <= wt::kMaxJnt, "the model has " + std::to_string(nbody) + " bodies and " + std::to_string(njnt) +
                                                           " joints, above the kernels' capacity of " + std::to_string(wt::kMaxBody) + " and " + std::to_string(wt::kMaxJnt));
    ffe::check_device(device, "ffe_walktask_create", true);
    ffe::DeviceGuard guard(device);
    const std::vector<unsigned char> &arena = p.f64 ? p.pd.arena : p.pf.arena;
    unsigned char *dev = p.mem.zeroed<unsigned char>(arena.size());
    must(hipMemcpy(dev, arena.data(), arena.size(), hipMemcpyHostToDevice) == hipSuccess && hipDeviceSynchronize() == hipSuccess, "the upload of the tables failed");
    if (p.f64) p.td = p.pd.rebase(dev); else p.tf = p.pf.rebase(dev);
  });
}

int ffe_walktask_features(ffe_walktask_handle h, const double *qpos_dev, const double *qvel_dev, int n, double *com_dev, void *qvel_out_dev,
                          void *root2site_dev, void *joint_quat_dev, void *stream) {
  return ffe::on_handle(h, "ffe_walktask_features", &g_werr, [&](ffe_walktask &p) {
    need(qpos_dev && (!qvel_out_dev || qvel_dev), "ffe_walktask_features: a null required pointer (qpos_dev; qvel_dev when qvel_out_dev is given)");
    if (n < 0) throw Refused("ffe_walktask_features: n " + std::to_string(n) + " is negative");
    if (n == 0) return;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (p.f64)
      hipLaunchKernelGGL(wt::walk_features_kernel<double>, dim3(n), dim3(64), 0, s, p.td, qpos_dev, qvel_dev, com_dev, (double *)qvel_out_dev,
                         (double *)root2site_dev, (double *)joint_quat_dev);
    else
      hipLaunchKernelGGL(wt::walk_features_kernel<float>, dim3(n), dim3(64), 0, s, p.tf, qpos_dev, qvel_dev, com_dev, (float *)qvel_out_dev,
                         (float *)root2site_dev, (float *)joint_quat_dev);
    ffe::launched("ffe_walktask_features");
  });
}

int ffe_walktask_evaluate(ffe_walktask_handle h, const double *qpos_dev, const double *qvel_dev, const int32_t *clip_dev, const int32_t *step_dev,
                          int n, void *factors_dev, void *reward_dev, int32_t *term_bits_dev, void *obs_dev, int obs_stride, void *stream) {
  return ffe::on_handle(h, "ffe_walktask_evaluate", &g_werr, [&](ffe_walktask &p) {
    const int ntraj = p.f64 ? p.td.ntraj : p.tf.ntraj, obs_dim = p.f64 ? p.td.obs_dim : p.tf.obs_dim;
    need(ntraj > 0, "ffe_walktask_evaluate: the handle was created without reference clips");
    need(qpos_dev && qvel_dev && clip_dev && step_dev, "ffe_walktask_evaluate: a null required pointer (qpos_dev, qvel_dev, clip_dev, step_dev)");
    if (n < 0) throw Refused("ffe_walktask_evaluate: n " + std::to_string(n) + " is negative");
    if (obs_dev && obs_stride < obs_dim)
      throw Refused("ffe_walktask_evaluate: obs_stride " + std::to_string(obs_stride) + " is below the observation row of " + std::to_string(obs_dim));
    if (n == 0) return;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (p.f64)
      hipLaunchKernelGGL(wt::walk_evaluate_kernel<double>, dim3(n), dim3(64), 0, s, p.td, qpos_dev, qvel_dev, clip_dev, step_dev, (double *)factors_dev,
                         (double *)reward_dev, term_bits_dev, (double *)obs_dev, (long long)obs_stride);
    else
      hipLaunchKernelGGL(wt::walk_evaluate_kernel<float>, dim3(n), dim3(64), 0, s, p.tf, qpos_dev, qvel_dev, clip_dev, step_dev, (float *)factors_dev,
                         (float *)reward_dev, term_bits_dev, (float *)obs_dev, (long long)obs_stride);
    ffe::launched("ffe_walktask_evaluate");
  });
}

int ffe_walktask_reference_pose(ffe_walktask_handle h, const int32_t *clip_dev, const int32_t *step_dev, int n, double *qpos_dev, double *qvel_dev,
                                void *stream) {
  return ffe::on_handle(h, "ffe_walktask_reference_pose", &g_werr, [&](ffe_walktask &p) {
    need((p.f64 ? p.td.ntraj : p.tf.ntraj) > 0, "ffe_walktask_reference_pose: the handle was created without reference clips");
    need(clip_dev && step_dev, "ffe_walktask_reference_pose: a null required pointer (clip_dev, step_dev)");
    if (n < 0) throw Refused("ffe_walktask_reference_pose: n " + std::to_string(n) + " is negative");
    if (n == 0) return;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (p.f64)
      hipLaunchKernelGGL(wt::walk_reference_pose_kernel<double>, dim3(n), dim3(64), 0, s, p.td, clip_dev, step_dev, qpos_dev, qvel_dev);
    else
      hipLaunchKernelGGL(wt::walk_reference_pose_kernel<float>, dim3(n), dim3(64), 0, s, p.tf, clip_dev, step_dev, qpos_dev, qvel_dev);
    ffe::launched("ffe_walktask_reference_pose");
  });
}

int ffe_walktask_info(ffe_walktask_handle h, int32_t *dims, int32_t *episode_steps) {
  return ffe::on_handle(h, "ffe_walktask_info", &g_werr, [&](ffe_walktask &p) {
    need(dims, "ffe_walktask_info: a null required pointer (dims)");
    auto fill = [&](const auto &t, const std::vector<int> &ep) {
      const int v[16] = {t.nq, t.nv, t.J, t.S, t.ntraj, t.future, t.obs_dim, t.off_app, t.off_jpos, t.off_jvel, t.off_disp, t.off_rquat, t.off_zaxis,
                         t.nappend, t.nobsj, p.f64 ? 1 : 0};
      for (int k = 0; k < 16; k++) dims[k] = v[k];
      if (episode_steps)
        for (size_t c = 0; c < ep.size(); c++) episode_steps[c] = ep[c];
    };
    if (p.f64) fill(p.td, p.pd.ep_steps); else fill(p.tf, p.pf.ep_steps);
  });
}

int ffe_walktask_destroy(ffe_walktask_handle h) { return ffe::destroy(h, "ffe_walktask_destroy", &g_werr); }

const char *ffe_walktask_last_error(ffe_walktask_handle h) { return h ? h->err.c_str() : g_werr.c_str(); }

}  // extern "C"
