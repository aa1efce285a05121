// walk_task.hip - kernels and C ABI of the walk_imitation task layer (ffe_walktask_*, include/flybody_env.h).  The maths lives in
// walk_task.hpp, shared with the host harness of the tests; here: one wavefront (one 64-thread workgroup) per state row, its body
// poses and joint axes in LDS (float32: 3.1 KB, float64: 6.3 KB per wave), the tables in one HBM arena built at create.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>

#include "env_backend.hpp"
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
  void *arena = nullptr;
  std::string err;
};

static thread_local std::string g_werr;

namespace {
int launched(ffe_walktask *h, const char *who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { h->err = std::string(who) + ": " + hipGetErrorString(e); return -2; }
  return 0;
}
}  // namespace

extern "C" {

int ffe_walktask_create(const void *model_blob, size_t blob_size, const ffe_walk_task *task, int flags, int device, ffe_walktask_handle *out) {
  if (!out) { g_werr = "ffe_walktask_create: a null required pointer (out)"; return -1; }
  *out = nullptr;
  auto fail = [&](const std::string &text) { g_werr = "ffe_walktask_create: " + text; return -1; };
  if (flags & ~FFE_WALKTASK_FLOAT64) return fail("unknown flags " + std::to_string(flags));
  std::unique_ptr<ffe_walktask> p(new ffe_walktask());
  p->device = device; p->f64 = (flags & FFE_WALKTASK_FLOAT64) != 0;
  std::string e;
  const bool built = p->f64 ? p->pd.build(model_blob, blob_size, task, e) : p->pf.build(model_blob, blob_size, task, e);
  if (!built) { g_werr = e; return -1; }
  const int nbody = p->f64 ? p->pd.tab.nbody : p->pf.tab.nbody, njnt = p->f64 ? p->pd.tab.njnt : p->pf.tab.njnt;
  if (nbody > wt::kMaxBody || njnt > wt::kMaxJnt)
    return fail("the model has " + std::to_string(nbody) + " bodies and " + std::to_string(njnt) + " joints, above the kernels' capacity of " +
                std::to_string(wt::kMaxBody) + " and " + std::to_string(wt::kMaxJnt));
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return fail("no such HIP device: the MI355X path has no CPU fallback");
  ffe::DeviceGuard guard(device);
  const std::vector<unsigned char> &arena = p->f64 ? p->pd.arena : p->pf.arena;
  if (hipMalloc(&p->arena, arena.size()) != hipSuccess) return fail("out of device memory");
  if (hipMemcpy(p->arena, arena.data(), arena.size(), hipMemcpyHostToDevice) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    (void)hipFree(p->arena);
    return fail("the upload of the tables failed");
  }
  if (p->f64) p->td = p->pd.rebase(p->arena); else p->tf = p->pf.rebase(p->arena);
  *out = p.release();
  return 0;
}

int ffe_walktask_features(ffe_walktask_handle h, const double *qpos_dev, const double *qvel_dev, int n, double *com_dev, void *qvel_out_dev,
                          void *root2site_dev, void *joint_quat_dev, void *stream) {
  if (!h) { g_werr = "ffe_walktask_features: null handle"; return -1; }
  if (!qpos_dev || (qvel_out_dev && !qvel_dev)) { h->err = "ffe_walktask_features: a null required pointer (qpos_dev; qvel_dev when qvel_out_dev is given)"; return -1; }
  if (n < 0) { h->err = "ffe_walktask_features: n " + std::to_string(n) + " is negative"; return -1; }
  if (n == 0) return 0;
  ffe::DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (h->f64)
    hipLaunchKernelGGL(wt::walk_features_kernel<double>, dim3(n), dim3(64), 0, s, h->td, qpos_dev, qvel_dev, com_dev, (double *)qvel_out_dev,
                       (double *)root2site_dev, (double *)joint_quat_dev);
  else
    hipLaunchKernelGGL(wt::walk_features_kernel<float>, dim3(n), dim3(64), 0, s, h->tf, qpos_dev, qvel_dev, com_dev, (float *)qvel_out_dev,
                       (float *)root2site_dev, (float *)joint_quat_dev);
  return launched(h, "ffe_walktask_features");
}

int ffe_walktask_evaluate(ffe_walktask_handle h, const double *qpos_dev, const double *qvel_dev, const int32_t *clip_dev, const int32_t *step_dev,
                          int n, void *factors_dev, void *reward_dev, int32_t *term_bits_dev, void *obs_dev, int obs_stride, void *stream) {
  if (!h) { g_werr = "ffe_walktask_evaluate: null handle"; return -1; }
  const int ntraj = h->f64 ? h->td.ntraj : h->tf.ntraj, obs_dim = h->f64 ? h->td.obs_dim : h->tf.obs_dim;
  if (ntraj <= 0) { h->err = "ffe_walktask_evaluate: the handle was created without reference clips"; return -1; }
  if (!qpos_dev || !qvel_dev || !clip_dev || !step_dev) { h->err = "ffe_walktask_evaluate: a null required pointer (qpos_dev, qvel_dev, clip_dev, step_dev)"; return -1; }
  if (n < 0) { h->err = "ffe_walktask_evaluate: n " + std::to_string(n) + " is negative"; return -1; }
  if (obs_dev && obs_stride < obs_dim) {
    h->err = "ffe_walktask_evaluate: obs_stride " + std::to_string(obs_stride) + " is below the observation row of " + std::to_string(obs_dim);
    return -1;
  }
  if (n == 0) return 0;
  ffe::DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (h->f64)
    hipLaunchKernelGGL(wt::walk_evaluate_kernel<double>, dim3(n), dim3(64), 0, s, h->td, qpos_dev, qvel_dev, clip_dev, step_dev, (double *)factors_dev,
                       (double *)reward_dev, term_bits_dev, (double *)obs_dev, (long long)obs_stride);
  else
    hipLaunchKernelGGL(wt::walk_evaluate_kernel<float>, dim3(n), dim3(64), 0, s, h->tf, qpos_dev, qvel_dev, clip_dev, step_dev, (float *)factors_dev,
                       (float *)reward_dev, term_bits_dev, (float *)obs_dev, (long long)obs_stride);
  return launched(h, "ffe_walktask_evaluate");
}

int ffe_walktask_reference_pose(ffe_walktask_handle h, const int32_t *clip_dev, const int32_t *step_dev, int n, double *qpos_dev, double *qvel_dev,
                                void *stream) {
  if (!h) { g_werr = "ffe_walktask_reference_pose: null handle"; return -1; }
  if ((h->f64 ? h->td.ntraj : h->tf.ntraj) <= 0) { h->err = "ffe_walktask_reference_pose: the handle was created without reference clips"; return -1; }
  if (!clip_dev || !step_dev) { h->err = "ffe_walktask_reference_pose: a null required pointer (clip_dev, step_dev)"; return -1; }
  if (n < 0) { h->err = "ffe_walktask_reference_pose: n " + std::to_string(n) + " is negative"; return -1; }
  if (n == 0) return 0;
  ffe::DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (h->f64)
    hipLaunchKernelGGL(wt::walk_reference_pose_kernel<double>, dim3(n), dim3(64), 0, s, h->td, clip_dev, step_dev, qpos_dev, qvel_dev);
  else
    hipLaunchKernelGGL(wt::walk_reference_pose_kernel<float>, dim3(n), dim3(64), 0, s, h->tf, clip_dev, step_dev, qpos_dev, qvel_dev);
  return launched(h, "ffe_walktask_reference_pose");
}

int ffe_walktask_info(ffe_walktask_handle h, int32_t *dims, int32_t *episode_steps) {
  if (!h) { g_werr = "ffe_walktask_info: null handle"; return -1; }
  if (!dims) { h->err = "ffe_walktask_info: a null required pointer (dims)"; return -1; }
  auto fill = [&](const auto &t, const std::vector<int> &ep) {
    const int v[16] = {t.nq, t.nv, t.J, t.S, t.ntraj, t.future, t.obs_dim, t.off_app, t.off_jpos, t.off_jvel, t.off_disp, t.off_rquat, t.off_zaxis,
                       t.nappend, t.nobsj, h->f64 ? 1 : 0};
    for (int k = 0; k < 16; k++) dims[k] = v[k];
    if (episode_steps)
      for (size_t c = 0; c < ep.size(); c++) episode_steps[c] = ep[c];
  };
  if (h->f64) fill(h->td, h->pd.ep_steps); else fill(h->tf, h->pf.ep_steps);
  return 0;
}

int ffe_walktask_destroy(ffe_walktask_handle h) {
  if (!h) { g_werr = "ffe_walktask_destroy: null handle"; return -1; }
  {
    ffe::DeviceGuard guard(h->device);
    (void)hipFree(h->arena);
  }
  delete h;
  return 0;
}

const char *ffe_walktask_last_error(ffe_walktask_handle h) { return h ? h->err.c_str() : g_werr.c_str(); }

}  // extern "C"
