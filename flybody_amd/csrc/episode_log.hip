// episode_log.hip - one record per finished episode, kept on the device: what the reference's EnvironmentLoop hands to its logger
// after every episode (agents/ray_distributed_dmpo.py:401-440: episode_length, episode_return) and what its evaluator aggregates
// over the last eval_average_over of them (_eval_agg_stat, :417-440), for B envs per call.  ffe_episode_stats (nstep.hip) folds a
// finished episode into two totals; this keeps it: which env, which tag (flight imitation: the reference clip), how long, its
// return, the call that closed it, how many of its steps ran truncated physics and whether it terminated or hit the time limit.
// acme's loop is not in the reference tree: the per-episode rule restates it and is checked against a numpy restatement only.
//
// One ffe_eplog_observe = one launch on the caller's stream, nothing read on the host (graph-capturable).  One lane per env:
//   FIRST  restarts the env's running return and length, adds nothing (an episode abandoned by a reset leaves no record)
//   MID    ret += reward (float32, step order, as episode_stats_kernel), length += 1
//   LAST   the same, then the record is written and the counters restart
// LAST rows are rare, so slots are claimed per wavefront: ballot of the emitting lanes, one 64-bit atomic add of the popcount on
// `count` by the first of them, the base broadcast, lane's slot = (base + its rank among the set bits) mod capacity.  A call's
// records therefore occupy one contiguous range of `count`, in no particular order inside it.  A record is two 16-byte stores.
// The call index lives on the device (info[1]): every workgroup reads it on entry; the workgroup that draws the last ticket of the
// launch - by then every other one has read it - stores call + 1 and returns the ticket counter to zero.
// One-shot logs (FFE_EPLOG_ONE_SHOT): only armed envs emit; an env disarms on its LAST and armed_left goes down by the same popcount.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>

#include "env_backend.hpp"

namespace ffl {

struct alignas(32) Record {
  int env, tag, length;
  float ret;
  long long call;
  int flagged_steps, bits;
};
static_assert(sizeof(Record) == 32, "a record is 32 bytes");

// info block: {records written, calls, armed_left, reserved}
enum { kWritten = 0, kCalls = 1, kArmedLeft = 2 };

template <bool ONE_SHOT>
__global__ __launch_bounds__(256) void episode_log_kernel(const int *__restrict__ st, const float *__restrict__ rew, const float *__restrict__ disc,
                                                          const int *__restrict__ info_in, const int *__restrict__ tag_in, long long tag_stride,
                                                          float *__restrict__ ep_ret, int *__restrict__ ep_len, unsigned char *__restrict__ armed,
                                                          Record *__restrict__ records, unsigned long long capacity, unsigned long long *info,
                                                          unsigned int *ticket, int batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  // the call index, read by every wavefront before its workgroup can draw a ticket: readfirstlane needs the loaded value, so the load
  // has completed before the barrier below
  const unsigned long long call_v = info[kCalls];
  const unsigned long long call = ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned int)(call_v >> 32)) << 32) |
                                  (unsigned int)__builtin_amdgcn_readfirstlane((unsigned int)call_v);
  bool emit = false;
  float r = 0.f;
  int l = 0;
  if (i < batch) {
    const int s = st[i];
    r = ep_ret[i];
    l = ep_len[i];
    if (s == FFE_STEP_FIRST) { r = 0.f; l = 0; }
    else { r += rew[i]; l += 1; }
    if (s == FFE_STEP_LAST) {
      emit = true;
      if (ONE_SHOT) {
        emit = armed[i] != 0;
        if (emit) armed[i] = 0;
      }
      ep_ret[i] = 0.f; ep_len[i] = 0;
    } else {
      ep_ret[i] = r; ep_len[i] = l;
    }
  }
  const unsigned long long mask = __ballot(emit);
  if (mask != 0) {  // wave-uniform
    const int leader = __ffsll((long long)mask) - 1;
    const unsigned long long n = (unsigned long long)__popcll(mask);
    unsigned long long base = 0;
    if (lane == leader) {
      base = atomicAdd(&info[kWritten], n);
      if (ONE_SHOT) atomicAdd(&info[kArmedLeft], 0ULL - n);
    }
    base = __shfl(base, leader);
    if (emit) {
      const unsigned long long rank = (unsigned long long)__popcll(mask & ((1ULL << lane) - 1ULL));
      const unsigned long long slot = (base + rank) % capacity;
      int flagged = 0, bits = 0;
      if (info_in) { flagged = info_in[4 * (long long)i + 1]; bits = info_in[4 * (long long)i + 2] & 255; }
      if (disc[i] == 0.f) bits |= 256;
      const int tag = tag_in ? tag_in[(long long)i * tag_stride] : 0;
      int4 *dst = reinterpret_cast<int4 *>(records + slot);
      dst[0] = make_int4(i, tag, l, __float_as_int(r));
      dst[1] = make_int4((int)(unsigned int)call, (int)(unsigned int)(call >> 32), flagged, bits);
    }
  }
  // the call counter: the last workgroup of the launch to get here advances it
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    if (atomicAdd(ticket, 1u) == gridDim.x - 1) {
      __threadfence();
      *ticket = 0;
      info[kCalls] = call + 1;
    }
  }
}

// one workgroup: armed[i] = mask[i] != 0 (or 1), armed_left = their number.  Arming is rare and B a few thousand.
__global__ __launch_bounds__(256) void episode_log_arm_kernel(const unsigned char *__restrict__ mask, unsigned char *__restrict__ armed,
                                                              unsigned long long *__restrict__ info, int batch) {
  __shared__ int s_n[4];
  int n = 0;
  for (int i = threadIdx.x; i < batch; i += 256) {
    const unsigned char a = mask ? (mask[i] != 0 ? 1 : 0) : 1;
    armed[i] = a;
    n += a;
  }
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
  if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) info[kArmedLeft] = (unsigned long long)(s_n[0] + s_n[1] + s_n[2] + s_n[3]);
}

}  // namespace ffl

struct ffe_eplog {
  int device = 0, batch = 0, flags = 0;
  long long capacity = 0;
  float *ep_ret = nullptr;
  int *ep_len = nullptr;
  unsigned char *armed = nullptr;
  ffl::Record *records = nullptr;
  unsigned long long *info = nullptr;  // [4]
  unsigned int *ticket = nullptr;
  std::string err;
};

static thread_local std::string g_lerr;

namespace {
void free_all(ffe_eplog *p) {
  (void)hipFree(p->ep_ret); (void)hipFree(p->ep_len); (void)hipFree(p->armed); (void)hipFree(p->records); (void)hipFree(p->info); (void)hipFree(p->ticket);
}
}  // namespace

extern "C" {

int ffe_eplog_create(int batch, long long capacity, int flags, int device, ffe_eplog_handle *out) {
  if (!out) { g_lerr = "ffe_eplog_create: null out"; return -1; }
  *out = nullptr;
  auto fail = [&](const std::string &text) { g_lerr = "ffe_eplog_create: " + text; return -1; };
  if (batch <= 0) return fail("batch " + std::to_string(batch) + " is below 1");
  if (flags & ~FFE_EPLOG_ONE_SHOT) return fail("unknown flags " + std::to_string(flags));
  // one call can emit a record for every env; in a smaller ring two records of the same launch would share a slot
  if (capacity < batch)
    return fail("capacity " + std::to_string(capacity) + " is below batch = " + std::to_string(batch) + ", the records one call can write: they would share slots of the ring");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return fail("no such HIP device: the MI355X path has no CPU fallback");
  ffe::DeviceGuard guard(device);
  std::unique_ptr<ffe_eplog> p(new ffe_eplog());
  p->device = device; p->batch = batch; p->flags = flags; p->capacity = capacity;
  const size_t B = (size_t)batch;
  bool ok = hipMalloc((void **)&p->ep_ret, B * sizeof(float)) == hipSuccess && hipMalloc((void **)&p->ep_len, B * sizeof(int)) == hipSuccess &&
            hipMalloc((void **)&p->armed, B) == hipSuccess && hipMalloc((void **)&p->records, (size_t)capacity * sizeof(ffl::Record)) == hipSuccess &&
            hipMalloc((void **)&p->info, 4 * sizeof(unsigned long long)) == hipSuccess && hipMalloc((void **)&p->ticket, sizeof(unsigned int)) == hipSuccess;
  if (ok)
    ok = hipMemset(p->ep_ret, 0, B * sizeof(float)) == hipSuccess && hipMemset(p->ep_len, 0, B * sizeof(int)) == hipSuccess &&
         hipMemset(p->armed, 0, B) == hipSuccess && hipMemset(p->records, 0, (size_t)capacity * sizeof(ffl::Record)) == hipSuccess &&
         hipMemset(p->info, 0, 4 * sizeof(unsigned long long)) == hipSuccess && hipMemset(p->ticket, 0, sizeof(unsigned int)) == hipSuccess &&
         hipDeviceSynchronize() == hipSuccess;
  if (!ok) { free_all(p.get()); return fail("out of device memory"); }
  *out = p.release();
  return 0;
}

int ffe_eplog_arm(ffe_eplog_handle h, const uint8_t *mask_dev, void *stream) {
  if (!h) { g_lerr = "ffe_eplog_arm: null handle"; return -1; }
  if (!(h->flags & FFE_EPLOG_ONE_SHOT)) { h->err = "ffe_eplog_arm: the log was not created one-shot (FFE_EPLOG_ONE_SHOT): a plain log records every episode"; return -1; }
  ffe::DeviceGuard guard(h->device);
  hipLaunchKernelGGL(ffl::episode_log_arm_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), mask_dev, h->armed, h->info, h->batch);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { h->err = std::string("ffe_eplog_arm: ") + hipGetErrorString(e); return -2; }
  return 0;
}

int ffe_eplog_observe(ffe_eplog_handle h, const int32_t *step_type_dev, const float *reward_dev, const float *discount_dev, const int32_t *info_dev,
                      const int32_t *tag_dev, int tag_stride_ints, void *stream) {
  if (!h) { g_lerr = "ffe_eplog_observe: null handle"; return -1; }
  if (!step_type_dev || !reward_dev || !discount_dev) { h->err = "ffe_eplog_observe: a null input (only info_dev and tag_dev may be NULL)"; return -1; }
  if (tag_dev && tag_stride_ints < 1) { h->err = "ffe_eplog_observe: tag_stride_ints " + std::to_string(tag_stride_ints) + " is below 1"; return -1; }
  ffe::DeviceGuard guard(h->device);
  const dim3 grid((h->batch + 255) / 256), block(256);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (h->flags & FFE_EPLOG_ONE_SHOT)
    hipLaunchKernelGGL(ffl::episode_log_kernel<true>, grid, block, 0, s, step_type_dev, reward_dev, discount_dev, info_dev, tag_dev, (long long)tag_stride_ints, h->ep_ret,
                       h->ep_len, h->armed, h->records, (unsigned long long)h->capacity, h->info, h->ticket, h->batch);
  else
    hipLaunchKernelGGL(ffl::episode_log_kernel<false>, grid, block, 0, s, step_type_dev, reward_dev, discount_dev, info_dev, tag_dev, (long long)tag_stride_ints, h->ep_ret,
                       h->ep_len, h->armed, h->records, (unsigned long long)h->capacity, h->info, h->ticket, h->batch);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { h->err = std::string("ffe_eplog_observe: ") + hipGetErrorString(e); return -2; }
  return 0;
}

int ffe_eplog_buffers(ffe_eplog_handle h, void **records_dev, long long **info_dev) {
  if (!h) { g_lerr = "ffe_eplog_buffers: null handle"; return -1; }
  if (!records_dev || !info_dev) { h->err = "ffe_eplog_buffers: a null output pointer"; return -1; }
  *records_dev = h->records;
  *info_dev = reinterpret_cast<long long *>(h->info);
  return 0;
}

int ffe_eplog_destroy(ffe_eplog_handle h) {
  if (!h) { g_lerr = "ffe_eplog_destroy: null handle"; return -1; }
  {
    ffe::DeviceGuard guard(h->device);
    free_all(h);
  }
  delete h;
  return 0;
}

const char *ffe_eplog_last_error(ffe_eplog_handle h) { return h ? h->err.c_str() : g_lerr.c_str(); }

}  // extern "C"
