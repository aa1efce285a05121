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

#include "../../include/flybody_env.h"
#include "handle.hpp"

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
  ffe::DeviceBuffers mem{"ffe_eplog_create"};
  std::string err;
};

static thread_local std::string g_lerr;  // of ffe_eplog_create and of calls on a NULL handle

using ffe::need;
using ffe::Refused;

extern "C" {

int ffe_eplog_create(int batch, long long capacity, int flags, int device, ffe_eplog_handle *out) {
  return ffe::create(out, "ffe_eplog_create: null out", g_lerr, [&](ffe_eplog &p) {
    auto must = [](bool ok, const std::string &text) { if (!ok) throw Refused("ffe_eplog_create: " + text); };
    must(batch > 0, "batch " + std::to_string(batch) + " is below 1");
    must(!(flags & ~FFE_EPLOG_ONE_SHOT), "unknown flags " + std::to_string(flags));
    // one call can emit a record for every env; in a smaller ring two records of the same launch would share a slot
    must(capacity >= batch,
         "capacity " + std::to_string(capacity) + " is below batch = " + std::to_string(batch) + ", the records one call can write: they would share slots of the ring");
    ffe::check_device(device, "ffe_eplog_create", true);
    ffe::DeviceGuard guard(device);
    p.device = device; p.batch = batch; p.flags = flags; p.capacity = capacity;
    const size_t B = (size_t)batch;
    p.ep_ret = p.mem.zeroed<float>(B); p.ep_len = p.mem.zeroed<int>(B); p.armed = p.mem.zeroed<unsigned char>(B);
    p.records = p.mem.zeroed<ffl::Record>((size_t)capacity); p.info = p.mem.zeroed<unsigned long long>(4); p.ticket = p.mem.zeroed<unsigned int>(1);
    p.mem.ready();
  });
}

int ffe_eplog_arm(ffe_eplog_handle h, const uint8_t *mask_dev, void *stream) {
  return ffe::on_handle(h, "ffe_eplog_arm", &g_lerr, [&](ffe_eplog &p) {
    need(p.flags & FFE_EPLOG_ONE_SHOT, "ffe_eplog_arm: the log was not created one-shot (FFE_EPLOG_ONE_SHOT): a plain log records every episode");
    hipLaunchKernelGGL(ffl::episode_log_arm_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), mask_dev, p.armed, p.info, p.batch);
    ffe::launched("ffe_eplog_arm");
  });
}

int ffe_eplog_observe(ffe_eplog_handle h, const int32_t *step_type_dev, const float *reward_dev, const float *discount_dev, const int32_t *info_dev,
                      const int32_t *tag_dev, int tag_stride_ints, void *stream) {
  return ffe::on_handle(h, "ffe_eplog_observe", &g_lerr, [&](ffe_eplog &p) {
    need(step_type_dev && reward_dev && discount_dev, "ffe_eplog_observe: a null input (only info_dev and tag_dev may be NULL)");
    if (tag_dev && tag_stride_ints < 1) throw Refused("ffe_eplog_observe: tag_stride_ints " + std::to_string(tag_stride_ints) + " is below 1");
    const dim3 grid((p.batch + 255) / 256), block(256);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (p.flags & FFE_EPLOG_ONE_SHOT)
      hipLaunchKernelGGL(ffl::episode_log_kernel<true>, grid, block, 0, s, step_type_dev, reward_dev, discount_dev, info_dev, tag_dev, (long long)tag_stride_ints, p.ep_ret,
                         p.ep_len, p.armed, p.records, (unsigned long long)p.capacity, p.info, p.ticket, p.batch);
    else
      hipLaunchKernelGGL(ffl::episode_log_kernel<false>, grid, block, 0, s, step_type_dev, reward_dev, discount_dev, info_dev, tag_dev, (long long)tag_stride_ints, p.ep_ret,
                         p.ep_len, p.armed, p.records, (unsigned long long)p.capacity, p.info, p.ticket, p.batch);
    ffe::launched("ffe_eplog_observe");
  });
}

int ffe_eplog_buffers(ffe_eplog_handle h, void **records_dev, long long **info_dev) {
  return ffe::on_handle(h, "ffe_eplog_buffers", &g_lerr, [&](ffe_eplog &p) {
    need(records_dev && info_dev, "ffe_eplog_buffers: a null output pointer");
    *records_dev = p.records;
    *info_dev = reinterpret_cast<long long *>(p.info);
  });
}

int ffe_eplog_destroy(ffe_eplog_handle h) { return ffe::destroy(h, "ffe_eplog_destroy", &g_lerr); }

const char *ffe_eplog_last_error(ffe_eplog_handle h) { return h ? h->err.c_str() : g_lerr.c_str(); }

}  // extern "C"
