// replay.hip - uniform minibatches from the n-step writers' replay rings, drawn and gathered on the device: the table the
// reference's learner reads, reverb.Table(sampler=Uniform(), remover=Fifo(), max_size=..., rate_limiter=MinSize(min_replay_size) |
// SampleToInsertRatio(...)) at agents/ray_distributed_dmpo.py:85-113, read in batches of batch_size = 256.  The ring of nstep.hip is
// already the Fifo remover (slot = count mod capacity) and max_size (capacity); this file adds the Uniform sampler (with replacement),
// the MinSize gate and the batching, over one ring or several (one per env group).  Reverb is not in the reference tree or in this
// image: the semantics restate its published behaviour and are checked against a numpy restatement only (parity unpinned).
//
// One ffe_sampler_sample = two launches on the caller's stream, nothing read on the host (graph-capturable):
//   1. sampler_prologue_kernel, one wavefront: N_r = min(written_r, capacity_r) of every ring, their prefix sums, total,
//      ready = total >= min_size and the call key, into a control block; the call counter and samples_drawn live on the device;
//   2. sampler_gather_kernel, one wavefront per sampled row: the draw is wave-uniform and stays in SGPRs (ring, slot, row bases),
//      the lanes move the row  obs[O] | act[A] | ret | disc | next_obs[O] | taint  with coalesced dword accesses, every load of
//      the row issued before its first store (as kBatch in nstep.hip's emit_all).  Not ready: nothing is read from a ring, divided
//      by total or written.
// The draw is exact and counter-based (splitmix64 as in fly_env.hip):
//   key    = splitmix64(splitmix64(seed ^ 0x5A3B1E) + call)        call = number of earlier sample calls on this handle
//   u(k,t) = splitmix64(key + (k << 3) + t)                        k = output row, t = try 0..7
//   g(k,t) = (u(k,t) * total) >> 64                                global row; ring r = the one whose prefix range holds g
// Row k is g(k,0); with FFE_SAMPLE_SKIP_TAINTED the first of the eight tries whose row has taint == 0, the eighth when all are
// tainted (counted in info[3], one atomic per workgroup that has any).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>

#include "../../include/flybody_env.h"
#include "handle.hpp"
#include "nstep_ring.hpp"

namespace ffs {

constexpr int kMaxRings = 8;
constexpr int kRowsPerBlock = 4;  // one wavefront per sampled row
constexpr int kTries = 8;

// one writer's replay ring as the sampler reads it (device memory, written once at creation)
struct Ring {
  const float *obs, *act, *ret, *disc, *next;
  const unsigned char *taint;         // null on an untracked writer
  const unsigned long long *written;  // the writer's running count
  unsigned long long capacity;
};

// what the prologue leaves for the gather of the same call
struct Ctrl {
  unsigned long long key, total;
  unsigned long long prefix[kMaxRings + 1];  // prefix[r] = rows eligible in rings 0 .. r - 1
  int ready;
};

// persistent counters (the prologue is their only writer)
struct State {
  unsigned long long next_call, samples_drawn;
};

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ULL;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
  return x ^ (x >> 31);
}

__global__ __launch_bounds__(64) void sampler_prologue_kernel(const Ring *__restrict__ rings, int n_rings, unsigned long long seed, unsigned long long min_size,
                                                              unsigned long long batch, State *__restrict__ state, Ctrl *__restrict__ ctrl,
                                                              long long *__restrict__ info) {
  const int lane = threadIdx.x;
  unsigned long long n_own = 0;
  if (lane < n_rings) {
    const unsigned long long w = *rings[lane].written, cap = rings[lane].capacity;
    n_own = w < cap ? w : cap;
  }
  // exclusive prefix over the (at most eight) rings, the same in every lane
  unsigned long long before = 0, total = 0;
  for (int r = 0; r < n_rings; r++) {
    const unsigned long long v = __shfl(n_own, r);
    if (r < lane) before += v;
    total += v;
  }
  if (lane <= n_rings) ctrl->prefix[lane] = before;  // (lane n_rings holds the total)
  if (lane == 0) {
    const unsigned long long call = state->next_call;
    const bool ready = total >= min_size;
    unsigned long long drawn = state->samples_drawn;
    if (ready) drawn += batch;
    state->next_call = call + 1;
    state->samples_drawn = drawn;
    ctrl->key = splitmix64(splitmix64(seed ^ 0x5A3B1EULL) + call);
    ctrl->total = total;
    ctrl->ready = ready ? 1 : 0;
    info[0] = ready ? 1 : 0;
    info[1] = (long long)total;
    info[2] = (long long)call;
    info[3] = 0;
    info[4] = (long long)drawn;
    info[5] = info[6] = info[7] = 0;
  }
}

// The ring pointers are read from a table in memory, so the compiler takes them for flat addresses (flat_load_dword, which also
// occupies the LDS counter); they are global: said so here, the loads become global_load_dword off an SGPR base.
typedef const __attribute__((address_space(1))) float *gfloat_p;
typedef const __attribute__((address_space(1))) unsigned char *gbyte_p;

// columns [0, n) of one row, dwords: lane l moves l, l + 64, ...; kChunk loads back to back, then their stores (the pointers may
// alias as far as the compiler knows, so the order written here is the order kept)
constexpr int kChunk = 8;
__device__ __forceinline__ void copy_tail(gfloat_p src, float *dst, int from, int n, int lane) {
  for (int c = from; c < n; c += 64 * kChunk) {
    float v[kChunk];
#pragma unroll
    for (int u = 0; u < kChunk; u++) { const int k = c + u * 64 + lane; v[u] = k < n ? src[k] : 0.f; }
#pragma unroll
    for (int u = 0; u < kChunk; u++) { const int k = c + u * 64 + lane; if (k < n) dst[k] = v[u]; }
  }
}

template <bool SKIP>
__global__ __launch_bounds__(64 * kRowsPerBlock) void sampler_gather_kernel(const Ring *__restrict__ rings, int n_rings, const Ctrl *__restrict__ ctrl, int batch,
                                                                            int O, int A, float *obs_out, float *act_out, float *ret_out, float *disc_out,
                                                                            float *next_out, unsigned char *taint_out, long long *index_out, long long *info) {
  __shared__ int s_kept[kRowsPerBlock];
  if (ctrl->ready == 0) return;  // the whole grid alike: nothing read from a ring, nothing written
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int k = blockIdx.x * kRowsPerBlock + wave;
  int kept = 0;
  if (k < batch) {
    const unsigned long long key = ctrl->key, total = ctrl->total;
    int ring = 0;
    unsigned long long slot = 0;
    for (int t = 0; t < (SKIP ? kTries : 1); t++) {
      const unsigned long long u = splitmix64(key + ((unsigned long long)k << 3) + (unsigned long long)t);
      const unsigned long long g = __umul64hi(u, total);
      // the ring whose range [prefix[r], prefix[r + 1]) holds g: an empty ring has an empty range and is never named
      ring = 0;
      for (int r = 1; r < n_rings; r++) ring += ctrl->prefix[r] <= g ? 1 : 0;
      slot = g - ctrl->prefix[ring];
      if (!SKIP) break;
      const int tainted = __builtin_amdgcn_readfirstlane((int)((gbyte_p)rings[ring].taint)[slot]);
      if (tainted == 0) break;
      if (t == kTries - 1) kept = 1;
    }
    const Ring R = rings[ring];
    const gfloat_p so = (gfloat_p)R.obs + slot * (unsigned long long)O, sn = (gfloat_p)R.next + slot * (unsigned long long)O,
                   sa = (gfloat_p)R.act + slot * (unsigned long long)A;
    float *d_o = obs_out + (size_t)k * O, *d_n = next_out + (size_t)k * O, *d_a = act_out + (size_t)k * A;
    // the row's head - up to 64 * kChunk columns of obs / next_obs, 128 of act, the three scalars: all loads, then all stores.  That is
    // the whole row at every deployed shape (flight 104 / 12, walk_on_ball 289 / 59); wider rows go on chunk by chunk.
    float vo[kChunk], vn[kChunk], va[2];
#pragma unroll
    for (int u = 0; u < kChunk; u++) {
      const int c = u * 64 + lane;
      vo[u] = c < O ? so[c] : 0.f;
      vn[u] = c < O ? sn[c] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 2; u++) { const int c = u * 64 + lane; va[u] = c < A ? sa[c] : 0.f; }
    const float ret = ((gfloat_p)R.ret)[slot], disc = ((gfloat_p)R.disc)[slot];
    unsigned char taint = 0;
    if (taint_out) taint = ((gbyte_p)R.taint)[slot];
#pragma unroll
    for (int u = 0; u < kChunk; u++) {
      const int c = u * 64 + lane;
      if (c < O) { d_o[c] = vo[u]; d_n[c] = vn[u]; }
    }
#pragma unroll
    for (int u = 0; u < 2; u++) { const int c = u * 64 + lane; if (c < A) d_a[c] = va[u]; }
    if (lane == 0) {
      ret_out[k] = ret;
      disc_out[k] = disc;
      if (taint_out) taint_out[k] = taint;
      if (index_out) index_out[k] = (long long)(((unsigned long long)ring << 40) | slot);
    }
    copy_tail(so, d_o, 64 * kChunk, O, lane);
    copy_tail(sn, d_n, 64 * kChunk, O, lane);
    copy_tail(sa, d_a, 128, A, lane);
  }
  if (SKIP) {
    if (lane == 0) s_kept[wave] = kept;
    __syncthreads();
    if (threadIdx.x == 0) {
      int sum = 0;
      for (int w = 0; w < kRowsPerBlock; w++) sum += s_kept[w];
      if (sum > 0) atomicAdd((unsigned long long *)&info[3], (unsigned long long)sum);
    }
  }
}

}  // namespace ffs

struct ffe_sampler {
  int device = 0, n_rings = 0, batch = 0, obs_dim = 0, act_dim = 0, flags = 0;
  bool tracked = false;  // every writer keeps a taint column
  unsigned long long seed = 0, min_size = 1;
  ffs::Ring *rings = nullptr;
  ffs::Ctrl *ctrl = nullptr;
  ffs::State *state = nullptr;
  long long *info = nullptr;
  ffe::DeviceBuffers mem{"ffe_sampler_create"};
  std::string err;
};

static thread_local std::string g_serr;  // of ffe_sampler_create and of calls on a NULL handle

using ffe::need;

extern "C" {

int ffe_sampler_create(const ffe_nstep_handle *writers, int n_writers, int batch, uint64_t seed, long long min_size, int flags, int device,
                       ffe_sampler_handle *out) {
  return ffe::create(out, "ffe_sampler_create: null out", g_serr, [&](ffe_sampler &s) {
    auto must = [](bool ok, const std::string &text) { if (!ok) throw ffe::Refused("ffe_sampler_create: " + text); };
    must(writers, "null writers");
    must(n_writers >= 1 && n_writers <= ffs::kMaxRings, "n_writers " + std::to_string(n_writers) + " is outside 1 .. 8");
    must(batch >= 1 && batch <= (1 << 20), "batch " + std::to_string(batch) + " is outside 1 .. 2^20");
    must(min_size >= 1, "min_size " + std::to_string(min_size) + " is below 1");
    must(!(flags & ~FFE_SAMPLE_SKIP_TAINTED), "unknown flags " + std::to_string(flags));
    ffs::Ring host[ffs::kMaxRings] = {};
    bool tracked = true;
    for (int r = 0; r < n_writers; r++) {
      must(writers[r], "writer " + std::to_string(r) + " is null");
      const ffn::Handle &W = writers[r]->h;
      const ffn::Dev &D = W.d, &D0 = writers[0]->h.d;
      must(W.device == device, "writer " + std::to_string(r) + " is on device " + std::to_string(W.device) + ", the sampler on " + std::to_string(device));
      must(D.obs_dim == D0.obs_dim && D.act_dim == D0.act_dim,
           "writer " + std::to_string(r) + " has rows of (" + std::to_string(D.obs_dim) + ", " + std::to_string(D.act_dim) + "), writer 0 of (" +
               std::to_string(D0.obs_dim) + ", " + std::to_string(D0.act_dim) + "): obs_dim and act_dim must be equal");
      must(D.capacity < (1LL << 40), "writer " + std::to_string(r) + " has a capacity of 2^40 or more: index packs the slot into 40 bits");
      tracked = tracked && D.t_taint != nullptr;
      host[r] = ffs::Ring{D.t_obs, D.t_act, D.t_ret, D.t_disc, D.t_next, D.t_taint, D.written, (unsigned long long)D.capacity};
    }
    must(!(flags & FFE_SAMPLE_SKIP_TAINTED) || tracked, "FFE_SAMPLE_SKIP_TAINTED needs every writer created with validity tracking (ffe_nstep_create_tracked)");
    ffe::check_device(device, "ffe_sampler_create", true);
    ffe::DeviceGuard guard(device);
    s.device = device; s.n_rings = n_writers; s.batch = batch; s.flags = flags; s.tracked = tracked;
    s.obs_dim = writers[0]->h.d.obs_dim; s.act_dim = writers[0]->h.d.act_dim;
    s.seed = seed; s.min_size = (unsigned long long)min_size;
    s.rings = s.mem.zeroed<ffs::Ring>(ffs::kMaxRings); s.ctrl = s.mem.zeroed<ffs::Ctrl>(1);
    s.state = s.mem.zeroed<ffs::State>(1); s.info = s.mem.zeroed<long long>(8);
    must(hipMemcpy(s.rings, host, sizeof(host), hipMemcpyHostToDevice) == hipSuccess, "out of device memory");
    s.mem.ready();
  });
}

int ffe_sampler_sample(ffe_sampler_handle s, float *obs_dev, float *act_dev, float *ret_dev, float *disc_dev, float *next_obs_dev, uint8_t *taint_dev,
                       int64_t *index_dev, void *stream) {
  const char *who = "ffe_sampler_sample";
  return ffe::on_handle(s, who, &g_serr, [&](ffe_sampler &S) {
    need(obs_dev && act_dev && ret_dev && disc_dev && next_obs_dev, "ffe_sampler_sample: a null output (only taint_dev and index_dev may be NULL)");
    need(!taint_dev || S.tracked, "ffe_sampler_sample: taint_dev needs every writer created with validity tracking (ffe_nstep_create_tracked)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(ffs::sampler_prologue_kernel, dim3(1), dim3(64), 0, st, S.rings, S.n_rings, S.seed, S.min_size, (unsigned long long)S.batch, S.state,
                       S.ctrl, S.info);
    ffe::launched(who);
    const dim3 grid((S.batch + ffs::kRowsPerBlock - 1) / ffs::kRowsPerBlock), block(64 * ffs::kRowsPerBlock);
    long long *index = reinterpret_cast<long long *>(index_dev);
    if (S.flags & FFE_SAMPLE_SKIP_TAINTED)
      hipLaunchKernelGGL(ffs::sampler_gather_kernel<true>, grid, block, 0, st, S.rings, S.n_rings, S.ctrl, S.batch, S.obs_dim, S.act_dim, obs_dev, act_dev,
                         ret_dev, disc_dev, next_obs_dev, taint_dev, index, S.info);
    else
      hipLaunchKernelGGL(ffs::sampler_gather_kernel<false>, grid, block, 0, st, S.rings, S.n_rings, S.ctrl, S.batch, S.obs_dim, S.act_dim, obs_dev, act_dev,
                         ret_dev, disc_dev, next_obs_dev, taint_dev, index, S.info);
    ffe::launched(who);
  });
}

int ffe_sampler_info(ffe_sampler_handle s, long long **info_dev) {
  return ffe::on_handle(s, "ffe_sampler_info", &g_serr, [&](ffe_sampler &S) {
    need(info_dev, "ffe_sampler_info: null info_dev");
    *info_dev = S.info;
  });
}

int ffe_sampler_destroy(ffe_sampler_handle s) { return ffe::destroy(s, "ffe_sampler_destroy", &g_serr); }

const char *ffe_sampler_last_error(ffe_sampler_handle s) { return s ? s->err.c_str() : g_serr.c_str(); }

}  // extern "C"
