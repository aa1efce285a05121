// nstep_ring.hpp - the n-step writer's device record and handle, shared by the writer (nstep.hip) and the replay sampler that
// reads its ring (replay.hip).  Nothing else may look inside an ffe_nstep_handle.
#pragma once

#include <string>

#include "handle.hpp"

namespace ffn {

struct Dev {
  int batch, obs_dim, act_dim, n_step;
  float gamma;
  long long capacity;
  // per-env rings
  float *r_obs, *r_act, *r_rew, *r_disc;  // [B][n][O], [B][n][A], [B][n], [B][n]
  float *last_obs;                        // [B][O] observation the next action will be taken from
  int *head, *count;                      // ring write position / entries held
  // replay ring
  float *t_obs, *t_act, *t_ret, *t_disc, *t_next;
  unsigned long long *written;            // transitions written so far (monotone)
  // validity tracking (null on a writer created without it)
  unsigned char *r_mark;                  // [B][n] mark e of each held entry
  int *prev_bits;                         // [B] step_bits passed with the previous call
  unsigned char *t_taint;                 // [capacity] taint of each replay slot
};

struct Handle {
  Dev d{};
  int device = 0;
  ffe::DeviceBuffers mem{"ffe_nstep_create"};
  std::string err;
};

}  // namespace ffn

struct ffe_nstep {
  ffn::Handle h;
};
