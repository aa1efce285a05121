// Stand-alone host program around the two table builders (ball_model.hpp, walk_model.hpp) for tests/test_walk_physics_cpu.py:
//   walk_model_host <fly_walk.ffmb> <fly_ball.ffmb>
// builds the device tables from both blobs, checks that the walk builder's link / dof / block / schedule / actuator tables are the ball
// builder's (the hinge order of the two models is the same), and prints `key value` lines.  Built with -fsanitize=address,undefined.
#define CVX_HOST 1  // convex.hpp (pulled in by dev_model.hpp) without the HIP runtime
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

struct float4 { float x, y, z, w; };  // the one HIP vector type dev_model.hpp names (flight tables, unused here)

#include "../flybody_amd/csrc/walk_model.hpp"

static std::vector<char> slurp(const char *path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw std::runtime_error(std::string("cannot open ") + path);
  return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

// FNV-1a over a table: a cheap fingerprint that changes when the ball builder's output does
static unsigned long long fnv(const void *p, size_t n) {
  unsigned long long h = 1469598103934665603ull;
  for (size_t k = 0; k < n; k++) { h ^= ((const unsigned char *)p)[k]; h *= 1099511628211ull; }
  return h;
}

#define SAME(field) (std::memcmp(&w.field, &b.field, sizeof(w.field)) == 0)

int main(int argc, char **argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s fly_walk.ffmb fly_ball.ffmb\n", argv[0]); return 2; }
  try {
    const std::vector<char> wb = slurp(argv[1]), bb = slurp(argv[2]);
    const ffb::WalkHost W = ffb::build_walk_model(ffb::Blob(wb.data(), wb.size()));
    const ffb::BallHost B = ffb::build_ball_model(ffb::Blob(bb.data(), bb.size()));
    const ffb::BallModel &w = W.m.b, &b = B.m;
    int nlinks = 0, nhalt = 0, ndof = 0, nact = 0;
    for (int l = 0; l < ffb::NL; l++) {
      nlinks += w.l_body[l] > 0 ? 1 : 0;
      nhalt += w.x_on[l] ? 1 : 0;
      for (int s = 0; s < 4; s++) ndof += w.s_dof[s][l] >= 0 ? 1 : 0;
    }
    for (int a = 0; a < ffb::NL; a++) nact += w.a_tau[a] > 0.f ? 1 : 0;
    std::printf("links %d\nhalteres %d\nhinge_dofs %d\nblocks %d\nactuators %d\n", nlinks, nhalt, ndof, w.nblk, nact);
    std::printf("nM %d\nnfs %d\nnp1 %d\nnp2 %d\n", w.nM, w.nfs, w.np1, w.np2);
    std::printf("root_mass %.17g\ntotal_mass %.17g\n", W.root_mass, W.total_mass);
    std::printf("floor_geom %d\nlimited_hinges %d\n", W.m.x.floor_geom, W.m.x.n_limited);
    std::printf("timestep %.9g\ngravity_z %.9g\n", (double)w.h, (double)w.gz);
    // the tables the leg code reads must be the ball builder's own
    const bool same_tree = SAME(l_parent) && SAME(l_depth) && SAME(l_ndof) && SAME(l_pack) && SAME(l_tree) && SAME(l_kids) && SAME(maxsub) && SAME(l_chain) && SAME(l_nchain);
    const bool same_dofs = SAME(s_dof) && SAME(s_axis) && SAME(s_stiff) && SAME(s_sref) && SAME(s_damp) && SAME(s_lo) && SAME(s_hi) && SAME(s_limited) && SAME(d_parent) &&
                           SAME(d_madr) && SAME(d_blk) && SAME(d_li) && SAME(d_amask) && SAME(x_on);
    const bool same_sched = SAME(fac_a) && SAME(fac_b) && SAME(p1) && SAME(p2) && SAME(ent_a) && SAME(ent_b) && SAME(nfs) && SAME(np1) && SAME(np2) && SAME(nM) && SAME(nblk);
    const bool same_act = SAME(a_trn) && SAME(a_nwrap) && SAME(a_wdof) && SAME(a_wcoef) && SAME(a_gain) && SAME(a_b0) && SAME(a_b1) && SAME(a_b2) && SAME(a_clo) && SAME(a_chi) &&
                          SAME(a_flo) && SAME(a_fhi) && SAME(a_tau) && SAME(a_climited) && SAME(a_flimited) && SAME(s_act) && SAME(s_actcoef) && SAME(act_lo) && SAME(act_hi);
    const bool same_mass = SAME(l_mass) && SAME(l_ipos) && SAME(l_iquat) && SAME(l_inertia) && SAME(l_fl);
    std::printf("same_tree %d\nsame_dofs %d\nsame_schedules %d\nsame_actuators %d\nsame_link_inertia %d\n", same_tree, same_dofs, same_sched, same_act, same_mass);
    std::printf("ball_model_bytes %zu\nball_model_fnv %016llx\n", sizeof(ffb::BallModel), fnv(&b, sizeof(b)));
    // a blob that is not the walk model is refused with a text
    try {
      (void)ffb::build_walk_model(ffb::Blob(bb.data(), bb.size()));
      std::printf("ball_blob_refused 0\n");
    } catch (const std::exception &e) { std::printf("ball_blob_refused 1\n"); std::fprintf(stderr, "refusal: %s\n", e.what()); }
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
