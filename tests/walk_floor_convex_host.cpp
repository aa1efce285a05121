// Stand-alone host program for tests/test_walk_floor_convex_cpu.py (built with -fsanitize=address,undefined, never loaded into Python):
//   walk_floor_convex_host <fly_walk.ffmb> <poses.bin> <out.bin>
// 1. The second floor table (csrc/walk_self_model.hpp `build_walk_floor_convex`): prints `table_rows`, `table_ok`, one `row` line per
//    row (geom, type, link, adhesion actuator, block, chain mask), and `extra_untouched` / `first_table_untouched`: WalkExtra's bytes and
//    the 48-row table are what `build_walk_model` left.
// 2. Both instantiations of csrc/walk_floor_convex.hpp on the poses of poses.bin (float64: npose; per pose: type 4 / 5, n[3], x0[3],
//    c[3], R[9] row-major, size[3], margin), formed as the kernel forms them: the plane distance's first term in float64
//    (wf::plane_distance), the position by wf::contact_position with radius 0.  out.bin (float64): per pose and scalar type (float64 first):
//    the mask of contacts, then four slots of (pos[3], dist); an ellipsoid uses slot 0.
#define CVX_HOST 1  // convex.hpp (pulled in by dev_model.hpp) without the HIP runtime
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

struct float4 { float x, y, z, w; };  // the one HIP vector type dev_model.hpp names (flight tables, unused here)

#include "../flybody_amd/csrc/walk_self_model.hpp"
#include "../flybody_amd/csrc/walk_floor_convex.hpp"

using namespace ffb;

static std::vector<char> slurp(const char *path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw std::runtime_error(std::string("cannot open ") + path);
  return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

template <class T>
static void run(const double *p, std::vector<double> &out) {
  const int type = (int)p[0];
  T n[3], c[3], R[9], s[3];
  for (int k = 0; k < 3; k++) { n[k] = (T)p[1 + k]; c[k] = (T)p[7 + k]; s[k] = (T)p[19 + k]; }
  for (int k = 0; k < 9; k++) R[k] = (T)p[10 + k];
  const T margin = (T)p[22];
  const double height = -(p[1] * p[4] + p[2] * p[5] + p[3] * p[6]);  // n . (origin - x0): the frame's origin plays the root's part
  T sp[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, dist[4] = {0, 0, 0, 0};
  int mask;
  if (type == 4) {
    wfc::ellipsoid_support<T>(n, c, R, s, sp[0]);
    dist[0] = wf::plane_distance<T>(height, n, sp[0], T(0));
    mask = dist[0] <= margin ? 1 : 0;
  } else {
    const T dist0 = wf::plane_distance<T>(height, n, c, T(0));
    mask = wfc::plane_cylinder<T>(n, c, R, s[0], s[1], dist0, margin, sp, dist);
  }
  out.push_back((double)mask);
  for (int e = 0; e < 4; e++) {
    T pos[3];
    wf::contact_position<T>(sp[e], n, T(0), dist[e], pos);
    for (int k = 0; k < 3; k++) out.push_back((double)pos[k]);
    out.push_back((double)dist[e]);
  }
}

int main(int argc, char **argv) {
  if (argc != 4) { std::fprintf(stderr, "usage: walk_floor_convex_host <blob> <poses.bin> <out.bin>\n"); return 2; }
  try {
    const std::vector<char> raw = slurp(argv[1]);
    Blob b(raw.data(), raw.size());
    WalkHost W = build_walk_model(b);
    const WalkExtra before = W.m.x;
    build_walk_floor_convex(b, W);
    const WalkFloorConvex &F = W.xc;
    std::printf("table_rows %d\ntable_ok %d\n", F.n, F.ok);
    for (int s = 0; s < F.n; s++) std::printf("row%d %d %d %d %d %d %d\n", s, F.geom[s], F.type[s], F.link[s], F.adh[s], F.blk[s], F.amask[s]);
    std::printf("extra_untouched %d\n", std::memcmp(&before, &W.m.x, sizeof(WalkExtra)) == 0 ? 1 : 0);
    std::printf("first_table_rows %d\n", W.m.x.f_n);
    for (int s = 0; s < W.m.x.f_n; s++) std::printf("first%d %d %d\n", s, W.m.x.f_geom[s], W.m.x.f_link[s]);
    // the pair parameters are floor_geom_params' (rounded to float32)
    int params_ok = 1;
    for (int s = 0; s < F.n; s++) {
      const FloorGeom fp = floor_geom_params(b, W.m.x.floor_geom, F.geom[s]);
      params_ok &= F.fric[s] == (float)fp.fric && F.K[s] == (float)fp.K && F.B[s] == (float)fp.B && F.margin[s] == (float)fp.margin &&
                   F.gap[s] == (float)fp.gap && F.invw[s] == (float)fp.invw;
    }
    std::printf("params_ok %d\n", params_ok);
    const std::vector<char> pb = slurp(argv[2]);
    if (pb.size() < sizeof(double)) throw std::runtime_error("poses file: truncated");
    std::vector<double> poses(pb.size() / sizeof(double));
    std::memcpy(poses.data(), pb.data(), poses.size() * sizeof(double));
    const int np = (int)poses[0];
    if (poses.size() != (size_t)1 + (size_t)np * 23) throw std::runtime_error("poses file: unexpected size");
    std::vector<double> out;
    for (int i = 0; i < np; i++) {
      run<double>(&poses[1 + (size_t)i * 23], out);
      run<float>(&poses[1 + (size_t)i * 23], out);
    }
    std::ofstream o(argv[3], std::ios::binary);
    o.write(reinterpret_cast<const char *>(out.data()), (std::streamsize)(out.size() * sizeof(double)));
    std::printf("poses %d\n", np);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "walk_floor_convex_host: %s\n", e.what());
    return 1;
  }
  return 0;
}
