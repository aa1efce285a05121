// Host harness of csrc/walk_imu.hpp (tests/test_walk_episode_cpu.py builds it with -fsanitize=address,undefined and runs it on its
// own): the closed-form thorax IMU in float64 and float32 on root states of the float64 oracle, against the oracle's own sensors.
//
// Input file (float64): n, site_pos[3], site_quat[4], gravity_z, then n records of
//   root quaternion 4 | vlin 3 (world) | wb 3 (body) | root qacc 6 | gyro 3 | velocimeter 3 | accelerometer 3.
// Output: one "key value" line per figure; errors are per group, relative to max(1, max |reference|) of the group over all states.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "../flybody_amd/csrc/walk_imu.hpp"

template <class T>
static void run(const std::vector<double> &in, int n, double (&err)[3], double (&scale)[3]) {
  T sp[3], sq[4];
  for (int k = 0; k < 3; k++) sp[k] = (T)in[1 + k];
  for (int k = 0; k < 4; k++) sq[k] = (T)in[4 + k];
  const T gz = (T)in[8];
  for (int g = 0; g < 3; g++) { err[g] = 0; scale[g] = 1; }
  for (int i = 0; i < n; i++) {
    const double *r = in.data() + 9 + (size_t)i * 25;
    T q[4], v[3], w[3], a[3], wd[3];
    for (int k = 0; k < 4; k++) q[k] = (T)r[k];
    for (int k = 0; k < 3; k++) { v[k] = (T)r[4 + k]; w[k] = (T)r[7 + k]; a[k] = (T)r[10 + k]; wd[k] = (T)r[13 + k]; }
    wi::Imu<T> s;
    wi::imu_velocity(q, v, w, sp, sq, s.gyro, s.velocimeter);
    wi::imu_acceleration(q, w, a, wd, gz, sp, sq, s.accelerometer);
    const T *got[3] = {s.gyro, s.velocimeter, s.accelerometer};
    for (int g = 0; g < 3; g++)
      for (int k = 0; k < 3; k++) {
        const double ref = r[16 + 3 * g + k];
        err[g] = std::max(err[g], std::fabs((double)got[g][k] - ref));
        scale[g] = std::max(scale[g], std::fabs(ref));
      }
  }
}

int main(int argc, char **argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: walk_imu_host states.bin\n"); return 2; }
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::vector<double> in;
  double buf[256];
  size_t got;
  while ((got = std::fread(buf, sizeof(double), 256, f)) > 0) in.insert(in.end(), buf, buf + got);
  std::fclose(f);
  if (in.size() < 9) { std::fprintf(stderr, "short file\n"); return 2; }
  const int n = (int)in[0];
  if (n < 0 || in.size() != 9 + (size_t)n * 25) { std::fprintf(stderr, "the file holds %zu values, %d records need %zu\n", in.size(), n, 9 + (size_t)n * 25); return 2; }
  double e64[3], e32[3], sc[3];
  run<double>(in, n, e64, sc);
  static const char *name[3] = {"gyro", "velocimeter", "accelerometer"};
  std::printf("states %d\n", n);
  for (int g = 0; g < 3; g++) std::printf("f64_%s %.6e\n", name[g], e64[g] / sc[g]);
  run<float>(in, n, e32, sc);
  for (int g = 0; g < 3; g++) std::printf("f32_%s %.6e\n", name[g], e32[g] / sc[g]);
  for (int g = 0; g < 3; g++) std::printf("scale_%s %.6e\n", name[g], sc[g]);
  return 0;
}
