// Host build of flybody_amd/csrc/walk_task.hpp (-DWT_HOST): the same maths and table packing the HIP kernels use, in both scalar
// types, behind a small C interface for tests/test_walk_task_cpu.py.  Every reference row index the code forms is recorded
// (WT_RECORD_ROW) so the clamp tests can assert that none leaves its clip.
#include <climits>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#define WT_HOST 1
static long long g_rows_formed = 0, g_rows_outside = 0;
static int g_min_rel = INT_MAX, g_max_rel_end = INT_MIN;  // smallest row - first row; largest row - (one past the last row)
#define WT_RECORD_ROW(row, lo, hi)                               \
  do {                                                           \
    g_rows_formed++;                                             \
    if ((row) < (lo) || (row) >= (hi)) g_rows_outside++;         \
    if ((row) - (lo) < g_min_rel) g_min_rel = (row) - (lo);      \
    if ((row) - (hi) > g_max_rel_end) g_max_rel_end = (row) - (hi); \
  } while (0)
#include "../flybody_amd/csrc/walk_task.hpp"

namespace {
struct Handle {
  bool f64 = false;
  wt::Packed<float> pf;
  wt::Packed<double> pd;
  wt::Tables<float> tf;
  wt::Tables<double> td;
};

template <class T>
void features(const wt::Tables<T> &t, const double *qpos, const double *qvel, int n, double *com, T *qv, T *r2s, T *jq) {
  std::vector<T> P(7 * (size_t)t.nbody), AX(3 * (size_t)t.njnt);
  for (size_t i = 0; i < (size_t)n; i++) {
    wt::RowOut<T> o{};
    o.com = com ? com + 3 * i : nullptr;
    o.qvel = qv ? qv + i * (6 + t.J) : nullptr;
    o.r2s = r2s ? r2s + i * 3 * t.S : nullptr;
    o.jq = jq ? jq + i * 4 * (1 + t.J) : nullptr;
    wt::row_task<T, false>(t, qpos + i * t.nq, qvel ? qvel + i * t.nv : nullptr, 0, 0, o, P.data(), AX.data());
  }
}
template <class T>
void evaluate(const wt::Tables<T> &t, const double *qpos, const double *qvel, const int *clip, const int *step, int n, T *factors, T *reward,
              int *term, T *obs, int stride) {
  std::vector<T> P(7 * (size_t)t.nbody), AX(3 * (size_t)t.njnt);
  for (size_t i = 0; i < (size_t)n; i++) {
    wt::RowOut<T> o{};
    o.factors = factors ? factors + 4 * i : nullptr;
    o.reward = reward ? reward + i : nullptr;
    o.term = term ? term + i : nullptr;
    o.obs = obs ? obs + i * (size_t)stride : nullptr;
    wt::row_task<T, true>(t, qpos + i * t.nq, qvel + i * t.nv, clip[i], step[i], o, P.data(), AX.data());
  }
}
}  // namespace

extern "C" {

void *wth_create(const void *blob, size_t size, const ffe_walk_task *task, int f64, char *err, int errlen) {
  Handle *h = new Handle();
  h->f64 = f64 != 0;
  std::string e;
  const bool ok = h->f64 ? h->pd.build(blob, size, task, e) : h->pf.build(blob, size, task, e);
  if (!ok) {
    if (err && errlen > 0) std::snprintf(err, (size_t)errlen, "%s", e.c_str());
    delete h;
    return nullptr;
  }
  if (h->f64) h->td = h->pd.rebase(h->pd.arena.data()); else h->tf = h->pf.rebase(h->pf.arena.data());
  return h;
}
void wth_destroy(void *p) { delete static_cast<Handle *>(p); }

void wth_features(void *p, const double *qpos, const double *qvel, int n, double *com, void *qv, void *r2s, void *jq) {
  Handle *h = static_cast<Handle *>(p);
  if (h->f64) features<double>(h->td, qpos, qvel, n, com, (double *)qv, (double *)r2s, (double *)jq);
  else features<float>(h->tf, qpos, qvel, n, com, (float *)qv, (float *)r2s, (float *)jq);
}
int wth_evaluate(void *p, const double *qpos, const double *qvel, const int *clip, const int *step, int n, void *factors, void *reward, int *term,
                 void *obs, int stride) {
  Handle *h = static_cast<Handle *>(p);
  if (obs && stride < (h->f64 ? h->td.obs_dim : h->tf.obs_dim)) return -1;
  if (h->f64) evaluate<double>(h->td, qpos, qvel, clip, step, n, (double *)factors, (double *)reward, term, (double *)obs, stride);
  else evaluate<float>(h->tf, qpos, qvel, clip, step, n, (float *)factors, (float *)reward, term, (float *)obs, stride);
  return 0;
}
void wth_reference_pose(void *p, const int *clip, const int *step, int n, double *qpos, double *qvel) {
  Handle *h = static_cast<Handle *>(p);
  for (size_t i = 0; i < (size_t)n; i++) {
    if (h->f64) wt::row_reference_pose<double>(h->td, clip[i], step[i], qpos + i * h->td.nq, qvel + i * h->td.nv);
    else wt::row_reference_pose<float>(h->tf, clip[i], step[i], qpos + i * h->tf.nq, qvel + i * h->tf.nv);
  }
}
void wth_info(void *p, int *dims, int *episode_steps) {
  Handle *h = static_cast<Handle *>(p);
  auto fill = [&](const auto &t, const std::vector<int> &ep) {
    const int v[16] = {t.nq, t.nv, t.J, t.S, t.ntraj, t.future, t.obs_dim, t.off_app, t.off_jpos, t.off_jvel, t.off_disp, t.off_rquat, t.off_zaxis,
                       t.nappend, t.nobsj, h->f64 ? 1 : 0};
    for (int k = 0; k < 16; k++) dims[k] = v[k];
    if (episode_steps)
      for (size_t c = 0; c < ep.size(); c++) episode_steps[c] = ep[c];
  };
  if (h->f64) fill(h->td, h->pd.ep_steps); else fill(h->tf, h->pf.ep_steps);
}
// a packed table as the kernels see it: 0 b_depth, 1 pose_src (int32) / 2 pose_const, 3 r_root7 (float64); returns the element count copied
int wth_table(void *p, int which, void *out, int cap) {
  Handle *h = static_cast<Handle *>(p);
  auto get = [&](const auto &t) -> int {
    const size_t rows = t.ntraj > 0 ? (size_t)t.traj_off[t.ntraj] : 0;
    const void *src = nullptr; size_t n = 0, w = 4;
    if (which == 0) { src = t.b_depth; n = t.nbody; }
    else if (which == 1) { src = t.pose_src; n = t.nq; }
    else if (which == 2) { src = t.pose_const; n = t.nq; w = 8; }
    else if (which == 3) { src = t.r_root7; n = rows * 7; w = 8; }
    if (!src || (int)n > cap) return -1;
    std::memcpy(out, src, n * w);
    return (int)n;
  };
  return h->f64 ? get(h->td) : get(h->tf);
}
// joint_orientation_quat / short-arc distance squared of the header on their own (edge branches, goldens)
void wth_joint_orientation_quat(const double *axis, double ang, int f64, double *out) {
  if (f64) { wt::joint_orientation_quat<double>(out, axis, ang); return; }
  const float a[3] = {(float)axis[0], (float)axis[1], (float)axis[2]};
  float q[4];
  wt::joint_orientation_quat<float>(q, a, (float)ang);
  for (int k = 0; k < 4; k++) out[k] = q[k];
}
double wth_short_arc_sq(const double *a, const double *b, int f64) {
  if (f64) return wt::short_arc_sq<double>(a, b);
  const float fa[4] = {(float)a[0], (float)a[1], (float)a[2], (float)a[3]}, fb[4] = {(float)b[0], (float)b[1], (float)b[2], (float)b[3]};
  return wt::short_arc_sq<float>(fa, fb);
}
// rows formed since the last call, how many lay outside their clip, min(row - first), max(row - end); resets the record
void wth_row_record(long long *out4) {
  out4[0] = g_rows_formed; out4[1] = g_rows_outside; out4[2] = g_min_rel; out4[3] = g_max_rel_end;
  g_rows_formed = g_rows_outside = 0; g_min_rel = INT_MAX; g_max_rel_end = INT_MIN;
}

}  // extern "C"

#if defined(WTH_MAIN)
// Stand-alone driver for sanitizer builds (never loaded into Python):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -DWTH_MAIN tests/walk_task_host.cpp -o wth && ./wth flybody_amd/assets/fly_walk.ffmb
// Every hinge and every site tracked, three random clips, steps from far below to far beyond each clip in both scalar types.
#include <cstdlib>
#include <fstream>
#include <iterator>
int main(int argc, char **argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s model.ffmb\n", argv[0]); return 2; }
  std::ifstream f(argv[1], std::ios::binary);
  std::vector<char> blob((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  wt::BlobView bv;
  std::string e;
  std::vector<int> jtype, sbody;
  std::vector<double> qpos0;
  if (!bv.parse(blob.data(), blob.size(), e) || !bv.ints("jnt_type", jtype, e) || !bv.ints("sites_bodyid", sbody, e) || !bv.reals("qpos0", qpos0, e)) {
    std::fprintf(stderr, "%s\n", e.c_str());
    return 2;
  }
  std::vector<int32_t> joints, sites;
  for (size_t j = 0; j < jtype.size(); j++) if (jtype[j] == wt::kJntHinge) joints.push_back((int32_t)j);
  for (size_t s = 0; s < sbody.size(); s++) sites.push_back((int32_t)s);
  const int J = (int)joints.size(), S = (int)sites.size(), F = 64;
  const std::vector<int32_t> off = {0, 66, 166, 283};
  const size_t rows = (size_t)off.back();
  auto rnd = [](size_t n) { std::vector<double> v(n); for (auto &x : v) x = std::rand() / (double)RAND_MAX - 0.5; return v; };
  std::vector<double> rq = rnd(rows * (7 + J)), rv = rnd(rows * (6 + J)), rs = rnd(rows * 3 * S), rj = rnd(rows * 4 * J);
  ffe_walk_task task{};
  task.n_joints = J; task.joints = joints.data(); task.n_sites = S; task.sites = sites.data();
  task.ntraj = 3; task.traj_off = off.data(); task.ref_qpos = rq.data(); task.ref_qvel = rv.data(); task.ref_root2site = rs.data(); task.ref_joint_quat = rj.data();
  task.future_steps = F; task.control_timestep = 2e-3; task.time_limit = 10.0; task.terminal_com_dist = 0.3;
  const double sd[4] = {0.078487, 53.7801, 0.0735, 1.2247}, wg[4] = {20, 1, 1, 1};
  for (int k = 0; k < 4; k++) { task.std[k] = sd[k]; task.weights[k] = wg[k]; }
  const int nq = (int)qpos0.size();
  for (int f64 = 0; f64 < 2; f64++) {
    char err[256] = "";
    void *h = wth_create(blob.data(), blob.size(), &task, f64, err, sizeof err);
    if (!h) { std::fprintf(stderr, "%s\n", err); return 1; }
    int dims[16];
    wth_info(h, dims, nullptr);
    std::vector<int> clip, step;
    for (int c = -1; c <= 3; c++)
      for (int k = -80; k <= 200; k++) { clip.push_back(c); step.push_back(k); }
    for (int k : {INT_MAX, INT_MIN, INT_MAX - 30}) { clip.push_back(2); step.push_back(k); }
    const int n = (int)clip.size();
    std::vector<double> qpos((size_t)n * nq), qvel((size_t)n * dims[1]);
    wth_reference_pose(h, clip.data(), step.data(), n, qpos.data(), qvel.data());
    const size_t w = f64 ? 8 : 4;
    std::vector<unsigned char> fac(n * 4 * w), rew(n * w), obs((size_t)n * dims[6] * w), qv((size_t)n * (6 + J) * w), r2s((size_t)n * 3 * S * w),
        jq((size_t)n * 4 * (1 + J) * w);
    std::vector<int> term(n);
    std::vector<double> com((size_t)n * 3);
    if (wth_evaluate(h, qpos.data(), qvel.data(), clip.data(), step.data(), n, fac.data(), rew.data(), term.data(), obs.data(), dims[6])) return 1;
    wth_features(h, qpos.data(), qvel.data(), n, com.data(), qv.data(), r2s.data(), jq.data());
    long long rec[4];
    wth_row_record(rec);
    std::printf("%s: %d states, %lld reference rows formed, %lld outside their clip\n", f64 ? "float64" : "float32", n, rec[0], rec[1]);
    if (rec[1] != 0) return 1;
    wth_destroy(h);
  }
  return 0;
}
#endif
