// walk_imu.hpp - the thorax IMU of the walking fly in closed form (walk_imitation).
//
// The IMU site (gyro, velocimeter, accelerometer) sits on the thorax, and the thorax is the free root: its pose, velocity and
// acceleration are the first seven qpos, six qvel and six qacc entries, so the three sensors need no pass over the tree.  With R the
// root's rotation, r and R_s the site's position and orientation in the root frame, w the root's angular velocity (body frame, as a
// free joint stores it), v the linear velocity of the root origin (world frame), and (a, wd) the root rows of qacc (world, body):
//   gyro          = R_s' w                                                mj_objectVelocity(mjOBJ_SITE, local), angular half
//   velocimeter   = R_s' (R' v + w x r)                                   ... linear half
//   accelerometer = R_s' (R' (a - g) + wd x r + w x (w x r))              mj_objectAcceleration: the spatial acceleration moved to the
//                                                                         site plus its Coriolis term w_s x v_s, on top of cacc[world] = -g
// (the classical acceleration of the site point minus gravity).  Templated on the scalar type so that the host can compile it
// (tests/walk_imu_host.cpp compares it with the float64 oracle); the step kernel of walk_env.hip calls it in float32.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WI_FN __host__ __device__ __forceinline__
#else
#define WI_FN inline
#endif

namespace wi {

template <class T>
struct Imu {
  T gyro[3], velocimeter[3], accelerometer[3];
};

template <class T>
WI_FN void cross(T *r, const T *a, const T *b) {
  const T x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
  r[0] = x; r[1] = y; r[2] = z;
}
// rotation matrix of a unit quaternion (w, x, y, z), row-major (mju_quat2Mat)
template <class T>
WI_FN void quat2mat(T *m, const T *q) {
  const T w = q[0], x = q[1], y = q[2], z = q[3];
  m[0] = w * w + x * x - y * y - z * z; m[1] = 2 * (x * y - w * z); m[2] = 2 * (x * z + w * y);
  m[3] = 2 * (x * y + w * z); m[4] = w * w - x * x + y * y - z * z; m[5] = 2 * (y * z - w * x);
  m[6] = 2 * (x * z - w * y); m[7] = 2 * (y * z + w * x); m[8] = w * w - x * x - y * y + z * z;
}
template <class T>
WI_FN void mat_t_vec(T *r, const T *m, const T *v) {  // r = m' v
  const T x = m[0] * v[0] + m[3] * v[1] + m[6] * v[2], y = m[1] * v[0] + m[4] * v[1] + m[7] * v[2], z = m[2] * v[0] + m[5] * v[1] + m[8] * v[2];
  r[0] = x; r[1] = y; r[2] = z;
}

// gyro and velocimeter of the root state (quat: root orientation; vlin: world frame; wb: body frame)
template <class T>
WI_FN void imu_velocity(const T *quat, const T *vlin, const T *wb, const T *site_pos, const T *site_quat, T *gyro, T *velocimeter) {
  T R[9], Rs[9], vb[3], wr[3];
  quat2mat(R, quat);
  quat2mat(Rs, site_quat);
  mat_t_vec(vb, R, vlin);
  cross(wr, wb, site_pos);
  for (int k = 0; k < 3; k++) vb[k] += wr[k];
  mat_t_vec(gyro, Rs, wb);
  mat_t_vec(velocimeter, Rs, vb);
}

// accelerometer of the root state and the root rows of qacc (alin: world frame; wd: body frame); gz: gravity along world z (0: off)
template <class T>
WI_FN void imu_acceleration(const T *quat, const T *wb, const T *alin, const T *wd, T gz, const T *site_pos, const T *site_quat, T *accelerometer) {
  T R[9], Rs[9], ab[3], t[3], u[3];
  quat2mat(R, quat);
  quat2mat(Rs, site_quat);
  const T aw[3] = {alin[0], alin[1], alin[2] - gz};
  mat_t_vec(ab, R, aw);
  cross(t, wd, site_pos);
  cross(u, wb, site_pos);
  cross(u, wb, u);
  for (int k = 0; k < 3; k++) ab[k] += t[k] + u[k];
  mat_t_vec(accelerometer, Rs, ab);
}

}  // namespace wi
