// walk_self_sense.hpp - what the fly's own contacts add to the force and touch sensors of the walking fly (walk_imitation on the floor
// with self_contacts), next to walk_sense.hpp, whose functions stay as they are.
//
// mj: mj_rnePostConstraint / mj_sensorAcc add a contact's force to the bodies of both geoms: -frame' f on geom1's body, +frame' f on
// geom2's.  A fly-fly contact is condim 1: one force f along the normal n from geom1 to geom2, so
//   f_ext    += n f on the link of geom2 (`pos`, c_link), -= n f on the link of geom1 (`neg`, c_link1).  A geom of the thorax has no link:
//            the thorax is the root, above every force sensor, and contributes to none.  The subtree sum of walk_sense.hpp does the
//            rest: a contact between two links of one sensor's subtree cancels there, as it must (an internal force).
//   touch    the positive normal forces of the contacts that have rows and lie on the claw's link, on either side of the pair
//            (tests/test_walk_self_env_cpu.py checks that against the oracle's ray test on the shipped model).
// Templated on the scalar type so that the host can compile it (tests/walk_self_sense_host.cpp compares both instantiations with the
// float64 oracle); the kernel calls the float32 one.
#pragma once

#include "walk_sense.hpp"

namespace wss {

// acc += (on_pos - on_neg) n f: a fly-fly contact's force on a link that carries geom2 (`on_pos`) or geom1 (`on_neg`) of the pair
template <class T>
WF_FN void add_pair_force(const T *n, T f, bool on_pos, bool on_neg, T *acc) {
  const T s = (on_pos ? T(1) : T(0)) - (on_neg ? T(1) : T(0));
  for (int k = 0; k < 3; k++) acc[k] += s * n[k] * f;
}
// a fly-fly contact's share of the touch sensor of a link on either side of it
template <class T>
WF_FN T pair_touch_share(T normal_force, bool on_pos, bool on_neg) { return (on_pos || on_neg) ? ws::touch_share<T>(normal_force) : T(0); }

}  // namespace wss
