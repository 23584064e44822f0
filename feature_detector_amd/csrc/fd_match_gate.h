// The model gate of fd_brief_match_model / fd_nn_match_model (include/fd_hip.h), shared by both matchers
// (fd_match.hip, fd_nn_match.hip): which instance a launch takes, and the pair test on the per-entry gate
// vectors that k_match_gate_vectors (fd_match.hip) writes. All of it is double, one rounding per operation
// (the files are built without contraction).
//
// Gate vectors, four doubles per entry. F: query (l0, l1, l2, l0*l0 + l1*l1), train (u, v, 1.0, m0*m0 + m1*m1).
// H: query (px, py, w, (t*t) * (w*w)), train (u, v, 0, 0).
//
// F needs no roles. With the train side's third entry 1.0, e = (u*l0 + v*l1) + l2 is the grouped product
// (o0*x0 + o1*x1) + o2*x2 of the lane's own vector o and the other set's vector x, and the bound's sum is
// o3 + x3: products and sums commute bit for bit and l2 * 1.0 is l2, so either side may be the lane's own.
// H is directional (px - u*w has no such form): the forward and the reverse pass are two instances that take
// their operands from opposite sides and form the identical expression.
#pragma once

#include "fd_device.h"

namespace fdk {

// A matcher instance's gate. Every gate but kGateNone applies the window (a.a_xy, a.b_xy, a.radius_x / _y).
enum : int { kGateNone = 0, kGateWindow = 1, kGateF = 2, kGateHFwd = 3, kGateHRev = 4 };

// The instance a launch takes (Args: MatchArgs or NnMatchArgs).
template <typename Args>
int gate_of(const Args &a) {
    if (!a.a_xy) return kGateNone;
    if (!a.a_gate) return kGateWindow;
    if (a.gate_model == 0) return kGateF;
    return a.a_is_query ? kGateHFwd : kGateHRev;
}

// own: the gate vector of the lane's "a" entry, oth: the "b" entry's; tt = t*t. A NaN fails the compare.
template <int GATE>
__device__ __forceinline__ bool model_pass(const double (&own)[4], const double (&oth)[4], double tt) {
    static_assert(GATE == kGateF || GATE == kGateHFwd || GATE == kGateHRev, "a model gate");
    if constexpr (GATE == kGateF) {
        const double e = (own[0] * oth[0] + own[1] * oth[1]) + own[2] * oth[2];
        return e * e <= tt * (own[3] + oth[3]);
    } else {
        const double(&q)[4] = GATE == kGateHFwd ? own : oth;
        const double(&t)[4] = GATE == kGateHFwd ? oth : own;
        const double dx = q[0] - t[0] * q[2];
        const double dy = q[1] - t[1] * q[2];
        return dx * dx + dy * dy <= q[3];
    }
}

}  // namespace fdk
