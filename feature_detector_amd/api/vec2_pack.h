// Vec2 positions <-> the [n][2] float (x, y) arrays of the C ABI (include/fd_hip.h). Private to the api sources.
#ifndef FEATURE_DETECTOR_API_VEC2_PACK_H_
#define FEATURE_DETECTOR_API_VEC2_PACK_H_

#include <cstddef>
#include <vector>

#include "feature_detector/fd_types.h"

namespace feature_detector {

inline std::vector<float> Flatten(const Vec2 *uv, size_t n) {
    std::vector<float> xy(2 * n);
    for (size_t i = 0; i < n; ++i) {
        xy[2 * i] = uv[i].x();
        xy[2 * i + 1] = uv[i].y();
    }
    return xy;
}

inline std::vector<float> Flatten(const std::vector<Vec2> &uv) { return Flatten(uv.data(), uv.size()); }

inline std::vector<Vec2> Unflatten(const float *xy, size_t n) {
    std::vector<Vec2> uv;
    uv.reserve(n);
    for (size_t i = 0; i < n; ++i) uv.emplace_back(Vec2(xy[2 * i], xy[2 * i + 1]));
    return uv;
}

}  // namespace feature_detector

#endif  // FEATURE_DETECTOR_API_VEC2_PACK_H_
