// Headless demo of GeometricVerifier::BundleAdjust (an MI355X extension; the reference has no such stage): the
// poses of a file and the points and slot-aligned observations of another refined together.
// Prints JSON lines; doubles and floats as the decimal bit patterns of their 64 / 32 bits.
//   usage: fd_demo_ba <raw float32 file of n x (3 + 2 cams): X Y Z, then u v per camera> <raw float64 file of cams x 12>
//                     <n> <cams> <fx fy cx cy> <rounds> <threshold> <lambda> <up> <down> <fixed flags, e.g. 110>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "demo_util.h"
#include "feature_detector/geometric_verifier.h"

using namespace feature_detector;

template <typename T>
static bool ReadRaw(const char *path, std::vector<T> &v) {
    FILE *f = std::fopen(path, "rb");
    const bool read = f && std::fread(v.data(), sizeof(T), v.size(), f) == v.size();
    if (f) std::fclose(f);
    if (!read) std::fprintf(stderr, "cannot read %s\n", path);
    return read;
}

int main(int argc, char **argv) {
    if (argc < 15) {
        std::fprintf(stderr, "usage: %s <points.f32> <poses.f64> <n> <cams> <fx fy cx cy> <rounds> <threshold> <lambda> <up> <down> <fixed>\n",
                     argv[0]);
        return 2;
    }
    const size_t n = static_cast<size_t>(std::atoi(argv[3])), cams = static_cast<size_t>(std::atoi(argv[4]));
    const size_t width = 3 + 2 * cams;
    std::vector<float> raw(width * n);
    std::vector<double> raw_poses(12 * cams);
    if (!ReadRaw(argv[1], raw) || !ReadRaw(argv[2], raw_poses)) return 2;
    std::vector<std::array<float, 3>> points(n);
    std::vector<std::vector<Vec2>> obs(cams, std::vector<Vec2>(n));
    std::vector<std::array<double, 12>> poses(cams);
    for (size_t i = 0; i < n; ++i) {
        points[i] = {raw[width * i], raw[width * i + 1], raw[width * i + 2]};
        for (size_t c = 0; c < cams; ++c) obs[c][i] = Vec2(raw[width * i + 3 + 2 * c], raw[width * i + 4 + 2 * c]);
    }
    for (size_t c = 0; c < cams; ++c) std::copy(raw_poses.begin() + 12 * c, raw_poses.begin() + 12 * (c + 1), poses[c].begin());
    GeometricVerifier::Camera cam{std::atof(argv[5]), std::atof(argv[6]), std::atof(argv[7]), std::atof(argv[8])};
    GeometricVerifier verifier;
    GeometricVerifier::BundleOptions &o = verifier.bundle_options();
    o.kRounds = std::atoi(argv[9]);
    o.kThreshold = static_cast<float>(std::atof(argv[10]));
    o.kLambda = std::atof(argv[11]);
    o.kUp = std::atof(argv[12]);
    o.kDown = std::atof(argv[13]);
    std::vector<uint8_t> fixed(cams, 0);
    for (size_t c = 0; c < cams && c < std::strlen(argv[14]); ++c) fixed[c] = argv[14][c] != '0';

    const std::vector<std::array<double, 12>> given_poses = poses;
    const std::vector<std::array<float, 3>> given_points = points;
    std::vector<std::vector<uint8_t>> inlier;
    std::array<double, 2> cost{{-1.0, -1.0}};
    int32_t accepted = -1;
    const bool ok = verifier.BundleAdjust(poses, points, obs, cam, inlier, nullptr, nullptr, &fixed, &cost, &accepted);
    std::printf("{\"test\": \"adjust\", \"ok\": %s, \"extra\": %d, \"pose_bits\": [", ok ? "true" : "false", accepted);
    for (size_t c = 0; c < cams; ++c)
        for (size_t k = 0; k < 12; ++k) std::printf("%s%llu", c + k ? ", " : "", Bits(poses[c][k]));
    std::printf("], \"point_bits\": [");
    for (size_t i = 0; i < n; ++i)
        for (size_t k = 0; k < 3; ++k) std::printf("%s%u", i + k ? ", " : "", Bits(points[i][k]));
    std::printf("], \"inlier\": [");
    for (size_t c = 0; c < inlier.size(); ++c)
        for (size_t i = 0; i < inlier[c].size(); ++i) std::printf("%s%d", c + i ? ", " : "", inlier[c][i]);
    std::printf("], \"cost_bits\": [%llu, %llu]}\n", Bits(cost[0]), Bits(cost[1]));

    // a camera short of observations and rounds out of range are refused, poses and points left as given; a problem
    // whose cameras are all held is structure-only refinement: it succeeds and keeps every pose
    std::vector<std::array<double, 12>> p2 = given_poses;
    std::vector<std::array<float, 3>> x2 = given_points;
    std::vector<std::vector<Vec2>> short_obs(obs.begin(), obs.end() - 1);
    const bool wrong_size = verifier.BundleAdjust(p2, x2, short_obs, cam, inlier);
    GeometricVerifier::BundleOptions saved = o;
    o.kRounds = 17;
    const bool bad_rounds = verifier.BundleAdjust(p2, x2, obs, cam, inlier);
    o = saved;
    const bool kept = p2 == given_poses && x2 == given_points;
    const std::vector<uint8_t> all(cams, 1);
    const bool held_ok = verifier.BundleAdjust(p2, x2, obs, cam, inlier, nullptr, nullptr, &all);
    std::printf("{\"test\": \"ba_false_cases\", \"wrong_size\": %s, \"bad_rounds\": %s, \"kept\": %s, \"held_ok\": %s, \"held_poses_kept\": %s}\n",
                wrong_size ? "true" : "false", bad_rounds ? "true" : "false", kept ? "true" : "false", held_ok ? "true" : "false",
                p2 == given_poses ? "true" : "false");
    return 0;
}
