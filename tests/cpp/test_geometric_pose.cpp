// Headless demo of GeometricVerifier::RecoverPose and ::Triangulate (MI355X extensions; the reference has no such
// stage): the correspondences of a file (point i with point i), a fundamental matrix and an inlier mask turned
// into the relative pose and the inliers' 3-D points, then the points once more from that pose.
// Prints JSON lines; doubles and floats as the decimal bit patterns of their 64 / 32 bits.
//   usage: fd_demo_pose <raw float32 file of n x 4: qx qy tx ty> <n> <raw float64 file of 9: F> <raw uint8 file of n: inliers>
//                       <fx fy cx cy of the query camera> <fx fy cx cy of the train camera> <max_depth> <min_parallax>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "demo_util.h"
#include "feature_detector/geometric_verifier.h"

using namespace feature_detector;

template <typename T>
static bool ReadAll(const char *path, std::vector<T> &v) {
    FILE *f = std::fopen(path, "rb");
    const bool ok = f && std::fread(v.data(), sizeof(T), v.size(), f) == v.size();
    if (f) std::fclose(f);
    if (!ok) std::fprintf(stderr, "cannot read %s\n", path);
    return ok;
}

static void Print(const char *test, bool ok, int32_t extra, const std::array<double, 12> *pose,
                  const std::vector<std::array<float, 3>> &points, const std::vector<uint8_t> &valid) {
    std::printf("{\"test\": \"%s\", \"ok\": %s, \"extra\": %d, \"pose_bits\": [", test, ok ? "true" : "false", extra);
    for (size_t i = 0; pose && i < 12; ++i) std::printf("%s%llu", i ? ", " : "", Bits((*pose)[i]));
    std::printf("], \"valid\": [");
    for (size_t i = 0; i < valid.size(); ++i) std::printf("%s%d", i ? ", " : "", valid[i]);
    std::printf("], \"point_bits\": [");
    for (size_t i = 0; i < points.size(); ++i)
        std::printf("%s%u, %u, %u", i ? ", " : "", Bits(points[i][0]), Bits(points[i][1]), Bits(points[i][2]));
    std::printf("]}\n");
}

int main(int argc, char **argv) {
    if (argc < 15) {
        std::fprintf(stderr, "usage: %s <pairs.f32> <n> <model.f64> <inliers.u8> <4 x query camera> <4 x train camera> <max_depth> "
                             "<min_parallax>\n", argv[0]);
        return 2;
    }
    const size_t n = static_cast<size_t>(std::atoi(argv[2]));
    std::vector<float> raw(4 * n);
    std::vector<double> f9(9);
    std::vector<uint8_t> inlier(n);
    if (!ReadAll(argv[1], raw) || !ReadAll(argv[3], f9) || !ReadAll(argv[4], inlier)) return 2;
    std::vector<Vec2> query(n), train(n);
    for (size_t i = 0; i < n; ++i) {
        query[i] = Vec2(raw[4 * i], raw[4 * i + 1]);
        train[i] = Vec2(raw[4 * i + 2], raw[4 * i + 3]);
    }
    std::array<double, 9> model;
    for (size_t i = 0; i < 9; ++i) model[i] = f9[i];
    GeometricVerifier::Camera cq{std::atof(argv[5]), std::atof(argv[6]), std::atof(argv[7]), std::atof(argv[8])};
    GeometricVerifier::Camera ct{std::atof(argv[9]), std::atof(argv[10]), std::atof(argv[11]), std::atof(argv[12])};

    GeometricVerifier verifier;
    verifier.pose_options().kMaxDepth = static_cast<float>(std::atof(argv[13]));
    verifier.pose_options().kMinParallax = static_cast<float>(std::atof(argv[14]));

    std::array<double, 12> pose;
    std::vector<std::array<float, 3>> points;
    std::vector<uint8_t> valid;
    int32_t choice = 7, count = -1;
    bool ok = verifier.RecoverPose(query, train, inlier, model, cq, ct, pose, points, valid, nullptr, nullptr, &choice);
    Print("recover", ok, choice, &pose, points, valid);
    ok = verifier.Triangulate(query, train, pose, cq, ct, points, valid, &inlier, nullptr, nullptr, &count);
    Print("triangulate", ok, count, nullptr, points, valid);

    // a zero model has no pose; a wrong size and a bad camera are refused
    std::array<double, 9> zero{};
    std::array<double, 12> none;
    none.fill(1.0);
    const bool no_pose = verifier.RecoverPose(query, train, inlier, zero, cq, ct, none, points, valid, nullptr, nullptr, &choice);
    bool cleared = choice == -1;
    for (double v : none) cleared = cleared && v == 0.0;
    for (uint8_t v : valid) cleared = cleared && v == 0;
    std::vector<uint8_t> short_mask(n ? n - 1 : 0);
    const bool wrong_size = verifier.RecoverPose(query, train, short_mask, model, cq, ct, none, points, valid);
    GeometricVerifier::Camera bad = cq;
    bad.fx = 0.0;
    const bool bad_camera = verifier.Triangulate(query, train, pose, bad, ct, points, valid);
    std::printf("{\"test\": \"pose_false_cases\", \"no_pose\": %s, \"cleared\": %s, \"wrong_size\": %s, \"bad_camera\": %s}\n",
                no_pose ? "true" : "false", cleared ? "true" : "false", wrong_size ? "true" : "false", bad_camera ? "true" : "false");
    return 0;
}
