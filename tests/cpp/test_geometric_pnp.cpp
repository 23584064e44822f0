// Headless demo of GeometricVerifier::SolvePnP and ::RefinePnP (MI355X extensions; the reference has no such
// stage): the 3-D points and image positions of a file (point i with position i) turned into the camera pose
// and its inliers, then refined.
// Prints JSON lines; doubles as the decimal bit patterns of their 64 bits.
//   usage: fd_demo_pnp <raw float32 file of n x 5: X Y Z u v> <n> <fx fy cx cy> <hypotheses> <seed> <threshold>
//                      <center x y z> <scale> <rounds>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "demo_util.h"
#include "feature_detector/geometric_verifier.h"

using namespace feature_detector;

static void Print(const char *test, bool ok, int32_t extra, const std::array<double, 12> &pose, const std::vector<uint8_t> &inlier) {
    std::printf("{\"test\": \"%s\", \"ok\": %s, \"extra\": %d, \"pose_bits\": [", test, ok ? "true" : "false", extra);
    for (size_t i = 0; i < 12; ++i) std::printf("%s%llu", i ? ", " : "", Bits(pose[i]));
    std::printf("], \"inlier\": [");
    for (size_t i = 0; i < inlier.size(); ++i) std::printf("%s%d", i ? ", " : "", inlier[i]);
    std::printf("]}\n");
}

int main(int argc, char **argv) {
    if (argc < 15) {
        std::fprintf(stderr, "usage: %s <points.f32> <n> <fx fy cx cy> <hypotheses> <seed> <threshold> <center x y z> <scale> <rounds>\n",
                     argv[0]);
        return 2;
    }
    const size_t n = static_cast<size_t>(std::atoi(argv[2]));
    std::vector<float> raw(5 * n);
    FILE *f = std::fopen(argv[1], "rb");
    const bool read = f && std::fread(raw.data(), sizeof(float), raw.size(), f) == raw.size();
    if (f) std::fclose(f);
    if (!read) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    std::vector<std::array<float, 3>> points(n);
    std::vector<Vec2> image(n);
    for (size_t i = 0; i < n; ++i) {
        points[i] = {raw[5 * i], raw[5 * i + 1], raw[5 * i + 2]};
        image[i] = Vec2(raw[5 * i + 3], raw[5 * i + 4]);
    }
    GeometricVerifier::Camera cam{std::atof(argv[3]), std::atof(argv[4]), std::atof(argv[5]), std::atof(argv[6])};
    GeometricVerifier verifier;
    GeometricVerifier::PnpOptions &o = verifier.pnp_options();
    o.kHypotheses = std::atoi(argv[7]);
    o.kSeed = static_cast<uint32_t>(std::strtoul(argv[8], nullptr, 10));
    o.kThreshold = static_cast<float>(std::atof(argv[9]));
    o.kCenter = {std::atof(argv[10]), std::atof(argv[11]), std::atof(argv[12])};
    o.kScale = std::atof(argv[13]);
    const int32_t rounds = std::atoi(argv[14]);

    std::array<double, 12> pose;
    std::vector<uint8_t> inlier;
    int32_t best = 7, accepted = -1;
    bool ok = verifier.SolvePnP(points, image, cam, pose, inlier, nullptr, nullptr, nullptr, &best);
    Print("solve", ok, best, pose, inlier);
    ok = verifier.RefinePnP(points, image, cam, pose, inlier, rounds, nullptr, nullptr, nullptr, &accepted);
    Print("refine", ok, accepted, pose, inlier);

    // five points have no pose; a wrong size, a bad camera and rounds out of range are refused
    std::vector<std::array<float, 3>> five(points.begin(), points.begin() + (n < 5 ? n : 5));
    std::array<double, 12> none;
    none.fill(1.0);
    std::vector<uint8_t> few;
    const bool no_pose = verifier.SolvePnP(five, image, cam, none, few, nullptr, nullptr, nullptr, &best);
    bool cleared = best == -1 && few.size() == five.size();
    for (double v : none) cleared = cleared && v == 0.0;
    for (uint8_t v : few) cleared = cleared && v == 0;
    std::vector<uint8_t> short_mask(n ? n - 1 : 0);
    const bool wrong_size = verifier.SolvePnP(points, image, cam, none, few, &short_mask);
    GeometricVerifier::Camera bad = cam;
    bad.fx = 0.0;
    const bool bad_camera = verifier.SolvePnP(points, image, bad, none, few);
    std::array<double, 12> kept = pose;
    const bool bad_rounds = verifier.RefinePnP(points, image, cam, kept, inlier, 9);
    std::printf("{\"test\": \"pnp_false_cases\", \"no_pose\": %s, \"cleared\": %s, \"wrong_size\": %s, \"bad_camera\": %s, "
                "\"bad_rounds\": %s, \"kept\": %s}\n",
                no_pose ? "true" : "false", cleared ? "true" : "false", wrong_size ? "true" : "false", bad_camera ? "true" : "false",
                bad_rounds ? "true" : "false", kept == pose ? "true" : "false");
    return 0;
}
