// What the nine drop-in classes do with their device context (set_device / device() / last_error() and the
// "[feature_detector]" lines on stderr), for tests/test_cpp_device.py. Uses the public headers only.
//   fd_demo_device        each class's main entry once on the smallest valid input (a 16 x 16 frame); one
//                         JSON line per class: the return value, last_error(), and device() before the
//                         call, after it and after set_device(3)
//   fd_demo_device gpu    ImageWarper and CornerRefiner across set_device calls on a working GPU
//   fd_demo_device time   ImageWarper::Warp and CornerRefiner::Refine on a 240 x 320 frame: 5 warm calls,
//                         then 40 timed ones; median, minimum and p90 in microseconds
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "demo_util.h"
#include "feature_detector/corner_refiner.h"
#include "feature_detector/descriptor_brief.h"
#include "feature_detector/descriptor_matcher.h"
#include "feature_detector/feature_line_detector.h"
#include "feature_detector/feature_point_detector.h"
#include "feature_detector/geometric_verifier.h"
#include "feature_detector/image_warper.h"
#include "feature_detector/optical_flow_lk.h"

using namespace feature_detector;

namespace {

const double kIdentity[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};

// a frame with gradients in both directions everywhere
std::vector<uint8_t> Frame(int rows, int cols) {
    std::vector<uint8_t> f(static_cast<size_t>(rows) * cols);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) f[static_cast<size_t>(r) * cols + c] = static_cast<uint8_t>((r * 37 + c * 11 + (r / 4) * (c / 4) * 29) & 255);
    return f;
}

void PrintLine(const char *test, bool ok, const std::string &error, const std::vector<int> &device) {
    std::printf("{\"test\": \"%s\", \"ok\": %s, ", test, ok ? "true" : "false");
    PrintError(error);
    if (!device.empty()) std::printf(", \"device\": [%d, %d, %d]", device[0], device[1], device[2]);
    std::printf("}\n");
}

// call() between device() before and after, then set_device(3)
template <typename T, typename Call>
void Pin(const char *test, T &object, Call call) {
    std::vector<int> device{object.device()};
    const bool ok = call();
    device.push_back(object.device());
    object.set_device(3);
    device.push_back(object.device());
    PrintLine(test, ok, object.last_error(), device);
}

int PinAll() {
    std::vector<uint8_t> bytes = Frame(16, 16), other = Frame(16, 16);
    GrayImage image(bytes.data(), 16, 16), image1(other.data(), 16, 16);
    const std::vector<Vec2> points{Vec2(5, 5), Vec2(8, 9), Vec2(10, 6), Vec2(6, 10)};
    std::vector<uint8_t> status;

    FeaturePointHarrisDetector harris;
    std::vector<Vec2> features;
    Pin("harris", harris, [&] { return harris.DetectGoodFeatures(image, 4, features); });

    FeatureLineDetector lines;
    std::vector<Vec4> segments;
    const bool ok_lines = lines.DetectGoodFeatures(image, 4, segments);
    lines.set_device(3);
    PrintLine("lines", ok_lines, lines.last_error(), {});

    BriefDescriptor brief;
    brief.options().kLength = 32;
    std::vector<BriefType> descriptors;
    Pin("brief", brief, [&] { return brief.Compute(image, points, descriptors); });

    const std::vector<BriefType> bits{BriefType(32, false), BriefType(32, true)};
    std::vector<int32_t> index;
    BriefMatcher brief_matcher;
    Pin("brief_match", brief_matcher, [&] { return brief_matcher.Match(bits, bits, index); });

    const float rows[8] = {1, 0, 0, 0, 0, 1, 0, 0};
    NNDescriptorMatcher nn_matcher;
    Pin("nn_match", nn_matcher, [&] { return nn_matcher.Match(rows, 2, rows, 2, 4, index); });

    OpticalFlowLK flow;
    flow.options().kLevels = 1;
    flow.options().kHalfWindow = 2;
    std::vector<Vec2> tracked;
    Pin("flow", flow, [&] { return flow.Track(image, image1, points, tracked, status); });

    CornerRefiner refiner;
    refiner.options().kHalfWindow = 2;
    std::vector<Vec2> refined = points;
    Pin("refine", refiner, [&] { return refiner.Refine(image, refined, status); });

    GeometricVerifier verifier;
    verifier.options().kModel = GeometricVerifier::kHomography;
    Pin("verify", verifier, [&] { return verifier.Verify(points, points, status); });

    ImageWarper warper;
    std::vector<uint8_t> out(bytes.size(), 0xA5);
    GrayImage dst(out.data(), 16, 16);
    Pin("warp", warper, [&] { return warper.Warp(image, kIdentity, dst); });
    return 0;
}

// One warper and one refiner taken through set_device: the same device, a device fd_ctx_create rejects
// by its range check, and back to the default.
int Gpu() {
    std::vector<uint8_t> bytes = Frame(16, 16);
    GrayImage image(bytes.data(), 16, 16);
    ImageWarper warper;
    CornerRefiner refiner;
    const struct { const char *test; int device; bool set; } steps[] = {
        {"first", 0, false}, {"same_device", 0, true}, {"bad_device", 1 << 20, true}, {"default_device", -1, true}};
    for (const auto &s : steps) {
        if (s.set) {
            warper.set_device(s.device);
            refiner.set_device(s.device);
        }
        std::vector<uint8_t> out(bytes.size(), 0xA5);
        GrayImage dst(out.data(), 16, 16);
        const bool ok = warper.Warp(image, kIdentity, dst);
        std::vector<Vec2> uv{Vec2(8, 8)};
        std::vector<uint8_t> status;
        const bool ok_r = refiner.Refine(image, uv, status);
        std::printf("{\"test\": \"%s.warp\", \"ok\": %s, \"equals_source\": %s, \"untouched\": %s, \"device\": %d, ", s.test,
                    ok ? "true" : "false", out == bytes ? "true" : "false",
                    out == std::vector<uint8_t>(bytes.size(), 0xA5) ? "true" : "false", warper.device());
        PrintError(ok ? std::string() : warper.last_error());
        std::printf("}\n{\"test\": \"%s.refine\", \"ok\": %s, \"status\": %d, \"xy_bits\": [%u, %u], ", s.test,
                    ok_r ? "true" : "false", status.empty() ? -1 : status[0], Bits(uv[0].x()), Bits(uv[0].y()));
        PrintError(ok_r ? std::string() : refiner.last_error());
        std::printf("}\n");
    }
    return 0;
}

template <typename Call>
void TimeRow(const char *test, Call call) {
    for (int i = 0; i < 5; ++i) call();
    std::vector<double> us;
    bool ok = true;
    for (int i = 0; i < 40; ++i) {
        const auto t0 = std::chrono::steady_clock::now();
        ok = call() && ok;
        us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(us.begin(), us.end());
    std::printf("{\"test\": \"%s\", \"ok\": %s, \"calls\": 40, \"median_us\": %.1f, \"min_us\": %.1f, \"p90_us\": %.1f}\n", test,
                ok ? "true" : "false", 0.5 * (us[19] + us[20]), us[0], us[35]);
}

int Time() {
    std::vector<uint8_t> bytes = Frame(240, 320), out(bytes.size());
    GrayImage image(bytes.data(), 240, 320), dst(out.data(), 240, 320);
    ImageWarper warper;
    TimeRow("warp", [&] { return warper.Warp(image, kIdentity, dst); });
    CornerRefiner refiner;
    std::vector<Vec2> grid;
    for (int r = 20; r < 240; r += 20)
        for (int c = 20; c < 320; c += 20) grid.emplace_back(Vec2(static_cast<float>(c), static_cast<float>(r)));
    std::vector<uint8_t> status;
    TimeRow("refine", [&] {
        std::vector<Vec2> uv = grid;
        return refiner.Refine(image, uv, status);
    });
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) return PinAll();
    if (!std::strcmp(argv[1], "gpu")) return Gpu();
    if (!std::strcmp(argv[1], "time")) return Time();
    std::fprintf(stderr, "usage: %s [gpu | time]\n", argv[0]);
    return 2;
}
