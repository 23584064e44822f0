// Headless demo of ImageWarper (an MI355X extension; the reference has no warp): a frame warped by a fixed
// homography and by a fixed camera model. Prints JSON lines (the parameters as the bit patterns of their
// doubles) and writes each warped frame and its mask as raw bytes to <out prefix>.<test>.u8 / .mask.
//   usage: fd_demo_warp <raw u8 gray file> <rows> <cols> <out rows> <out cols> <out prefix>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "demo_util.h"
#include "feature_detector/image_warper.h"

using namespace feature_detector;

static void Run(ImageWarper &warper, const char *test, const GrayImage &src, const std::vector<double> &params, int out_rows,
                int out_cols, const std::string &prefix) {
    const size_t n = static_cast<size_t>(out_rows) * out_cols;
    std::vector<uint8_t> out(n, 0xA5), mask(n, 0xA5);
    GrayImage dst(out.data(), out_rows, out_cols);
    const bool ok = warper.Warp(src, params.data(), dst, mask.data());
    std::printf("{\"test\": \"%s\", \"ok\": %s, \"params_bits\": [", test, ok ? "true" : "false");
    for (size_t i = 0; i < params.size(); ++i) std::printf("%s%llu", i ? ", " : "", Bits(params[i]));
    std::printf("], \"untouched\": %s, ", out[0] == 0xA5 && out[n - 1] == 0xA5 && mask[n / 2] == 0xA5 ? "true" : "false");
    PrintError(ok ? std::string() : warper.last_error());
    std::printf("}\n");
    if (ok) {
        WriteBytes(prefix + "." + test + ".u8", out);
        WriteBytes(prefix + "." + test + ".mask", mask);
    }
}

int main(int argc, char **argv) {
    if (argc < 7) {
        std::fprintf(stderr, "usage: %s <raw u8 file> <rows> <cols> <out rows> <out cols> <out prefix>\n", argv[0]);
        return 2;
    }
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), out_rows = std::atoi(argv[4]), out_cols = std::atoi(argv[5]);
    GrayImage image(ReadFrame(argv[1], rows, cols), rows, cols, true);
    const std::string prefix = argv[6];

    ImageWarper warper;
    warper.options().kFill = 200;
    // a rotation by 7 degrees with scale 1.1 about (cols / 2, rows / 2) and a mild perspective
    const double c = 1.1 * std::cos(7.0 * M_PI / 180.0), s = 1.1 * std::sin(7.0 * M_PI / 180.0);
    const double cx = cols / 2.0, cy = rows / 2.0;
    const std::vector<double> h{c, -s, cx - (c * cx - s * cy), s, c, cy - (s * cx + c * cy), 1e-4, -2e-4, 1.0};
    Run(warper, "homography", image, h, out_rows, out_cols, prefix);

    warper.options().kModel = ImageWarper::kCamera;
    const double f = 0.9 * cols;
    const double fn = 0.7 * cols;  // a wider destination view: its corners have no source
    const std::vector<double> cam{fn, fn, out_cols / 2.0, out_rows / 2.0, 1, 0, 0, 0, 1, 0, 0, 0, 1, f * 1.02, f * 0.98, cx + 1.5,
                                  cy - 2.25, -0.28, 0.09, 0.001, -0.002, 0.01};
    Run(warper, "camera", image, cam, out_rows, out_cols, prefix);

    // Warp's false cases: no parameters, the source as its own destination, an option out of range
    std::vector<uint8_t> out(static_cast<size_t>(out_rows) * out_cols);
    GrayImage dst(out.data(), out_rows, out_cols);
    const bool no_params = warper.Warp(image, nullptr, dst);
    GrayImage alias(image.data(), rows, cols);
    const bool aliased = warper.Warp(image, cam.data(), alias);
    warper.options().kFill = 256;
    const bool bad_option = warper.Warp(image, cam.data(), dst);
    std::printf("{\"test\": \"warp_false_cases\", \"no_params\": %s, \"aliased\": %s, \"bad_option\": %s, ",
                no_params ? "true" : "false", aliased ? "true" : "false", bad_option ? "true" : "false");
    PrintError(warper.last_error());
    std::printf("}\n");
    return 0;
}
