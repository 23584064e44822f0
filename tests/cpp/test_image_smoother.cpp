// Headless demo of ImageSmoother (an MI355X extension; the reference has no smoothing): a frame smoothed with
// the default options (sigma 2, the radius chosen), with ORB's 7 x 7 kernel (sigma 2, radius 3), and with
// pyrDown's taps {96, 64, 16} at step 2.
// Prints JSON lines and writes each smoothed frame as raw bytes to <out prefix>.<test>.u8.
//   usage: fd_demo_blur <raw u8 gray file> <rows> <cols> <out prefix>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "demo_util.h"
#include "feature_detector/image_smoother.h"

using namespace feature_detector;

static void Run(ImageSmoother &sm, const char *test, const GrayImage &src, const std::string &prefix) {
    const ImageSmoother::Options &o = sm.options();
    const int step = o.kStep == 2 ? 2 : 1;
    const int rows = (src.rows() + step - 1) / step, cols = (src.cols() + step - 1) / step;
    std::vector<uint8_t> out(static_cast<size_t>(rows) * cols, 0xA5);
    GrayImage dst(out.data(), rows, cols);
    const bool ok = sm.Smooth(src, dst);
    std::printf("{\"test\": \"%s\", \"ok\": %s, \"sigma_bits\": %u, \"radius\": %d, \"step\": %d, \"rows\": %d, \"cols\": %d, \"taps\": [",
                test, ok ? "true" : "false", Bits(o.kSigma), o.kRadius, o.kStep, rows, cols);
    if (ok)
        for (size_t k = 0; k < sm.taps().size(); ++k) std::printf("%s%d", k ? ", " : "", sm.taps()[k]);
    std::printf("], \"untouched\": %s, ", out == std::vector<uint8_t>(out.size(), 0xA5) ? "true" : "false");
    PrintError(ok ? std::string() : sm.last_error());
    std::printf("}\n");
    if (ok) WriteBytes(prefix + "." + test + ".u8", out);
}

int main(int argc, char **argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: %s <raw u8 file> <rows> <cols> <out prefix>\n", argv[0]);
        return 2;
    }
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);
    GrayImage image(ReadFrame(argv[1], rows, cols), rows, cols, true);
    const std::string prefix = argv[4];

    ImageSmoother sm;
    Run(sm, "default", image, prefix);
    sm.options().kRadius = 3;
    Run(sm, "orb", image, prefix);
    sm.options().kTaps = {96, 64, 16};
    sm.options().kStep = 2;
    Run(sm, "pyr_down", image, prefix);

    // Smooth's false cases: an empty image, a shape mismatch, a shared buffer, options out of range; dst stays
    sm.options() = ImageSmoother::Options();
    std::vector<uint8_t> out(static_cast<size_t>(rows) * cols, 0xA5);
    GrayImage dst(out.data(), rows, cols), empty, narrower(out.data(), rows, cols - 1);
    const bool no_image = sm.Smooth(empty, dst);
    const bool mismatch = sm.Smooth(image, narrower);
    GrayImage alias(image.data(), rows, cols);
    const bool in_place = sm.Smooth(image, alias);
    sm.options().kSigma = 0.0f;
    const bool bad_sigma = sm.Smooth(image, dst);
    sm.options().kSigma = 2.0f;
    sm.options().kStep = 3;
    const bool bad_step = sm.Smooth(image, dst);
    sm.options().kStep = 1;
    sm.options().kTaps = {96, 64, 17};
    const bool bad_taps = sm.Smooth(image, dst);
    bool untouched = true;
    for (uint8_t v : out) untouched = untouched && v == 0xA5;
    std::printf("{\"test\": \"blur_false_cases\", \"no_image\": %s, \"mismatch\": %s, \"in_place\": %s, \"bad_sigma\": %s, "
                "\"bad_step\": %s, \"bad_taps\": %s, \"untouched\": %s, ",
                no_image ? "true" : "false", mismatch ? "true" : "false", in_place ? "true" : "false", bad_sigma ? "true" : "false",
                bad_step ? "true" : "false", bad_taps ? "true" : "false", untouched ? "true" : "false");
    PrintError(sm.last_error());
    std::printf("}\n");
    return 0;
}
