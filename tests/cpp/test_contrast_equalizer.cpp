// Headless demo of ContrastEqualizer (an MI355X extension; the reference has no equalization): a frame
// equalized with the default options into a second buffer, then in place with 5 x 3 tiles and clip limit 2.5.
// Prints JSON lines and writes each equalized frame as raw bytes to <out prefix>.<test>.u8.
//   usage: fd_demo_equalize <raw u8 gray file> <rows> <cols> <out prefix>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "demo_util.h"
#include "feature_detector/contrast_equalizer.h"

using namespace feature_detector;

static void Run(ContrastEqualizer &eq, const char *test, const GrayImage &src, bool in_place, const std::string &prefix) {
    const size_t n = static_cast<size_t>(src.rows()) * src.cols();
    const std::vector<uint8_t> before(src.data(), src.data() + n);
    std::vector<uint8_t> out(in_place ? before : std::vector<uint8_t>(n, 0xA5));
    GrayImage dst(out.data(), src.rows(), src.cols());
    const GrayImage &from = in_place ? static_cast<const GrayImage &>(dst) : src;
    const bool ok = eq.Equalize(from, dst);
    const ContrastEqualizer::Options &o = eq.options();
    std::printf("{\"test\": \"%s\", \"ok\": %s, \"tiles_x\": %d, \"tiles_y\": %d, \"clip_limit_bits\": %u, \"untouched\": %s, ", test,
                ok ? "true" : "false", o.kTilesX, o.kTilesY, Bits(o.kClipLimit),
                out == (in_place ? before : std::vector<uint8_t>(n, 0xA5)) ? "true" : "false");
    PrintError(ok ? std::string() : eq.last_error());
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

    ContrastEqualizer eq;
    Run(eq, "default", image, false, prefix);
    eq.options().kTilesX = 5;
    eq.options().kTilesY = 3;
    eq.options().kClipLimit = 2.5f;
    Run(eq, "in_place", image, true, prefix);

    // Equalize's false cases: an empty image, a shape mismatch, options out of range; dst stays as it was
    std::vector<uint8_t> out(static_cast<size_t>(rows) * cols, 0xA5);
    GrayImage dst(out.data(), rows, cols), empty, narrower(out.data(), rows, cols - 1);
    const bool no_image = eq.Equalize(empty, dst);
    const bool mismatch = eq.Equalize(image, narrower);
    eq.options().kClipLimit = -1.0f;
    const bool bad_clip = eq.Equalize(image, dst);
    eq.options().kClipLimit = 3.0f;
    eq.options().kTilesX = 33;
    const bool bad_tiles = eq.Equalize(image, dst);
    bool untouched = true;
    for (uint8_t v : out) untouched = untouched && v == 0xA5;
    std::printf("{\"test\": \"equalize_false_cases\", \"no_image\": %s, \"mismatch\": %s, \"bad_clip\": %s, \"bad_tiles\": %s, "
                "\"untouched\": %s, ",
                no_image ? "true" : "false", mismatch ? "true" : "false", bad_clip ? "true" : "false", bad_tiles ? "true" : "false",
                untouched ? "true" : "false");
    PrintError(eq.last_error());
    std::printf("}\n");
    return 0;
}
