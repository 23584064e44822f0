// Headless demo of LineDescriptor (an MI355X extension; the reference's line path stops at the segments):
// FeatureLineDetector's segments of a frame described with the default options, then with 3 bands of 5 rows.
// Prints JSON lines and writes, per run, the lines, descriptors, midpoints (float32) and valid flags as raw
// bytes to <out prefix>.<test>.{lines,desc,xy,valid}.
//   usage: fd_demo_line_desc <raw u8 gray file> <rows> <cols> <out prefix>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "demo_util.h"
#include "feature_detector/feature_line_detector.h"
#include "feature_detector/line_descriptor.h"

using namespace feature_detector;

template <typename T>
static std::vector<uint8_t> Raw(const T *p, size_t n) {
    const uint8_t *b = reinterpret_cast<const uint8_t *>(p);
    return std::vector<uint8_t>(b, b + n * sizeof(T));
}

static void Run(LineDescriptor &ld, const char *test, const GrayImage &image, const std::vector<Vec4> &lines,
                const std::string &prefix) {
    std::vector<float> desc(3, -1.0f);
    const bool ok = ld.Compute(image, lines, desc);
    std::printf("{\"test\": \"%s\", \"ok\": %s, \"bands\": %d, \"band_width\": %d, \"dim\": %d, \"lines\": %zu, \"floats\": %zu, "
                "\"untouched\": %s, ",
                test, ok ? "true" : "false", ld.options().kBands, ld.options().kBandWidth, ld.dim(), lines.size(), desc.size(),
                desc == std::vector<float>(3, -1.0f) ? "true" : "false");
    PrintError(ok ? std::string() : ld.last_error());
    std::printf("}\n");
    if (!ok) return;
    std::vector<float> flat, xy;
    for (const Vec4 &l : lines)
        for (int j = 0; j < 4; ++j) flat.push_back(l[j]);
    for (const Vec2 &m : ld.midpoints()) {
        xy.push_back(m.x());
        xy.push_back(m.y());
    }
    const std::string base = prefix + "." + test;
    WriteBytes(base + ".lines", Raw(flat.data(), flat.size()));
    WriteBytes(base + ".desc", Raw(desc.data(), desc.size()));
    WriteBytes(base + ".xy", Raw(xy.data(), xy.size()));
    WriteBytes(base + ".valid", ld.valid());
}

int main(int argc, char **argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: %s <raw u8 file> <rows> <cols> <out prefix>\n", argv[0]);
        return 2;
    }
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);
    GrayImage image(ReadFrame(argv[1], rows, cols), rows, cols, true);
    const std::string prefix = argv[4];

    FeatureLineDetector detector;
    std::vector<Vec4> lines;
    const bool detected = detector.DetectGoodFeatures(image, 200, lines);
    std::printf("{\"test\": \"detect\", \"ok\": %s, \"lines\": %zu}\n", detected ? "true" : "false", lines.size());
    if (!detected) {  // (no GPU: the descriptor is still asked, on lines of its own)
        lines.assign(1, Vec4(10.0f, 10.0f, 40.0f, 25.0f));
        lines.push_back(Vec4(5.5f, 30.25f, 5.5f, 12.0f));
    }
    lines.push_back(Vec4(20.0f, 20.0f, 20.25f, 20.0f));  // shorter than a pixel: no descriptor

    LineDescriptor ld;
    Run(ld, "default", image, lines, prefix);
    ld.options().kBands = 3;
    ld.options().kBandWidth = 5;
    Run(ld, "narrow", image, lines, prefix);

    // Compute's false cases: an empty image, options out of range; descriptors stay as they were
    std::vector<float> desc(3, -1.0f);
    GrayImage empty;
    const bool no_image = ld.Compute(empty, lines, desc);
    ld.options().kBands = 33;
    const bool bad_bands = ld.Compute(image, lines, desc);
    ld.options().kBands = 9;
    ld.options().kBandWidth = 0;
    const bool bad_width = ld.Compute(image, lines, desc);
    std::printf("{\"test\": \"compute_false_cases\", \"no_image\": %s, \"bad_bands\": %s, \"bad_width\": %s, \"untouched\": %s, ",
                no_image ? "true" : "false", bad_bands ? "true" : "false", bad_width ? "true" : "false",
                desc == std::vector<float>(3, -1.0f) ? "true" : "false");
    PrintError(ld.last_error());
    std::printf("}\n");
    return 0;
}
