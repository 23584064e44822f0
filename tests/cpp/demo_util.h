// What the headless demos of this directory share: reading a raw frame, writing raw bytes, and printing
// floats as bit patterns and error strings as JSON.
#ifndef FEATURE_DETECTOR_TESTS_DEMO_UTIL_H_
#define FEATURE_DETECTOR_TESTS_DEMO_UTIL_H_

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

// rows x cols bytes of `path` in a malloc'ed buffer (for an owning GrayImage); exits with 2 if it cannot
static inline uint8_t *ReadFrame(const char *path, int rows, int cols) {
    const size_t n = static_cast<size_t>(rows) * cols;
    uint8_t *buf = static_cast<uint8_t *>(std::malloc(n));
    FILE *f = std::fopen(path, "rb");
    if (!f || std::fread(buf, 1, n, f) != n) {
        std::fprintf(stderr, "cannot read %s\n", path);
        std::exit(2);
    }
    std::fclose(f);
    return buf;
}

static inline void WriteBytes(const std::string &path, const std::vector<uint8_t> &v) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(v.data(), 1, v.size(), f) != v.size()) {
        std::fprintf(stderr, "cannot write %s\n", path.c_str());
        std::exit(2);
    }
    std::fclose(f);
}

static inline unsigned Bits(float v) {
    unsigned u;
    std::memcpy(&u, &v, sizeof(u));
    return u;
}

static inline unsigned long long Bits(double v) {
    unsigned long long u;
    std::memcpy(&u, &v, sizeof(u));
    return u;
}

// "error": "<e>", with the characters JSON would need escaped replaced by spaces
static inline void PrintError(const std::string &e) {
    std::printf("\"error\": \"");
    for (char ch : e) std::putchar(ch == '"' || ch == '\\' || static_cast<unsigned char>(ch) < 32 ? ' ' : ch);
    std::printf("\"");
}

#endif  // FEATURE_DETECTOR_TESTS_DEMO_UTIL_H_
