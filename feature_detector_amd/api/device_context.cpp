// DeviceContext: the one owner of an fd_ctx for the drop-in classes (include/feature_detector/device_context.h).
#include "feature_detector/device_context.h"

#include <cstdio>
#include <cstdlib>

#include "fd_hip.h"

namespace feature_detector {

DeviceContext::~DeviceContext() {
    if (ctx_) fd_ctx_destroy(ctx_);
}

void DeviceContext::set_device(int device) {
    if (ctx_ && device != device_) {
        fd_ctx_destroy(ctx_);
        ctx_ = nullptr;
    }
    device_ = device;
}

int DeviceContext::DefaultDevice() {
    const char *e = std::getenv("FD_DEVICE");
    return e ? std::atoi(e) : 0;
}

fd_ctx *DeviceContext::Create() {
    if (!ctx_ && fd_ctx_create(device_ < 0 ? DefaultDevice() : device_, &ctx_) != FD_OK) {
        ctx_ = nullptr;
        error_ = "fd_ctx_create failed (no MI355X visible?)";
    }
    return ctx_;
}

fd_ctx *DeviceContext::Acquire() {
    if (!Create()) Fail(std::string(error_));
    return ctx_;
}

bool DeviceContext::Fail(const std::string &what) {
    error_ = what;
    std::fprintf(stderr, "[feature_detector] %s\n", error_.c_str());
    return false;
}

bool DeviceContext::FailCall(const std::string &call) { return Fail(call + ": " + fd_last_error(ctx_)); }

}  // namespace feature_detector
