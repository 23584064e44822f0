// DeviceContext: what every drop-in class keeps of libfdhip.so between calls -- the fd_ctx, created on first
// use, the GPU ordinal it belongs to and the message of the last failure. Each class holds one as a member and
// forwards its set_device() / device() / last_error() here.
#ifndef FEATURE_DETECTOR_DEVICE_CONTEXT_H_
#define FEATURE_DETECTOR_DEVICE_CONTEXT_H_

#include <string>

struct fd_ctx;

namespace feature_detector {

class DeviceContext {
public:
    DeviceContext() = default;
    ~DeviceContext();
    DeviceContext(const DeviceContext &) = delete;
    DeviceContext &operator=(const DeviceContext &) = delete;

    // The GPU ordinal of the next Acquire(); < 0 (the default): DefaultDevice(). A context of another
    // ordinal is destroyed.
    void set_device(int device);
    int device() const { return device_; }
    const std::string &last_error() const { return error_; }

    // $FD_DEVICE, or 0
    static int DefaultDevice();

    // The context, null before the first Acquire() / Create() and after a set_device() that dropped it.
    fd_ctx *get() const { return ctx_; }
    // The context, created on first use. Null if it cannot be created; Acquire() reports that as Fail()
    // does, Create() only leaves it in last_error().
    fd_ctx *Acquire();
    fd_ctx *Create();

    // Stores `what` as last_error(), prints it to stderr as "[feature_detector] <what>", returns false.
    bool Fail(const std::string &what);
    // Fail("<call>: <fd_last_error of the context>")
    bool FailCall(const std::string &call);

private:
    fd_ctx *ctx_ = nullptr;
    int device_ = -1;
    std::string error_;
};

}  // namespace feature_detector

#endif  // FEATURE_DETECTOR_DEVICE_CONTEXT_H_
