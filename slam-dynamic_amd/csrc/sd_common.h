// Internal helpers shared by the translation units of libsd_frontend.so (sd_api.hip: front end + tracker; sd_yolo_api.hip: detector):
// the thread-local error text behind sd_last_error(), the two return-on-error macros, the owning device buffer and the dynamic-LDS limit.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include "sd_frontend.h"

int sd_set_err(int code, const std::string& msg);        // defined in sd_api.hip
#define set_err sd_set_err

// Raises the dynamic-LDS limit of `kernel` on the current device to `bytes`: nothing to do at or below the 64 KB default, and the limit only
// ever grows (workspaces and detectors of different sizes share the kernels).  Defined in sd_api.hip.
hipError_t sd_raise_lds_limit(const void* kernel, int bytes);
#define SD_LDS_MAX_BYTES (160 * 1024)      // LDS of one gfx950 workgroup: above it a per-key-point table goes to device memory

// Device memory owned by one object: hipFree on destruction, move-only.  The untyped owner, so that buffers of different element types can
// be listed together (sd_grow in sd_api.hip).
class SdDevMem {
public:
    SdDevMem() = default;
    SdDevMem(SdDevMem&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }        // declaring the moves deletes the copies
    SdDevMem& operator=(SdDevMem&& o) noexcept { if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; } return *this; }
    ~SdDevMem() { reset(); }
    // frees what the buffer held, then allocates `bytes`; on failure the buffer stays empty
    hipError_t alloc(size_t bytes) { reset(); void* p = nullptr; hipError_t e = hipMalloc(&p, bytes); if (e == hipSuccess) p_ = p; return e; }
    void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; }
protected:
    void* p_ = nullptr;
};

// SdDevMem read as a plain T* wherever a pointer is expected.
template <typename T>
class SdDevBuf : public SdDevMem {
public:
    T* get() const { return (T*)p_; }
    operator T*() const { return (T*)p_; }
};

#define HIPCHK(call)                                                                                      \
    do {                                                                                                  \
        hipError_t e_ = (call);                                                                           \
        if (e_ != hipSuccess)                                                                             \
            return set_err(e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice ? SD_ERR_NO_DEVICE : SD_ERR_HIP, \
                           std::string(#call) + ": " + hipGetErrorString(e_));                            \
    } while (0)

static inline int sd_check_launch(const char* name)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(SD_ERR_HIP, std::string(name) + " launch: " + hipGetErrorString(e));
    return SD_OK;
}
#define LAUNCH_CHECK(name) do { int rc_ = sd_check_launch(name); if (rc_ != SD_OK) return rc_; } while (0)
