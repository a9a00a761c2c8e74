// staging.hpp -- what every one-shot batch call does around its kernels: choose the device, lay the arrays out in one block
// (staging_layout.hpp), take that block from the buffer cache (buf_cache.hpp), upload, download, give the block back.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "buf_cache.hpp"
#include "common.hpp"
#include "staging_layout.hpp"

namespace qsp {

#define QSP_TRY(call)                                                                             \
    do {                                                                                          \
        const int qsp_rc_ = (call);                                                               \
        if (qsp_rc_) return qsp_rc_;                                                              \
    } while (0)

inline int use_device(int device, const char* who) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return qsp_fail(QSP_ERR_NO_DEVICE, "no HIP device");
    if (device < 0 || device >= ndev) return qsp_fail(QSP_ERR_INVALID, (std::string(who) + ": device out of range").c_str());
    QSP_HIP(hipSetDevice(device));
    return QSP_OK;
}

// a zeroed host staging buffer; false: out of host memory (no exception may leave an extern "C" function)
inline bool host_staging(std::vector<char>& v, size_t bytes) {
    try { v.assign(bytes, 0); } catch (const std::exception&) { return false; }
    return true;
}
// src (which may be null when bytes == 0) to offset `at` of a host staging buffer
inline void put(std::vector<char>& up, size_t at, const void* src, size_t bytes) { if (bytes) memcpy(up.data() + at, src, bytes); }

// One device block out of the per-device cache (hipMalloc when nothing there fits).  It goes back when the call ends, under the
// size the cache reported for it -- which may be more than was asked for -- so that the cache's byte accounting stays right.
class DeviceBlock {
  public:
    DeviceBlock() = default;
    DeviceBlock(const DeviceBlock&) = delete;
    DeviceBlock& operator=(const DeviceBlock&) = delete;
    ~DeviceBlock() { if (d_ && !buf_cache_put(g_dev_cache, device_, d_, held_, 0, kDevCacheBytes)) (void)hipFree(d_); }
    int take(int device, size_t bytes) {                         // once per block, on the current device
        device_ = device;
        held_ = bytes;
        d_ = (char*)buf_cache_take(g_dev_cache, device, bytes, 0, &held_);
        if (d_) return QSP_OK;
        const hipError_t e = hipMalloc((void**)&d_, bytes);
        if (e != hipSuccess) d_ = nullptr;
        QSP_HIP(e);
        return QSP_OK;
    }
    char* data() const { return d_; }
    int upload(const void* host, size_t n) { QSP_HIP(hipMemcpy(d_, host, n, hipMemcpyHostToDevice)); return QSP_OK; }   // -> [0, n)
    int download(void* host, size_t from, size_t n) const { QSP_HIP(hipMemcpy(host, d_ + from, n, hipMemcpyDeviceToHost)); return QSP_OK; }

  private:
    char* d_ = nullptr;
    size_t held_ = 0;
    int device_ = 0;
};

}  // namespace qsp
