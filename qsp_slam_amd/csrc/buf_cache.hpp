// buf_cache.hpp -- the per-device cache of freed device blocks and pinned host buffers (defined in c_abi.cpp).  hipMalloc / hipFree
// and hipHostMalloc / hipHostFree cost 0.1-0.5 ms apiece, and a caller that builds a problem per bundle adjustment or runs a one-shot
// batch call per key frame asks for the same sizes again and again.  16 entries per device and cache, kDevCacheBytes of device
// memory (the host-buffer bound is the caller's).  A taken block holds whatever its last user left.  qsp_ba_release_caches frees all.
#pragma once
#include <cstddef>
#include <mutex>
#include <vector>

namespace qsp {
struct CachedBuf { void* p; size_t bytes; unsigned flags; };
constexpr size_t kDevCacheBytes = (size_t)512 << 20;
extern std::mutex g_buf_cache_mu;
extern std::vector<CachedBuf> g_dev_cache[64], g_host_cache[64];
// best fit with bytes <= have <= 2 * bytes + 64 KiB; *got = what the buffer really holds (give THAT back); nullptr: none fits
void* buf_cache_take(std::vector<CachedBuf>* cache, int dev, size_t bytes, unsigned flags, size_t* got);
// false: the cache is full, the caller frees the buffer
bool buf_cache_put(std::vector<CachedBuf>* cache, int dev, void* q, size_t bytes, unsigned flags, size_t max_total);
}  // namespace qsp
