// c_abi.cpp -- library-wide C-ABI entry points (version, error text, device count), the buffer cache, and the one-shot batch calls:
// the object map-point gate, Sim3 RANSAC, SearchBySim3, SearchByBoW, SearchForTriangulation, the triangulation of CreateNewMapPoints, Fuse, tracking's SearchByProjection, the ellipsoid fits, OptimizeSim3 and the essential graph.  The
// last launches the dense factorisation that ba_solver.hip defines, through dense_chol.hpp; nothing else here is the solver's.
#include <hip/hip_runtime.h>

#include "buf_cache.hpp"
#include "common.hpp"
#include "ellipsoid_fit.hpp"
#include "essential_graph.hpp"
#include "fuse.hpp"
#include "object_gate.hpp"
#include "place_db.hpp"
#include "search_bow.hpp"
#include "search_projection.hpp"
#include "search_projection_kf.hpp"
#include "search_sim3.hpp"
#include "search_triangulation.hpp"
#include "sim3_opt.hpp"
#include "sim3_ransac.hpp"
#include "triangulate.hpp"

namespace qsp {
std::string& last_error_ref() {
    static thread_local std::string e;
    return e;
}

std::mutex g_buf_cache_mu;
std::vector<CachedBuf> g_dev_cache[64], g_host_cache[64];
void* buf_cache_take(std::vector<CachedBuf>* cache, int dev, size_t bytes, unsigned flags, size_t* got) {
    std::lock_guard<std::mutex> lk(g_buf_cache_mu);
    auto& v = cache[dev & 63];
    int best = -1;
    for (int i = 0; i < (int)v.size(); ++i)
        if (v[i].flags == flags && v[i].bytes >= bytes && v[i].bytes <= 2 * bytes + (1 << 16) && (best < 0 || v[i].bytes < v[best].bytes)) best = i;
    if (best < 0) return nullptr;
    void* q = v[best].p;
    *got = v[best].bytes;
    v.erase(v.begin() + best);
    return q;
}
bool buf_cache_put(std::vector<CachedBuf>* cache, int dev, void* q, size_t bytes, unsigned flags, size_t max_total) {
    std::lock_guard<std::mutex> lk(g_buf_cache_mu);
    auto& v = cache[dev & 63];
    size_t tot = bytes;
    for (const CachedBuf& c : v) tot += c.bytes;
    if (v.size() >= 16 || tot > max_total) return false;
    v.push_back({q, bytes, flags});
    return true;
}
}  // namespace qsp

extern "C" const char* qsp_last_error(void) { return qsp::last_error_ref().c_str(); }
extern "C" int qsp_version(void) { return 1; }
extern "C" int qsp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
