// Device-side mesh extraction: SDF volume on the reference's voxel grid (reconstruct/utils.py:98-117) decoded with the MLP
// tile kernel, then marching cubes on the GPU (replaces skimage.measure.marching_cubes_lewiner called from
// reconstruct/utils.py:120-141; MeshExtractor.extract_mesh_from_code, reconstruct/optimizer.py:284-304).
// Included at the end of sdf_refine.hip (same translation unit: it decodes with launch_grid_decode and reads qsp_decoder).
//
// Marching cubes: method 0 (default, round 4) is Lewiner's, exactly as scikit-image's marching_cubes_lewiner runs it -- mesh_lewiner.hpp,
// pinned by scikit-image's own output.  Method 1 is the triangulation rounds 2-3 shipped when the dependency had not been found in the
// image, generated from first principles:
//   * a vertex on every grid edge whose end points differ in sign (inside = sdf < 0), at the linear zero crossing --
//     the same vertex set every marching-cubes variant has, shared between the cells around the edge;
//   * per cell, each cube face with 2 crossings contributes one segment, a face with 4 (ambiguous) two segments that
//     cut off its inside corners separately -- a rule that depends on the face's own corner signs only, so neighbouring
//     cells always agree and the surface is watertight; the segments close into loops, each loop is oriented so that
//     the right-hand normal points to increasing sdf (outwards) and fan-triangulated from the first vertex whose fan has
//     no diagonal inside a cube face (such a fan exists for every loop of every case).
// Where Lewiner differs from method 1: the diagonals inside a cell's polygons, interior ambiguity tests and the extra centre vertex
// of a few of the 33 cases, face order, vertex order.  Both share the scan kernels and the buffers of this file.
//
// One launch chain runs every call.  A call is n codes or volumes -> n meshes in passes of at most `limit` volumes
// (QSP_MESH_BATCH_LIMIT_DEFAULT = 64; qsp_mesh_extractor_set_batch_limit lowers it); the single calls (qsp_mesh_extract /
// qsp_mesh_from_volume) are n = 1, the batch calls (qsp_mesh_extract_batch / qsp_mesh_from_volumes; method 0 only) any n, with the
// launches and the synchronisations of one mesh per pass instead of per mesh.  A pass (mesh_pass) runs
//   k_grid_decode* (one launch, every code of the pass; sdf_kernels.hpp) -> k_lew_count -> k_mc_scan_blocks over all volumes'
//   scan blocks -> k_mc_scan_top_batch (one workgroup per volume) -> k_mc_scan_top over the volumes' totals -> [the host reads the
//   pass's totals: the one synchronisation that sizes the outputs] -> k_lew_verts -> k_lew_faces,
// plain launches in stream order; with method 1, k_mc_flags and k_mc_emit in the places of the k_lew_* kernels.  Every volume of a
// pass owns n_pad = whole scan blocks of the count array, so the scan restarts with each volume and a mesh is numbered from 0;
// where its vertices and faces go in the call's concatenated arrays is the device-side scan of the totals plus what the passes
// before produced.
// Buffers: the scratch of a pass -- 20 bytes per padded grid point and volume (64-bit counts, three int32 maps): 42 MB for 64
// volumes of 32^3, 336 MB at 64^3, 2.7 GB at 128^3 -- exists once and every call uses it: nothing in it is read after the call
// returns.  What a fetch reads (the decoded or uploaded volumes, 4 bytes per point, the meshes, the counts) exists twice, `single`
// and `batch`: qsp_mesh_fetch / _fetch_f64 always give the last SINGLE call's mesh, qsp_mesh_fetch_batch the last batch call's,
// whatever was called in between.  All of it grows to the high-water mark (mesh_reserve) and is freed with the extractor.  A
// result does not depend on the pass size.  A call that fails leaves no result of its kind to fetch.
//
// An extractor over a decoder GROUP (qsp_mesh_extractor_create_group) is the same extractor with one different launch: its codes
// come with a class index each (qsp_mesh_extract_batch_group) and the pass decodes them with k_group_grid_decode*, volume v on
// the parameters of member cls[v]; passes, scratch, results and the marching-cubes stages are those above.  The group's first
// member lends stream and settings (the members agree on them: group_check), the call holds every member's lock.  A pass is
// repeated on the f32 pipe when the range flag of ANY member is up after it, and counted as a group refinement call counts its
// own repeat: once per repeated pass, on the group's first member.
#pragma once

namespace qsp {
namespace mc {

constexpr int TMAX = 8;   // triangles per cell the generated table may need (asserted at start-up)

struct Tables {
    int8_t ntri[256];
    int8_t tri[256][TMAX * 3];   // cube-edge ids 0..11: id = 4 * axis + (u + 2 v), (u, v) offsets along the other two axes
};

inline void edge_ends(int e, int& c0, int& c1) {
    const int a = e >> 2, u = e & 1, v = (e >> 1) & 1;
    int base;
    if (a == 0) base = (u << 1) | (v << 2);
    else if (a == 1) base = u | (v << 2);
    else base = u | (v << 1);
    c0 = base;
    c1 = base | (1 << a);
}

inline int edge_between(int ca, int cb) {
    for (int e = 0; e < 12; ++e) {
        int c0, c1;
        edge_ends(e, c0, c1);
        if ((c0 == ca && c1 == cb) || (c0 == cb && c1 == ca)) return e;
    }
    return -1;
}

// bit (2 * axis + side) set when both end points of cube edge e lie on that cube face
inline int edge_face_mask(int e) {
    int c0, c1, m = 0;
    edge_ends(e, c0, c1);
    for (int a = 0; a < 3; ++a)
        for (int sd = 0; sd < 2; ++sd)
            if (((c0 >> a) & 1) == sd && ((c1 >> a) & 1) == sd) m |= 1 << (2 * a + sd);
    return m;
}

inline bool build_tables(Tables& T) {
    for (int cs = 0; cs < 256; ++cs) {
        int nb[12][2], deg[12];
        for (int e = 0; e < 12; ++e) { deg[e] = 0; nb[e][0] = nb[e][1] = -1; }
        auto link = [&](int ea, int eb) {
            if (deg[ea] < 2) nb[ea][deg[ea]] = eb;
            if (deg[eb] < 2) nb[eb][deg[eb]] = ea;
            deg[ea]++; deg[eb]++;
        };
        for (int a = 0; a < 3; ++a)
            for (int sd = 0; sd < 2; ++sd) {
                const int b = (a + 1) % 3, c = (a + 2) % 3;
                const int ob[4] = {0, 1, 1, 0}, oc[4] = {0, 0, 1, 1};
                int q[4], in[4], fe[4];
                for (int k = 0; k < 4; ++k) {
                    q[k] = (sd << a) | (ob[k] << b) | (oc[k] << c);
                    in[k] = (cs >> q[k]) & 1;
                }
                int ncross = 0, cross[4];
                for (int k = 0; k < 4; ++k) {
                    fe[k] = edge_between(q[k], q[(k + 1) & 3]);
                    if (in[k] != in[(k + 1) & 3]) cross[ncross++] = k;
                }
                if (ncross == 2) link(fe[cross[0]], fe[cross[1]]);
                else if (ncross == 4)
                    for (int k = 0; k < 4; ++k)
                        if (in[k]) link(fe[(k + 3) & 3], fe[k]);      // the two face edges meeting at inside corner k
            }
        bool used[12] = {};
        int nt = 0;
        for (int e0 = 0; e0 < 12; ++e0) {
            if (deg[e0] == 0 || used[e0]) continue;
            if (deg[e0] != 2) return false;
            int loop[12], n = 0, prev = -1, cur = e0;
            do {
                loop[n++] = cur;
                used[cur] = true;
                int nx = nb[cur][0], ny = nb[cur][1];
                int next;
                if (prev < 0) next = nx < ny ? nx : ny;
                else next = (nx == prev) ? ny : nx;
                if (nx == ny) next = nx;          // two-edge loops cannot occur on a cube, kept for safety
                prev = cur;
                cur = next;
            } while (cur != e0 && n < 12);
            if (n < 3) return false;
            // orientation: Newell normal of the mid-point polygon against the inside -> outside direction
            double nrm[3] = {0, 0, 0}, g[3] = {0, 0, 0}, P[12][3];
            for (int k = 0; k < n; ++k) {
                int c0, c1;
                edge_ends(loop[k], c0, c1);
                for (int ax = 0; ax < 3; ++ax) {
                    const double p0 = (c0 >> ax) & 1, p1 = (c1 >> ax) & 1;
                    P[k][ax] = 0.5 * (p0 + p1);
                    const int in0 = (cs >> c0) & 1;
                    g[ax] += in0 ? (p1 - p0) : (p0 - p1);
                }
            }
            for (int k = 0; k < n; ++k) {
                const double* p = P[k];
                const double* qn = P[(k + 1) % n];
                nrm[0] += (p[1] - qn[1]) * (p[2] + qn[2]);
                nrm[1] += (p[2] - qn[2]) * (p[0] + qn[0]);
                nrm[2] += (p[0] - qn[0]) * (p[1] + qn[1]);
            }
            const double dot = nrm[0] * g[0] + nrm[1] * g[1] + nrm[2] * g[2];
            if (dot == 0) return false;
            if (dot < 0)
                for (int lo = 1, hi = n - 1; lo < hi; ++lo, --hi) { const int tmp = loop[lo]; loop[lo] = loop[hi]; loop[hi] = tmp; }
            // fan apex: the first loop vertex none of whose fan diagonals joins two edges of one cube face -- such a
            // diagonal would lie IN that face, where the neighbouring cell could pick the same one (a non-manifold flap)
            int apex = -1;
            for (int s0 = 0; s0 < n && apex < 0; ++s0) {
                bool ok = true;
                for (int k = 2; k + 1 < n; ++k)
                    if (edge_face_mask(loop[s0]) & edge_face_mask(loop[(s0 + k) % n])) ok = false;
                if (ok) apex = s0;
            }
            if (apex < 0) return false;
            for (int k = 1; k + 1 < n; ++k) {
                if (nt >= TMAX) return false;
                T.tri[cs][3 * nt] = (int8_t)loop[apex];
                T.tri[cs][3 * nt + 1] = (int8_t)loop[(apex + k) % n];
                T.tri[cs][3 * nt + 2] = (int8_t)loop[(apex + k + 1) % n];
                ++nt;
            }
        }
        T.ntri[cs] = (int8_t)nt;
        for (int k = 3 * nt; k < TMAX * 3; ++k) T.tri[cs][k] = -1;
    }
    return true;
}

constexpr int SCAN_ITEMS = 8;
constexpr int SCAN_BLOCK = 256 * SCAN_ITEMS;

// per grid point: bits 0..2 = its three owned edges (+axis 0/1/2) cross the surface; packed counts: low 32 bits
// vertices owned by the point, high 32 bits triangles of the cell whose lowest corner it is
__global__ __launch_bounds__(256) void k_mc_flags(const float* __restrict__ sdf, int d, const Tables* __restrict__ T,
                                                  uint8_t* __restrict__ flags, unsigned long long* __restrict__ cnt, int64_t n_pad) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pad) return;
    const int64_t n = (int64_t)d * d * d;
    if (p >= n) { cnt[p] = 0; return; }
    const int i2 = (int)(p % d), i1 = (int)((p / d) % d), i0 = (int)(p / ((int64_t)d * d));
    const int64_t st[3] = {(int64_t)d * d, d, 1};
    const int idx[3] = {i0, i1, i2};
    const bool in0 = sdf[p] < 0.f;
    unsigned f = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
        if (idx[a] + 1 < d && ((sdf[p + st[a]] < 0.f) != in0)) f |= 1u << a;
    unsigned nt = 0;
    if (i0 + 1 < d && i1 + 1 < d && i2 + 1 < d) {
        unsigned cs = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (sdf[p + (c & 1) * st[0] + ((c >> 1) & 1) * st[1] + ((c >> 2) & 1) * st[2]] < 0.f) cs |= 1u << c;
        nt = (unsigned)T->ntri[cs];
    }
    flags[p] = (uint8_t)f;
    cnt[p] = (unsigned long long)__popc(f) | ((unsigned long long)nt << 32);
}

// exclusive scan inside blocks of SCAN_BLOCK items (in place) + block totals
__global__ __launch_bounds__(256) void k_mc_scan_blocks(unsigned long long* __restrict__ cnt, unsigned long long* __restrict__ bsum) {
    __shared__ unsigned long long wsum[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned long long* base = cnt + (size_t)blockIdx.x * SCAN_BLOCK + (size_t)t * SCAN_ITEMS;
    unsigned long long v[SCAN_ITEMS], tot = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) { v[i] = base[i]; tot += v[i]; }
    unsigned long long inc = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned long long off = inc - tot;
    for (int w = 0; w < wave; ++w) off += wsum[w];
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) { base[i] = off; off += v[i]; }
    if (t == 255) bsum[blockIdx.x] = off;
}

// exclusive scan of the block totals (<= 1024) by one workgroup; total[0] = grand total
__device__ inline void scan_top(unsigned long long* __restrict__ bsum, int nb, unsigned long long* __restrict__ total) {
    __shared__ unsigned long long wsum[16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned long long v = t < nb ? bsum[t] : 0;
    unsigned long long inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned long long off = inc - v;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    if (t < nb) bsum[t] = off;
    if (t == 1023) total[0] = off + v;
}
__global__ __launch_bounds__(1024) void k_mc_scan_top(unsigned long long* __restrict__ bsum, int nb, unsigned long long* __restrict__ total) {
    scan_top(bsum, nb, total);
}
// a batch pass: volume blockIdx.x's nb block totals, scanned from 0; its totals to vtot (for the host) and voff (scanned next)
__global__ __launch_bounds__(1024) void k_mc_scan_top_batch(unsigned long long* __restrict__ bsum, int nb, unsigned long long* __restrict__ vtot,
                                                            unsigned long long* __restrict__ voff) {
    const int v = blockIdx.x;
    scan_top(bsum + (size_t)v * nb, nb, vtot + v);
    if (threadIdx.x == 1023) voff[v] = vtot[v];      // (the thread that wrote it)
}

__device__ inline unsigned vertex_id(const uint8_t* flags, const unsigned long long* cnt, const unsigned long long* bsum, int64_t q, int a) {
    const unsigned base = (unsigned)(cnt[q] & 0xffffffffull) + (unsigned)(bsum[q / SCAN_BLOCK] & 0xffffffffull);
    return base + __popc((unsigned)flags[q] & ((1u << a) - 1u));
}

__global__ __launch_bounds__(256) void k_mc_emit(const float* __restrict__ sdf, int d, float voxel_size, const Tables* __restrict__ T,
                                                 const uint8_t* __restrict__ flags, const unsigned long long* __restrict__ cnt,
                                                 const unsigned long long* __restrict__ bsum, float* __restrict__ verts,
                                                 int32_t* __restrict__ faces) {
    const int64_t n = (int64_t)d * d * d;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int i2 = (int)(p % d), i1 = (int)((p / d) % d), i0 = (int)(p / ((int64_t)d * d));
    const int64_t st[3] = {(int64_t)d * d, d, 1};
    const int idx[3] = {i0, i1, i2};
    const unsigned f = flags[p];
    const float v0 = sdf[p];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!(f & (1u << a))) continue;
        const float v1 = sdf[p + st[a]];
        const unsigned vid = vertex_id(flags, cnt, bsum, p, a);
        {
#pragma clang fp contract(off)      // separately rounded multiply and add, like the numpy restatement (bit-exact vertices)
            const float t = v0 / (v0 - v1);
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const float ci = (ax == a) ? (float)idx[ax] + t : (float)idx[ax];
                const float scaled = ci * voxel_size;
                verts[3 * (size_t)vid + ax] = scaled + (-1.0f);
            }
        }
    }
    if (i0 + 1 < d && i1 + 1 < d && i2 + 1 < d) {
        unsigned cs = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (sdf[p + (c & 1) * st[0] + ((c >> 1) & 1) * st[1] + ((c >> 2) & 1) * st[2]] < 0.f) cs |= 1u << c;
        const int nt = T->ntri[cs];
        if (nt) {
            const size_t f0 = (size_t)(cnt[p] >> 32) + (size_t)(bsum[p / SCAN_BLOCK] >> 32);
            for (int k = 0; k < 3 * nt; ++k) {
                const int e = T->tri[cs][k];
                const int a = e >> 2, u = e & 1, v = (e >> 1) & 1;
                int o[3];
                if (a == 0) { o[0] = 0; o[1] = u; o[2] = v; }
                else if (a == 1) { o[0] = u; o[1] = 0; o[2] = v; }
                else { o[0] = u; o[1] = v; o[2] = 0; }
                const int64_t q = p + o[0] * st[0] + o[1] * st[1] + o[2] * st[2];
                faces[3 * f0 + k] = (int32_t)vertex_id(flags, cnt, bsum, q, a);
            }
        }
    }
}

}  // namespace mc
}  // namespace qsp

#include "mesh_lewiner.hpp"

constexpr int QSP_MESH_BATCH_LIMIT_DEFAULT = 64;      // volumes per pass of a batch call

// a device buffer and the number of elements it holds
template <class T> struct MeshBuf {
    T* p = nullptr;
    int64_t cap = 0;
};

struct qsp_mesh_extractor {
    qsp_decoder* dec = nullptr;     // over a group: its first member (stream, device, settings -- the same for every member)
    qsp_decoder_group* grp = nullptr;   // set: codes come with a class index each and are decoded by their member of grp->Pd
    int device = 0;         // of the decoder, cached: destroy must not touch a decoder that may already be gone
    int method = 0;         // 0: Lewiner's marching cubes, what the reference calls (mesh_lewiner.hpp); 1: the face-consistent table of rounds 2-3
    int limit = QSP_MESH_BATCH_LIMIT_DEFAULT;
    int dim = 0;
    int64_t n = 0, n_pad = 0;
    int nb = 0;
    float voxel_size = 0;
    float* xyz = nullptr;
    qsp::mc::Tables* tables = nullptr;
    // scratch of a pass of V volumes, shared by all calls: nothing in it is read after the call that filled it
    struct Scratch {
        MeshBuf<float> codes;                           // (items, CODE_LEN): the whole call's
        MeshBuf<int32_t> cls;                           // (items): their class indices (an extractor over a decoder group)
        MeshBuf<unsigned long long> cnt, bsum, vtot, voff;      // (V, n_pad), (V, nb), (V), (V + 1: the grand total last)
        MeshBuf<int32_t> vmap;                          // Lewiner: (V, 3, n), (axis, grid point) -> vertex number
        MeshBuf<uint8_t> flags;                         // method 1: (n_pad)
    } s;
    // what a fetch reads: one for the single calls, one for the batch calls
    struct Result {
        MeshBuf<float> sdf;                             // (items, n): decoded or uploaded
        MeshBuf<float> verts, vidx;                     // the meshes, concatenated in item order; vidx (Lewiner): float32 index
        MeshBuf<int32_t> faces;                         // coordinates (the float64 mesh of the reference is these x spacing - 1)
        std::vector<int64_t> n_verts, n_faces;          // per item
        int64_t tot_verts = 0, tot_faces = 0;
        int method = 0;                                 // that marched it
        bool have = false;
    } single, batch;
};

extern "C" void qsp_mesh_extractor_destroy(qsp_mesh_extractor* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    void* ptrs[] = {m->xyz, m->tables, m->s.codes.p, m->s.cls.p, m->s.cnt.p, m->s.bsum.p, m->s.vtot.p, m->s.voff.p, m->s.vmap.p, m->s.flags.p,
                    m->single.sdf.p, m->single.verts.p, m->single.vidx.p, m->single.faces.p,
                    m->batch.sdf.p, m->batch.verts.p, m->batch.vidx.p, m->batch.faces.p};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    delete m;
    (void)hipGetLastError();   // errors are ignored here; do not leave one behind for the next call's launch check
}

// an extractor over `dec`, or over the group `grp` whose first member `dec` is
static int mesh_extractor_new(qsp_decoder* dec, qsp_decoder_group* grp, int32_t voxels_dim, const float* voxel_points,
                              qsp_mesh_extractor** out) {
    using namespace qsp;
    if (voxels_dim < 2 || voxels_dim > 128) return qsp_fail(QSP_ERR_UNSUPPORTED, "mesh extractor: 2 <= voxels_dim <= 128");
    static mc::Tables host_tables;
    static const bool tables_ok = mc::build_tables(host_tables);
    if (!tables_ok) return qsp_fail(QSP_ERR_DEVICE, "marching-cubes table generation failed");
    QSP_HIP(hipSetDevice(dec->device));
    qsp_mesh_extractor* m = new qsp_mesh_extractor();
    m->dec = dec;
    m->grp = grp;
    m->device = dec->device;
    m->dim = voxels_dim;
    m->n = (int64_t)voxels_dim * voxels_dim * voxels_dim;
    m->nb = (int)((m->n + mc::SCAN_BLOCK - 1) / mc::SCAN_BLOCK);
    m->n_pad = (int64_t)m->nb * mc::SCAN_BLOCK;
    m->voxel_size = (float)(2.0 / (voxels_dim - 1));
    // the two buffers that are filled here; every other one grows with the calls (mesh_call)
    hipError_t e = hipMalloc((void**)&m->xyz, sizeof(float) * 3 * m->n);
    if (e == hipSuccess) e = hipMalloc((void**)&m->tables, sizeof(mc::Tables));
    if (e == hipSuccess) e = hipMemcpy(m->xyz, voxel_points, sizeof(float) * 3 * m->n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(m->tables, &host_tables, sizeof(mc::Tables), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        qsp_mesh_extractor_destroy(m);
        return qsp_fail(QSP_ERR_DEVICE, hipGetErrorString(e));
    }
    *out = m;
    return QSP_OK;
}

extern "C" int qsp_mesh_extractor_create(qsp_decoder* dec, int32_t voxels_dim, const float* voxel_points,
                                         qsp_mesh_extractor** out) {
    if (!dec || !out || !voxel_points) return qsp_fail(QSP_ERR_INVALID, "qsp_mesh_extractor_create: null argument");
    return mesh_extractor_new(dec, nullptr, voxels_dim, voxel_points, out);
}

extern "C" int qsp_mesh_extractor_create_group(qsp_decoder_group* g, int32_t voxels_dim, const float* voxel_points,
                                               qsp_mesh_extractor** out) {
    if (!g || !out || !voxel_points) return qsp_fail(QSP_ERR_INVALID, "qsp_mesh_extractor_create_group: null argument");
    const CallLock lk(g);
    const int rc = group_check(g);
    if (rc) return rc;
    return mesh_extractor_new(g->m[0], g, voxels_dim, voxel_points, out);
}

// The locks of a call on an extractor: its decoder's, or over a group every member's in the group's order (a null extractor: none).
static CallLock mesh_lock(qsp_mesh_extractor* m) {
    if (m && m->grp) return CallLock(m->grp);
    return CallLock(m ? m->dec : (qsp_decoder*)nullptr);
}

// after a synchronisation of the extractor's stream: did the grid decode leave fp16's range?  Over a group every member's flag
// is read (and cleared): each is raised by the tiles that ran on that member.
static bool mesh_range_hit(qsp_mesh_extractor* m) {
    if (!m->grp) return range_hit(m->dec);
    bool hit = false;
    for (qsp_decoder* d : m->grp->lock_order) hit = range_hit(d) || hit;
    return hit;
}

// device buffer of at least `need` elements; its first `keep` elements survive when it has to move
template <class T> static int mesh_reserve(MeshBuf<T>& b, int64_t need, int64_t keep, hipStream_t s) {
    if (need <= b.cap) return QSP_OK;
    const int64_t ncap = need + need / 4 + 1024;
    T* q = nullptr;
    QSP_HIP(hipMalloc((void**)&q, sizeof(T) * ncap));
    if (keep && b.p) {
        hipError_t e = hipMemcpyAsync(q, b.p, sizeof(T) * keep, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            (void)hipFree(q);
            return qsp_fail(QSP_ERR_DEVICE, hipGetErrorString(e));
        }
    } else if (b.p) {
        QSP_HIP(hipStreamSynchronize(s));      // (nothing queued may still use the buffer that goes)
    }
    if (b.p) (void)hipFree(b.p);
    b.p = q;
    b.cap = ncap;
    return QSP_OK;
}

// marching cubes on items [i0, i0 + V) of a call, whose volumes are in r.sdf; with `decode`, the grid decode of their codes
// first, in the same stream order.  One synchronisation: the read of the pass's totals (and of the fp16 range flag with them).
// Method 1 (k_mc_flags / k_mc_emit) is a pass of V = 1 of a single call: voff[0] = 0 and nothing before it, so its kernels
// take the pass's buffers as they are.
static int mesh_pass(qsp_mesh_extractor* m, qsp_mesh_extractor::Result& r, int64_t i0, int V, bool decode, bool* hit) {
    using namespace qsp;
    auto& sc = m->s;
    hipStream_t s = m->dec->stream;
    float* sdf = r.sdf.p + i0 * m->n;
    const bool lewiner = m->method == 0;
    const lew::BatchPass bp = {m->dim, m->nb, mc::SCAN_BLOCK, m->n, m->n_pad, m->voxel_size};
    if (decode && m->grp) launch_grid_decode_group(m->grp, sc.codes.p + i0 * CODE_LEN, sc.cls.p + i0, m->xyz, m->n, V, sdf);
    else if (decode) launch_grid_decode(m->dec, sc.codes.p + i0 * CODE_LEN, m->xyz, m->n, V, sdf);
    const dim3 gc((int)(m->n_pad / 256), V);
    if (lewiner) hipLaunchKernelGGL(lew::k_lew_count, gc, dim3(256), 0, s, sdf, bp, sc.cnt.p);
    else hipLaunchKernelGGL(mc::k_mc_flags, gc, dim3(256), 0, s, sdf, m->dim, m->tables, sc.flags.p, sc.cnt.p, m->n_pad);
    hipLaunchKernelGGL(mc::k_mc_scan_blocks, dim3(m->nb * V), dim3(256), 0, s, sc.cnt.p, sc.bsum.p);
    hipLaunchKernelGGL(mc::k_mc_scan_top_batch, dim3(V), dim3(1024), 0, s, sc.bsum.p, m->nb, sc.vtot.p, sc.voff.p);
    hipLaunchKernelGGL(mc::k_mc_scan_top, dim3(1), dim3(1024), 0, s, sc.voff.p, V, sc.voff.p + V);
    QSP_HIP(hipGetLastError());
    std::vector<unsigned long long> tot(V);
    QSP_HIP(hipMemcpyAsync(tot.data(), sc.vtot.p, sizeof(unsigned long long) * V, hipMemcpyDeviceToHost, s));
    QSP_HIP(hipStreamSynchronize(s));
    *hit = decode && mesh_range_hit(m);
    if (*hit) return QSP_OK;        // (the caller decodes the pass again on the f32 pipe, or fails)
    int64_t nv = 0, nf = 0;
    for (int v = 0; v < V; ++v) {
        r.n_verts[i0 + v] = (int64_t)(tot[v] & 0xffffffffull);
        r.n_faces[i0 + v] = (int64_t)(tot[v] >> 32);
        nv += r.n_verts[i0 + v];
        nf += r.n_faces[i0 + v];
    }
    if (nv) {       // (a pass without any surface launches nothing more)
        int rc = mesh_reserve(r.verts, 3 * (r.tot_verts + nv), 3 * r.tot_verts, s);
        if (!rc) rc = mesh_reserve(r.vidx, 3 * (r.tot_verts + nv), 3 * r.tot_verts, s);
        if (!rc) rc = mesh_reserve(r.faces, 3 * (r.tot_faces + nf), 3 * r.tot_faces, s);
        if (rc) return rc;
        const dim3 g((int)((m->n + 255) / 256), V);
        if (lewiner) {
            hipLaunchKernelGGL(lew::k_lew_verts, g, dim3(256), 0, s, sdf, bp, sc.cnt.p, sc.bsum.p, sc.voff.p, r.tot_verts, r.vidx.p, r.verts.p,
                               sc.vmap.p);
            hipLaunchKernelGGL(lew::k_lew_faces, g, dim3(256), 0, s, sdf, bp, sc.cnt.p, sc.bsum.p, sc.voff.p, r.tot_faces, sc.vmap.p, r.faces.p);
        } else
            hipLaunchKernelGGL(mc::k_mc_emit, g, dim3(256), 0, s, sdf, m->dim, m->voxel_size, m->tables, sc.flags.p, sc.cnt.p, sc.bsum.p,
                               r.verts.p, r.faces.p);
        QSP_HIP(hipGetLastError());
    }
    r.tot_verts += nv;
    r.tot_faces += nf;
    return QSP_OK;
}

// A call: n codes (decode; the decoder's code_len entries each; over a group with their n class indices cls, checked by the
// caller) or n volumes from the host -> r.  r holds no result until the call has succeeded.  Buffers for n volumes in passes of
// at most `limit`, the input's upload, then the passes.
static int mesh_call(qsp_mesh_extractor* m, qsp_mesh_extractor::Result& r, int32_t n, const float* in, bool decode,
                     const int32_t* cls = nullptr) {
    using namespace qsp;
    QSP_HIP(hipSetDevice(m->dec->device));
    r.have = false;
    auto& sc = m->s;
    hipStream_t s = m->dec->stream;
    const bool lewiner = m->method == 0;
    const int64_t n_pass = std::min<int64_t>(n, m->limit);
    int rc = mesh_reserve(sc.codes, (int64_t)n * CODE_LEN, 0, s);
    if (!rc && cls) rc = mesh_reserve(sc.cls, n, 0, s);
    if (!rc) rc = mesh_reserve(r.sdf, n * m->n, 0, s);
    if (!rc) rc = mesh_reserve(sc.cnt, n_pass * m->n_pad, 0, s);
    if (!rc) rc = mesh_reserve(sc.bsum, n_pass * m->nb, 0, s);
    if (!rc) rc = mesh_reserve(sc.vtot, n_pass, 0, s);
    if (!rc) rc = mesh_reserve(sc.voff, n_pass + 1, 0, s);
    if (!rc) rc = mesh_reserve(sc.vmap, lewiner ? n_pass * 3 * m->n : 0, 0, s);
    if (!rc) rc = mesh_reserve(sc.flags, lewiner ? 0 : m->n_pad, 0, s);
    if (rc) return rc;
    if (decode) {
        const int L = m->dec->code_len;
        std::vector<float> c64((size_t)n * CODE_LEN, 0.f);           // padded to CODE_LEN
        for (int32_t i = 0; i < n; ++i) memcpy(&c64[(size_t)i * CODE_LEN], in + (size_t)i * L, sizeof(float) * L);
        QSP_HIP(hipMemcpyAsync(sc.codes.p, c64.data(), sizeof(float) * c64.size(), hipMemcpyHostToDevice, s));
        if (cls) QSP_HIP(hipMemcpyAsync(sc.cls.p, cls, sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
        QSP_HIP(hipStreamSynchronize(s));                            // (c64 lives on this frame)
    } else {
        QSP_HIP(hipMemcpyAsync(r.sdf.p, in, sizeof(float) * n * m->n, hipMemcpyHostToDevice, s));
    }
    r.n_verts.assign(n, 0);
    r.n_faces.assign(n, 0);
    r.tot_verts = r.tot_faces = 0;
    r.method = m->method;
    for (int64_t i0 = 0; i0 < n; i0 += m->limit) {
        const int V = (int)std::min<int64_t>(m->limit, n - i0);
        bool hit = false;
        rc = mesh_pass(m, r, i0, V, decode, &hit);
        if (rc) return rc;
        if (hit) {      // a value of the grid decode left fp16's range: this pass again on the f32 pipe, counted once (over a group: on
                        // its first member, m->dec, whichever member's flag was up) -- or the call fails
            if (!range_should_fall_back(m->dec)) return range_error();
            F32Override f32(m->dec);
            m->dec->n_range_fallbacks++;
            rc = mesh_pass(m, r, i0, V, decode, &hit);
            if (rc) return rc;
        }
    }
    QSP_HIP(hipStreamSynchronize(s));
    r.have = true;
    return QSP_OK;
}

// the code-taking single-decoder calls on an extractor over a group: a code there needs its class
static int group_extractor_refusal(const char* who) {
    return qsp_fail(QSP_ERR_INVALID, (std::string(who) + ": this extractor is over a decoder group, where every code names its class: "
                                                         "call qsp_mesh_extract_batch_group").c_str());
}

static int mesh_single(qsp_mesh_extractor* m, const float* in, bool decode, int64_t* n_verts, int64_t* n_faces) {
    const int rc = mesh_call(m, m->single, 1, in, decode);
    if (rc) return rc;
    if (n_verts) *n_verts = m->single.n_verts[0];
    if (n_faces) *n_faces = m->single.n_faces[0];
    return QSP_OK;
}

extern "C" int qsp_mesh_extract(qsp_mesh_extractor* m, const float* code, int64_t* n_verts, int64_t* n_faces) {
    const CallLock lk = mesh_lock(m);
    if (!m || !code) return qsp_fail(QSP_ERR_INVALID, "qsp_mesh_extract: null argument");
    if (m->grp) return group_extractor_refusal("qsp_mesh_extract");
    return mesh_single(m, code, true, n_verts, n_faces);
}

extern "C" int qsp_mesh_from_volume(qsp_mesh_extractor* m, const float* sdf_volume, int64_t* n_verts, int64_t* n_faces) {
    const CallLock lk = mesh_lock(m);
    if (!m || !sdf_volume) return qsp_fail(QSP_ERR_INVALID, "qsp_mesh_from_volume: null argument");
    return mesh_single(m, sdf_volume, false, n_verts, n_faces);
}

// argument checks of both batch entry points, then the call; a batch that fails leaves no batch result behind
// (group: the call is qsp_mesh_extract_batch_group, cls its class indices)
static int mesh_batch(qsp_mesh_extractor* m, int32_t n, const float* in, bool decode, int64_t* n_verts, int64_t* n_faces, const char* who,
                      bool group = false, const int32_t* cls = nullptr) {
    const std::string w(who);
    if (!m || !in || !n_verts || !n_faces || (group && !cls)) return qsp_fail(QSP_ERR_INVALID, (w + ": null argument").c_str());
    if (n < 0) return qsp_fail(QSP_ERR_INVALID, (w + ": negative number of items").c_str());
    if (group && !m->grp)
        return qsp_fail(QSP_ERR_INVALID, (w + ": this extractor is over one decoder (qsp_mesh_extractor_create): call "
                                              "qsp_mesh_extract_batch, or create it with qsp_mesh_extractor_create_group").c_str());
    if (decode && !group && m->grp) return group_extractor_refusal(who);
    if (m->method != 0)
        return qsp_fail(QSP_ERR_UNSUPPORTED, (w + ": batches run Lewiner's marching cubes (method 0) only; method 1, the "
                                                  "face-consistent table, is extracted one mesh per call").c_str());
    if (n == 0) return QSP_OK;
    int rc = QSP_OK;
    if (group) {      // (a member's options may have changed since the extractor was created)
        rc = group_check(m->grp);
        if (!rc) rc = group_classes(m->grp, n, cls);
        if (rc) return rc;
    }
    rc = mesh_call(m, m->batch, n, in, decode, group ? cls : nullptr);
    if (rc) return rc;
    std::copy(m->batch.n_verts.begin(), m->batch.n_verts.end(), n_verts);
    std::copy(m->batch.n_faces.begin(), m->batch.n_faces.end(), n_faces);
    return QSP_OK;
}

extern "C" int qsp_mesh_extract_batch(qsp_mesh_extractor* m, int32_t n, const float* codes, int64_t* n_verts, int64_t* n_faces) {
    const CallLock lk = mesh_lock(m);
    return mesh_batch(m, n, codes, true, n_verts, n_faces, "qsp_mesh_extract_batch");
}

extern "C" int qsp_mesh_extract_batch_group(qsp_mesh_extractor* m, int32_t n, const float* codes, const int32_t* cls, int64_t* n_verts,
                                            int64_t* n_faces) {
    const CallLock lk = mesh_lock(m);
    return mesh_batch(m, n, codes, true, n_verts, n_faces, "qsp_mesh_extract_batch_group", true, cls);
}

extern "C" int qsp_mesh_from_volumes(qsp_mesh_extractor* m, int32_t n, const float* sdf_volumes, int64_t* n_verts, int64_t* n_faces) {
    const CallLock lk = mesh_lock(m);
    return mesh_batch(m, n, sdf_volumes, false, n_verts, n_faces, "qsp_mesh_from_volumes");
}

// A result to the host, concatenated in item order; any pointer may be null.  verts_f64: the vertices as the reference holds
// them, float64 = float32 index coordinate x (2 / (n - 1)) + (-1) (skimage multiplies its float32 vertices by the float64
// spacing, reconstruct/utils.py:131-139 adds the origin); the table method has no index coordinates: its float32 vertices, widened.
static int mesh_fetch(qsp_mesh_extractor* m, const qsp_mesh_extractor::Result& r, float* verts, double* verts_f64, int32_t* faces,
                      float* sdf_volumes, const char* who) {
    if (!r.have) return qsp_fail(QSP_ERR_INVALID, (std::string(who) + ": nothing extracted yet").c_str());
    QSP_HIP(hipSetDevice(m->dec->device));
    hipStream_t s = m->dec->stream;
    const bool lewiner = r.method == 0;
    std::vector<float> tmp;
    if (verts && r.tot_verts) QSP_HIP(hipMemcpyAsync(verts, r.verts.p, sizeof(float) * 3 * r.tot_verts, hipMemcpyDeviceToHost, s));
    if (verts_f64 && r.tot_verts) {
        tmp.resize((size_t)3 * r.tot_verts);
        QSP_HIP(hipMemcpyAsync(tmp.data(), lewiner ? r.vidx.p : r.verts.p, sizeof(float) * tmp.size(), hipMemcpyDeviceToHost, s));
    }
    if (faces && r.tot_faces) QSP_HIP(hipMemcpyAsync(faces, r.faces.p, sizeof(int32_t) * 3 * r.tot_faces, hipMemcpyDeviceToHost, s));
    if (sdf_volumes) QSP_HIP(hipMemcpyAsync(sdf_volumes, r.sdf.p, sizeof(float) * r.n_verts.size() * m->n, hipMemcpyDeviceToHost, s));
    QSP_HIP(hipStreamSynchronize(s));
    const double spacing = 2.0 / (double)(m->dim - 1);
    for (size_t i = 0; i < tmp.size(); ++i) verts_f64[i] = lewiner ? (double)tmp[i] * spacing + (-1.0) : (double)tmp[i];
    return QSP_OK;
}

extern "C" int qsp_mesh_fetch(qsp_mesh_extractor* m, float* verts, int32_t* faces, float* sdf_volume) {
    if (!m) return qsp_fail(QSP_ERR_INVALID, "qsp_mesh_fetch: null extractor");
    return mesh_fetch(m, m->single, verts, nullptr, faces, sdf_volume, "qsp_mesh_fetch");
}

extern "C" int qsp_mesh_fetch_f64(qsp_mesh_extractor* m, double* verts) {
    if (!m || !verts) return qsp_fail(QSP_ERR_INVALID, "qsp_mesh_fetch_f64: null argument");
    return mesh_fetch(m, m->single, nullptr, verts, nullptr, nullptr, "qsp_mesh_fetch_f64");
}

extern "C" int qsp_mesh_fetch_batch(qsp_mesh_extractor* m, float* verts, double* verts_f64, int32_t* faces, float* sdf_volumes) {
    if (!m) return qsp_fail(QSP_ERR_INVALID, "qsp_mesh_fetch_batch: null extractor");
    const CallLock lk = mesh_lock(m);
    return mesh_fetch(m, m->batch, verts, verts_f64, faces, sdf_volumes, "qsp_mesh_fetch_batch");
}

extern "C" int qsp_mesh_extractor_set_method(qsp_mesh_extractor* m, int32_t method) {
    if (!m) return qsp_fail(QSP_ERR_INVALID, "qsp_mesh_extractor_set_method: null extractor");
    if (method != 0 && method != 1) return qsp_fail(QSP_ERR_INVALID, "mesh method: 0 (Lewiner's marching cubes, the reference's) or 1 (face-consistent table)");
    m->method = method;
    return QSP_OK;
}

extern "C" int qsp_mesh_extractor_set_batch_limit(qsp_mesh_extractor* m, int32_t max_volumes_per_pass) {
    if (!m) return qsp_fail(QSP_ERR_INVALID, "qsp_mesh_extractor_set_batch_limit: null extractor");
    if (max_volumes_per_pass < 1 || max_volumes_per_pass > QSP_MESH_BATCH_LIMIT_DEFAULT)
        return qsp_fail(QSP_ERR_INVALID, "mesh batch limit: 1 .. 64 (QSP_MESH_BATCH_LIMIT_DEFAULT) volumes per pass");
    const CallLock lk = mesh_lock(m);
    m->limit = max_volumes_per_pass;
    return QSP_OK;
}

extern "C" int qsp_mc_tables(int8_t* ntri /*256*/, int8_t* tri /*256 x 24*/) {
    static qsp::mc::Tables t;
    static const bool ok = qsp::mc::build_tables(t);
    if (!ok) return qsp_fail(QSP_ERR_DEVICE, "marching-cubes table generation failed");
    if (ntri) memcpy(ntri, t.ntri, 256);
    if (tri) memcpy(tri, t.tri, 256 * qsp::mc::TMAX * 3);
    return QSP_OK;
}
