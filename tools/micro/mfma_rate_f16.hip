// Micro-benchmark: what the fp16 matrix pipe sustains when NOTHING else runs -- v_mfma_f32_32x32x16_f16 back to back on every
// SIMD of the chip for ~0.2 s, with realistic operands (random fp16 values of the decoder's magnitudes: switching activity sets
// the power and the power sets the clock).  Reports TFLOP/s of the pipe, cycles per MFMA and the shader clock (cycle counter
// against the constant 100 MHz real-time counter).  The dense fp16 peak of the data sheet (2.5 PFLOP/s) assumes 2.4 GHz.
// The second part compares the two fp16 MFMA shapes on the split-fp16 tile's work per wave: 128 units x 64 points, two
// accumulator sets (main and cross terms), three products per slab, operands in registers, one wave per SIMD, random data.
// The two loops alternate back to back after 2 s of launches, so both run at the clock the chip holds under that load.  Each
// shape runs twice: as one fixed share of the work per workgroup (the launch ends with its slowest workgroup) and as chunks
// taken from an atomic queue, the way k_mlp_jtj_h2 takes its work items (the wall time then follows the mean rate).
//   hipcc --offload-arch=gfx950 -O3 -o mfma_rate_f16 tools/micro/mfma_rate_f16.hip && ./mfma_rate_f16
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <vector>
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <int MODE>     // 0: zero operands, 1: random operands (|x| < 0.6), 2 / 3: random, with 1 in 4 / 1 in 2 issue slots left empty
__global__ __launch_bounds__(256) void k_rate(float* out, unsigned long long* cyc, unsigned long long* rt, int iters, const _Float16* rnd) {
    f32x16 acc[8];
    for (int a = 0; a < 8; ++a)
        for (int i = 0; i < 16; ++i) acc[a][i] = 0.f;
    f16x8 x[4], y[4];
    for (int u = 0; u < 4; ++u)
        for (int j = 0; j < 8; ++j) {
            x[u][j] = MODE ? rnd[(threadIdx.x * 32 + u * 8 + j) % 8192] : (_Float16)0.f;
            y[u][j] = MODE ? rnd[(threadIdx.x * 32 + u * 8 + j + 4099) % 8192] : (_Float16)0.f;
        }
    __syncthreads();
    const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
    const unsigned long long t0 = __builtin_readcyclecounter();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int a = 0; a < 8; ++a) {
                if ((MODE == 2 && (a & 3) == 3) || (MODE == 3 && (a & 1))) { asm volatile("s_nop 7"); continue; }     // (= 32 cycles)
                acc[a] = __builtin_amdgcn_mfma_f32_32x32x16_f16(x[u], y[(u + a) & 3], acc[a], 0, 0, 0);
            }
        }
    }
    const unsigned long long t1 = __builtin_readcyclecounter();
    const unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
    float s = 0;
    for (int a = 0; a < 8; ++a)
        for (int i = 0; i < 16; ++i) s += acc[a][i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
    if (threadIdx.x == 0) { cyc[blockIdx.x] = t1 - t0; rt[blockIdx.x] = r1 - r0; }
}

template <int MODE>
void run(const char* name, int iters, const _Float16* rnd, float* out, unsigned long long* cyc, unsigned long long* rt) {
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    for (int rep = 0; rep < 3; ++rep) {
        (void)hipEventRecord(e0);
        hipLaunchKernelGGL(k_rate<MODE>, dim3(256), dim3(256), 0, 0, out, cyc, rt, iters, rnd);
        (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
        float ms; (void)hipEventElapsedTime(&ms, e0, e1);
        unsigned long long hc, hr;
        (void)hipMemcpy(&hc, cyc, 8, hipMemcpyDeviceToHost);
        (void)hipMemcpy(&hr, rt, 8, hipMemcpyDeviceToHost);
        const double n_mfma = (MODE == 2 ? 24.0 : MODE == 3 ? 16.0 : 32.0) * iters;            // per wave = per SIMD
        const double tf = 2.0 * 32 * 32 * 16 * n_mfma * 4 * 256 / (ms * 1e-3) / 1e12;
        printf("%-44s %7.1f ms: %6.2f cycles/MFMA/SIMD, %7.1f TFLOP/s = %.3f of 2500, shader clock %.3f GHz\n", name, ms,
               (double)hc / n_mfma, tf, tf / 2500.0, (double)hc / (double)hr * 0.1);
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
}

// Accumulators pinned to AccVGPRs as in the production tile (with the builtin the compiler shuffles the 16x16 accumulators
// between the register files: 200 v_accvgpr_mov per 96 MFMAs).  Dependent MFMAs are interlocked by the hardware; the
// s_nops in front of the final read give the wait states a VALU read of an MFMA result needs.
__device__ __forceinline__ f32x16 mm(f16x8 a, f16x8 b, f32x16 c) {
    asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
    return c;
}
__device__ __forceinline__ f32x4 mm(f16x8 a, f16x8 b, f32x4 c) {
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
    return c;
}

// The split tile's products on one shape: S = 32 (v_mfma_f32_32x32x16_f16: 4 unit x 2 point tiles, 16 k per step, 24 MFMAs)
// or S = 16 (v_mfma_f32_16x16x32_f16: 8 x 4 tiles, 32 k per step, 96 MFMAs); `steps` is counted in 32 k for both.
// Q: the workgroup takes chunks of `steps` from *queue until `nchunks` are taken; otherwise it runs `steps` once.
// acc2 += w_lo' x_hi; acc2 += w_hi x_lo'; acc += w_hi x_hi, in the production loop's order.
template <int S, bool Q>
__global__ __launch_bounds__(256) void k_split(float* out, unsigned long long* cyc, unsigned long long* rt, int steps, const _Float16* rnd,
                                               int* queue, int nchunks) {
    __shared__ int chunk;
    constexpr int NU = 128 / S, NP = 64 / S, NA = S == 32 ? 16 : 4;
    typedef float accv __attribute__((ext_vector_type(NA)));
    accv acc[NP][NU], acc2[NP][NU];
    for (int r = 0; r < NP; ++r)
        for (int c = 0; c < NU; ++c)
            for (int i = 0; i < NA; ++i) { acc[r][c][i] = 0.f; acc2[r][c][i] = 0.f; }
    f16x8 wh[NU], wl[NU], xh[NP], xl[NP];
    const int t = threadIdx.x;
    // one 16-byte load per fragment (element-wise loads with wrapped indices cost the 16x16 form a ~1 ms prologue of SGPR spills)
    auto frag = [&](int i) { return *reinterpret_cast<const f16x8*>(rnd + 8 * (i & 1023)); };
    for (int c = 0; c < NU; ++c) { wh[c] = frag(t * 97 + c); wl[c] = frag(t * 97 + c + 129); }
    for (int r = 0; r < NP; ++r) { xh[r] = frag(t * 89 + r + 257); xl[r] = frag(t * 89 + r + 513); }
    __syncthreads();
    const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    const int iters = S == 32 ? 2 * steps : steps;
    for (;;) {
        if (Q) {
            if (threadIdx.x == 0) chunk = atomicAdd(queue, 1);
            __syncthreads();
            const int ch = chunk;
            __syncthreads();
            if (ch >= nchunks) break;
        }
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int c = 0; c < NU; ++c) {
#pragma unroll
            for (int r = 0; r < NP; ++r)
                acc2[r][c] = mm(wl[c], xh[r], acc2[r][c]);
#pragma unroll
            for (int r = 0; r < NP; ++r)
                acc2[r][c] = mm(wh[c], xl[r], acc2[r][c]);
#pragma unroll
            for (int r = 0; r < NP; ++r)
                acc[r][c] = mm(wh[c], xh[r], acc[r][c]);
        }
    }
        if (!Q) break;
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    const unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
    asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");
    float sum = 0;
    for (int r = 0; r < NP; ++r)
        for (int c = 0; c < NU; ++c)
            for (int i = 0; i < NA; ++i) sum += acc[r][c][i] + acc2[r][c][i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = sum;
    if (threadIdx.x == 0) { cyc[blockIdx.x] = t1 - t0; rt[blockIdx.x] = r1 - r0; }
}

// steps: the work of one workgroup; with Q it is taken in chunks of steps / QCH, QCH chunks per workgroup on average
constexpr int QCH = 64;
template <int S, bool Q>
float split_once(int steps, const _Float16* rnd, float* out, unsigned long long* cyc, unsigned long long* rt, int* queue, bool report) {
    static hipEvent_t e0, e1;
    static bool made = false;
    if (!made) { (void)hipEventCreate(&e0); (void)hipEventCreate(&e1); made = true; }
    (void)hipMemsetAsync(queue, 0, sizeof(int));
    (void)hipEventRecord(e0);
    hipLaunchKernelGGL((k_split<S, Q>), dim3(256), dim3(256), 0, 0, out, cyc, rt, Q ? steps / QCH : steps, rnd, queue, 256 * QCH);
    (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
    float ms; (void)hipEventElapsedTime(&ms, e0, e1);
    if (report) {
        std::vector<unsigned long long> hc(256), hr(256);
        (void)hipMemcpy(hc.data(), cyc, 8 * 256, hipMemcpyDeviceToHost);
        (void)hipMemcpy(hr.data(), rt, 8 * 256, hipMemcpyDeviceToHost);
        std::vector<double> clk(256), dur(256);
        double cys = 0;
        for (int b = 0; b < 256; ++b) { clk[b] = (double)hc[b] / (double)hr[b] * 0.1; dur[b] = (double)hr[b] * 1e-5; cys += (double)hc[b]; }
        std::sort(clk.begin(), clk.end()); std::sort(dur.begin(), dur.end());
        const double wg_steps = Q ? (double)(steps / QCH) * QCH : steps;                 // work of the average workgroup
        const double flop = 3.0 * 2.0 * 128 * 64 * 32 * wg_steps * 4 * 256;             // 3 products, 4 waves x 256 workgroups
        const double n32 = 2.0 * 3 * 8 * wg_steps;                                        // 32x32x16-equivalents per wave
        printf("split tile, %s, %s  %7.2f ms: %6.2f cycles per 32x32x16-equivalent, %7.1f TFLOP/s, in-kernel clock min / median / max "
               "%.3f / %.3f / %.3f GHz, workgroup time median / max %.2f / %.2f ms\n",
               S == 32 ? "32x32x16_f16" : "16x16x32_f16", Q ? "queue" : "fixed", ms, cys / 256 / n32, flop / (ms * 1e-3) / 1e12,
               clk[0], clk[128], clk[255], dur[128], dur[255]);
    }
    return ms;
}

int main() {
    float* out; unsigned long long *cyc, *rt; _Float16* rnd;
    (void)hipMalloc(&out, sizeof(float) * 256 * 256);
    int* queue;
    (void)hipMalloc(&cyc, 8 * 256); (void)hipMalloc(&rt, 8 * 256); (void)hipMalloc(&rnd, 2 * 8192); (void)hipMalloc(&queue, sizeof(int));
    std::vector<_Float16> h(8192);
    unsigned s = 12345;
    for (auto& v : h) { s = s * 1664525u + 1013904223u; v = (_Float16)(((int)(s >> 8) - (1 << 23)) * (0.6f / (1 << 23))); }
    (void)hipMemcpy(rnd, h.data(), 2 * 8192, hipMemcpyHostToDevice);
    run<0>("zero operands, one wave per SIMD", 200000, rnd, out, cyc, rt);
    run<1>("random operands, one wave per SIMD", 200000, rnd, out, cyc, rt);
    run<2>("random operands, 3 of 4 issue slots used", 200000, rnd, out, cyc, rt);
    run<3>("random operands, 1 of 2 issue slots used", 200000, rnd, out, cyc, rt);
    // shape comparison: >= 2 s of back-to-back launches, then the two shapes alternate (3 timed launches of each form)
    const int steps = 20000;
    const auto w0 = std::chrono::steady_clock::now();
    for (int i = 0; std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count() < 2.0; ++i)
        (i & 1) ? split_once<16, false>(steps, rnd, out, cyc, rt, queue, false) : split_once<32, false>(steps, rnd, out, cyc, rt, queue, false);
    for (int rep = 0; rep < 3; ++rep) {
        split_once<32, false>(steps, rnd, out, cyc, rt, queue, true);
        split_once<16, false>(steps, rnd, out, cyc, rt, queue, true);
        split_once<32, true>(steps, rnd, out, cyc, rt, queue, true);
        split_once<16, true>(steps, rnd, out, cyc, rt, queue, true);
    }
    return 0;
}
