// sdf_refine.hip -- path A of the hot path: batched DeepSDF object refinement on gfx950.
//
// Replaces reconstruct/optimizer.py:96-281 (Optimizer.reconstruct_object), :47-93 (estimate_pose_cam_obj),
// reconstruct/loss.py:22-178 and reconstruct/loss_utils.py:40-265 of the reference.  One Gauss-Newton iteration of
// EVERY hypothesis in the batch is five launches with no host round trip:
//
//   k_sample      per hypothesis: T_co, scale, depth range; ray x depth samples inside the unit ball (loss.py:60-74)
//   k_mlp_fwd     decoder forward on the valid samples                                  (loss.py:78)
//   k_scan        per ray: occupancy, transmittance, rendered depth, de/ds; keeps rows   (loss.py:84-141)
//   k_mlp_jtj     decoder forward+backward on surface points and kept render rows, Jacobian rows, Huber weights and
//                 the 72x72 augmented normal-equation tile J~^T J~ (J~ = [J | r~]) by MFMA (loss.py:22-43,143-150,
//                 optimizer.py:217-226)
//   k_solve       fixed-order reduction of the tile partials, priors, damping, 71x71 solve, exp_sim3, state update
//                 (optimizer.py:231-263)
//
// (plus k_c0 and k_plan: per-hypothesis bias vectors and the work queues of the two MLP kernels.)  The two MLP kernels exist
// per decoder pipe (qsp_decoder_set_option): k_mlp_fwd<false> / k_mlp_jtj<false> on the exact-f32 matrix pipe, <true> with three
// bf16 terms per operand, k_mlp_fwd_h2 / k_mlp_jtj_h2 with two fp16 terms (four waves per workgroup, sdf_mlp.hpp).
//
// The reference does the same work as ~60 small torch launches and ~10 host synchronisations per iteration,
// per hypothesis, serially.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <string>
#include <mutex>
#include <vector>

#include "../../include/qsp_hip.h"
#include "common.hpp"
#include "sdf_mlp.hpp"

#include "sdf_kernels.hpp"

#ifndef QSP_JTJ_WAVES_DEFAULT
#define QSP_JTJ_WAVES_DEFAULT 8
#endif
#ifndef QSP_SCREEN_WAVES_DEFAULT
#define QSP_SCREEN_WAVES_DEFAULT 4
#endif


// =================================================================================================================
// host side
// =================================================================================================================
using namespace qsp;

struct qsp_decoder {
    int device = 0;
    hipStream_t stream = nullptr;
    MlpParams P{};
    MlpParams* Pd = nullptr;   // device copy, read by the kernels
    std::vector<void*> allocs;
    double mac_per_point = 0;
    int code_len = CODE_LEN;   // the caller's code length L <= 64; the tile always works on 64 (columns L..63 are zero)
    int fwd_bf3 = 0;           // QSP_DEC_OPT_FORWARD_PRECISION: forward-only passes on the split-bf16 pipe (mlp_tile_bf3)
    int jac_bf3 = 0;           // QSP_DEC_OPT_JACOBIAN_PRECISION: the forward+backward pass (mlp_tile<true, .., B3>)
    bool fp16_ok = true;       // every weight of layers 0..7 fits fp16's range (split-fp16 planes are usable)
    int tile_p = 64;           // QSP_DEC_OPT_TILE_POINTS: points per MLP tile of the refinement batches created from now on
    int* range_flag_h = nullptr;   // host-mapped word the split-fp16 kernels set when a value left fp16's range (check_range)
    bool narrow_capable = false;   // the decoder is small enough for the NARROW tile (narrow_tables); QSP_DEC_OPT_NARROW_TILE toggles its use
    float screen_margin = 0.f;     // QSP_DEC_OPT_RENDER_SCREENING: > 0 = two-pass ray-sample forward with this band margin
    int32_t depth_staging = 1;     // QSP_DEC_OPT_DEPTH_STAGING: the screened forward in two depth stages (k_stage_list); same bits
    int32_t screen_audit = 100;    // QSP_DEC_OPT_SCREEN_AUDIT: one in this many OUT-of-band samples is re-evaluated too (0 = off, 1 = all)
    int64_t screen_min_samples = -1;   // QSP_DEC_OPT_SCREENING_MIN_SAMPLES: -1 = more than two rounds of 64-point tiles over the chip
    int range_fallback = 1;        // QSP_DEC_OPT_RANGE_FALLBACK: a call that left fp16's range is repeated on the f32 pipe
    int64_t n_range_fallbacks = 0; // QSP_DEC_CNT_RANGE_FALLBACKS
    int64_t n_screen_fallbacks = 0;    // QSP_DEC_CNT_SCREEN_FALLBACKS: runs repeated in one pass by the screening self-check
    // qsp_reconstruct_objects keeps ONE resident batch per decoder, sized by the high-water mark of the calls so far: the
    // reference's call pattern is one object per call (src/LocalMapping_util.cc:705-760), and creating / destroying ~25 device
    // buffers per call cost ~0.5 ms of a 3 ms call
    // One decoder = one stream, one resident batch (arena) and a few fields that calls rewrite for their own duration (the f32
    // override of a range fallback, the screening margin of a self-check repeat): entry points that launch on the decoder or
    // touch those serialise on this lock -- two host threads sharing a decoder get correct results, one call at a
    // time; threads that want to overlap use a decoder each (the weights are 15 MB).
    std::recursive_mutex mu;
    struct qsp_refine_batch* arena = nullptr;
    int64_t n_arena_reuse = 0, n_arena_create = 0;
};

// A decoder group (qsp_decoder_group_create): an ordered set of decoders, one per class, that the group entry points refine
// together -- every object names its member (ObjView::dec) and the GRP = true forms of the decoder kernels read that member's
// MlpParams from Pd.  The members' options must agree (group_check); the first member lends the group its stream and its
// option fields, and a range fallback / screening repeat of a group call overrides them there.
struct qsp_decoder_group {
    std::vector<qsp_decoder*> m;            // members, class order
    std::vector<qsp_decoder*> lock_order;   // the distinct members by address: a group call takes their locks in this order
    int device = 0;
    MlpParams* Pd = nullptr;                // device copy of the members' MlpParams, class order
    std::vector<MlpParams> Ph;              // what Pd holds (refreshed when a member's parameters change: use_tanh, narrow)
    struct qsp_refine_batch* arena = nullptr;   // the resident batch of qsp_reconstruct_objects_group
    int64_t n_arena_reuse = 0, n_arena_create = 0;
};

// Runs the enclosed call with every decoder pass on the exact-f32 pipe (the range fallback of the split-fp16 modes).
struct F32Override {
    qsp_decoder* d;
    int fwd, jac;
    explicit F32Override(qsp_decoder* d_) : d(d_), fwd(d_->fwd_bf3), jac(d_->jac_bf3) { d->fwd_bf3 = 0; d->jac_bf3 = 0; }
    ~F32Override() { d->fwd_bf3 = fwd; d->jac_bf3 = jac; }
};

// The family deep_sdf/deep_sdf_decoder.py:29-63 builds -- `dims` hidden layers of any width, one (or no) latent_in layer, any
// code length -- mapped EXACTLY onto the one network shape the tile kernels run (8 hidden layers x 512, code 64, skip into layer
// 4), so that specs.json decides the architecture, not the library:
//   * narrower layers: zero rows / columns (a unit with zero weights and zero bias outputs relu(0) = 0 and feeds nothing);
//   * fewer layers: identity layers.  Every hidden activation is a ReLU output, i.e. >= 0, and relu(1 * h + 0) == h bit for
//     bit (the other products of the row are exact zeros); in the backward pass the identity's ReLU mask (h > 0) only removes
//     gradient that the producing layer's own mask (pre-activation > 0, the same condition) removes anyway;
//   * shorter codes: zero code columns; the normal equations keep 64 code unknowns whose extra rows are decoupled (k_solve);
//   * the latent_in layer goes to slot 4, the layers before it to slots 0.., identity layers fill up to slot 3; the
//     layers after it to slots 5.., identity layers fill up to slot 7; the output layer is slot 8.
// Needs: at most 4 hidden layers before and at most 4 from the latent_in layer on, widths <= 512 (<= 445 in front of the skip).
// Cost: the arithmetic of the full 8 x 512 tile whatever the network's own size.
static int embed_family(const qsp_decoder_desc* desc, const std::vector<std::vector<float>>& W,
                        std::vector<std::vector<float>>& Wc, std::vector<std::vector<float>>& Bc, std::vector<int>& src) {
    const int nl = desc->n_layers, m = nl - 1, L = desc->code_len;
    if (nl < 3 || nl > 9 || L < 1 || L > CODE_LEN)
        return qsp_fail(QSP_ERR_UNSUPPORTED, "decoder family: 2..8 hidden layers and a code of 1..64 are supported");
    int s = desc->latent_in_layer;
    const bool has_skip = s >= 0;
    if (!has_skip) {   // no latent_in: any split with <= 4 layers on either side whose front part ends on a layer that fits slot 3
        s = -1;
        for (int c = std::max(1, m - 4); c <= std::min(4, m - 1) && s < 0; ++c)
            if (desc->out_dim[c - 1] >= 1 && desc->out_dim[c - 1] <= SKIP_COL) s = c;
        if (s < 0)
            return qsp_fail(QSP_ERR_UNSUPPORTED, "decoder family: without a latent_in layer one of the hidden layers 1..4 must be "
                                                  "at most 445 wide (it takes the place of the layer in front of the skip)");
    }
    if (s < 1 || s > 4 || s > m - 1 || m - s > 4)
        return qsp_fail(QSP_ERR_UNSUPPORTED, "decoder family: the latent_in layer needs 1..4 hidden layers in front of it and "
                                              "at most 4 from it on");
    if (desc->in_dim[0] != L + 3 || desc->out_dim[m] != 1)
        return qsp_fail(QSP_ERR_UNSUPPORTED, "decoder family: first layer takes [code | xyz], last layer has one output");
    for (int l = 0; l < m; ++l) {
        // canonical slot 3 is 445 wide whether or not the network has a skip connection: the layer in front of slot 4 (or the
        // identity layers that carry its output there) must fit it -- columns 445..511 of slot 4's input are [code | xyz]
        const int lim = (l == s - 1) ? SKIP_COL : HID;
        if (desc->out_dim[l] < 1 || desc->out_dim[l] > lim)
            return qsp_fail(QSP_ERR_UNSUPPORTED, "decoder family: hidden width above 512 (445 in front of the latent_in layer)");
    }
    for (int l = 1; l <= m; ++l) {
        const int expect = desc->out_dim[l - 1] + ((l == s && has_skip) ? L + 3 : 0);
        if (desc->in_dim[l] != expect) return qsp_fail(QSP_ERR_UNSUPPORTED, "decoder family: layer input widths do not chain");
    }
    auto in_c = [](int c) { return c == 0 ? NIN : HID; };
    auto out_c = [](int c) { return c == 8 ? 1 : (c == 3 ? SKIP_COL : HID); };
    Wc.assign(9, std::vector<float>());
    Bc.assign(9, std::vector<float>());
    src.assign(9, -1);                                      // canonical slot -> source layer (-1: identity)
    for (int l = 0; l < s; ++l) src[l] = l;
    for (int l = s; l < m; ++l) src[4 + (l - s)] = l;
    src[8] = m;
    for (int c = 0; c < 9; ++c) {
        const int ic = in_c(c), oc = out_c(c);
        Wc[c].assign((size_t)oc * ic, 0.f);
        Bc[c].assign((size_t)oc, 0.f);
        const int l = src[c];
        if (l < 0) {                                        // identity on the (<= 445 / 512 wide) activation
            for (int r = 0; r < oc; ++r) Wc[c][(size_t)r * ic + r] = 1.f;
            continue;
        }
        const int in = desc->in_dim[l], out = desc->out_dim[l];
        for (int o = 0; o < out; ++o) {
            Bc[c][o] = desc->bias[l][o];
            for (int k = 0; k < in; ++k) {
                int kc = k;
                if (c == 0) kc = (k < L) ? k : CODE_LEN + (k - L);                       // [code L | xyz] -> [code 64 | xyz]
                if (c == 4 && has_skip) {
                    const int w = desc->out_dim[l - 1];                                  // [prev w | code L | xyz]
                    kc = (k < w) ? k : (k < w + L ? SKIP_COL + (k - w) : SKIP_COL + CODE_LEN + (k - w - L));
                }
                Wc[c][(size_t)o * ic + kc] = W[l][(size_t)o * in + k];
            }
        }
    }
    return QSP_OK;
}

// Layer gains.  A ReLU network is positively homogeneous layer by layer: with a_L' = c_L a_L the network
//     W_L' = W_L c_L / c_{L-1},  b_L' = b_L c_L   (layer 4's [code | xyz] columns: W c_4, their input is not a hidden activation),
//     w_8' = w_8 / c_7
// computes the same function, and for c_L a power of two every intermediate of the f32 evaluation is the original one times a power
// of two -- same bits in the result, forward and backward.  The split-fp16 planes hold a value in [6.1e-5, 65504] to 22 bits and
// coarser below: a decoder whose layer gains are skewed (one layer's weights x 1e-4, the next x 1e4: the same function) would put a
// whole layer's activations into fp16's subnormal range.  So every layer whose median row norm -- seen from the rescaled layer in
// front of it -- is outside [2^-8, 2^8] is brought back to ~1 by such a c_L.  Decoders with ordinary gains (every golden and
// fitted one) get c_L = 1 throughout and are packed exactly as before.
static void equalize_gains(std::vector<std::vector<float>>& W, std::vector<std::vector<float>>& B) {
    const int in_dim[9] = {NIN, HID, HID, HID, HID, HID, HID, HID, HID};
    const int out_dim[9] = {HID, HID, HID, SKIP_COL, HID, HID, HID, HID, 1};
    float c_prev = 1.f;
    for (int l = 0; l < 8; ++l) {
        const int in = in_dim[l], out = out_dim[l];
        const int n_hidden = (l == 0) ? 0 : (l == 4 ? SKIP_COL : in);     // input columns that are the previous layer's activations
        std::vector<double> norms;                  // of the rows that exist (embedded narrower layers have zero rows)
        for (int o = 0; o < out; ++o) {
            double ss = 0;
            for (int k = 0; k < in; ++k) {
                const double v = (double)W[l][(size_t)o * in + k] / (k < n_hidden ? (double)c_prev : 1.0);
                ss += v * v;
            }
            if (ss > 0 && std::isfinite(ss)) norms.push_back(sqrt(ss));
        }
        // the MEDIAN row norm: a single outlier row must not push every other row of its layer out of fp16's normal range
        // (an outlier beyond 65 504 is what QSP_ERR_UNSUPPORTED of the split-fp16 mode is for)
        double m = 0;
        if (!norms.empty()) {
            std::nth_element(norms.begin(), norms.begin() + norms.size() / 2, norms.end());
            m = norms[norms.size() / 2];
        }
        float c = 1.f;
        if (m > 0 && (m < 0x1p-8 || m > 0x1p8)) c = (float)ldexp(1.0, -(int)lrint(log2(m)));
        if (c != 1.f || c_prev != 1.f) {
            for (int o = 0; o < out; ++o) {
                for (int k = 0; k < in; ++k) W[l][(size_t)o * in + k] *= (k < n_hidden) ? c / c_prev : c;
                B[l][o] *= c;
            }
        }
        c_prev = c;
    }
    if (c_prev != 1.f)
        for (int k = 0; k < HID; ++k) W[8][k] /= c_prev;
}

// What the NARROW form of the split-fp16 tile may skip (MlpParams::skip / ks_in / ks_out / ncb_in / ncb_out), read off the embedded
// matrices themselves: a slot is skipped when embed_family made it an identity; an input slab / output block "exists" up to the
// last column / row that carries a non-zero weight or bias.  `narrow` is set when the multiply-adds that remain are less than
// half of the full shape's: only then the narrow kernels (no hand-over of weight fragments between layers, idle waves) pay.
static void narrow_tables(qsp_decoder* d, const std::vector<std::vector<float>>& W, const std::vector<std::vector<float>>& B,
                          const std::vector<int>& src) {
    const int in_dim[9] = {NIN, HID, HID, HID, HID, HID, HID, HID, HID};
    const int out_dim[9] = {HID, HID, HID, SKIP_COL, HID, HID, HID, HID, 1};
    auto even4 = [](int v, int cap) { v = std::max(4, (v + 1) & ~1); return std::min(v, cap); };
    double macs = 0, full = 0;
    for (int l = 0; l < 8; ++l) {
        const int in = in_dim[l], out = out_dim[l];
        const int n_hidden = (l == 0) ? 0 : (l == 4 ? SKIP_COL : in);        // input columns that are hidden activations
        int w_out = 0, w_in = 0;
        for (int o = 0; o < out; ++o) {
            bool any = B[l][o] != 0.f;
            for (int k = 0; k < in; ++k)
                if (W[l][(size_t)o * in + k] != 0.f) {
                    any = true;
                    if (k < n_hidden) w_in = std::max(w_in, k + 1);
                }
            if (any) w_out = o + 1;
        }
        const bool skip = src[l] < 0;
        d->P.skip[l] = skip ? 1 : 0;
        const int ks_cap = (l == 4) ? K4 / 16 : HID / 16;
        int ks_in = even4((w_in + 15) / 16, ks_cap);
        if (l == 4 && ks_in >= K4 / 16 - 1) ks_in = K4 / 16;               // (the xyz slab is the last one: no gap left to skip)
        d->P.ks_in[l] = (uint8_t)ks_in;
        d->P.ks_out[l] = (uint8_t)even4((w_out + 15) / 16, HID / 16);
        d->P.ncb_in[l] = (uint8_t)std::max(1, (w_in + 31) / 32);
        d->P.ncb_out[l] = (uint8_t)std::max(1, (w_out + 31) / 32);
        full += (double)in * out;
        if (!skip) macs += (double)(l == 0 ? in : 16 * ks_in + (l == 4 ? NIN : 0)) * (32.0 * d->P.ncb_out[l]);
    }
    d->narrow_capable = macs < 0.5 * full;
    d->P.narrow = d->narrow_capable ? 1 : 0;
}

static inline uint16_t bf16_rne(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);       // NaN stays NaN
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
static inline float bf16_f32(uint16_t b) {
    const uint32_t u = (uint32_t)b << 16;
    float x;
    memcpy(&x, &u, 4);
    return x;
}
// x = hi + mid + lo, each a bf16: 8 + 8 + 8 mantissa bits
static inline void bf16_split3(float v, uint16_t& hi, uint16_t& mid, uint16_t& lo) {
    hi = bf16_rne(v);
    const float r1 = v - bf16_f32(hi);
    mid = bf16_rne(r1);
    const float r2 = r1 - bf16_f32(mid);
    lo = bf16_rne(r2);
}

static int pack_weights(qsp_decoder* d, const qsp_decoder_desc* desc) {
    if (desc->n_layers < 1 || desc->n_layers > 64) return qsp_fail(QSP_ERR_UNSUPPORTED, "decoder family: layer count");
    // fold weight norm:  W = g * v / ||v||_row   (torch.nn.utils.weight_norm, dim=0)
    std::vector<std::vector<float>> Wsrc(desc->n_layers);
    for (int l = 0; l < desc->n_layers; ++l) {
        const int in = desc->in_dim[l], out = desc->out_dim[l];
        if (in < 1 || out < 1 || in > 4096 || out > 4096 || !desc->weight[l] || !desc->bias[l])
            return qsp_fail(QSP_ERR_UNSUPPORTED, "decoder family: layer dims");
        Wsrc[l].assign((size_t)out * in, 0.f);
        const float* v = desc->weight[l];
        const float* g = (desc->weight_g && desc->weight_g[l]) ? desc->weight_g[l] : nullptr;
        for (int o = 0; o < out; ++o) {
            float sc = 1.f;
            if (g) {
                float ss = 0.f;
                for (int k = 0; k < in; ++k) ss += v[(size_t)o * in + k] * v[(size_t)o * in + k];
                sc = g[o] / sqrtf(ss);
            }
            for (int k = 0; k < in; ++k) Wsrc[l][(size_t)o * in + k] = v[(size_t)o * in + k] * sc;
        }
        d->mac_per_point += (double)in * out;
    }
    std::vector<std::vector<float>> W, Bias;
    std::vector<int> slot_src;
    {
        const int rc = embed_family(desc, Wsrc, W, Bias, slot_src);
        if (rc) return rc;
    }
    d->code_len = desc->code_len;
    equalize_gains(W, Bias);
    narrow_tables(d, W, Bias, slot_src);
    // from here on: the canonical 9-layer shape
    const int in_dim[9] = {NIN, HID, HID, HID, HID, HID, HID, HID, HID};
    const int out_dim[9] = {HID, HID, HID, SKIP_COL, HID, HID, HID, HID, 1};
    auto upload = [&](const std::vector<float>& h, const void** dst) -> int {
        void* p = nullptr;
        QSP_HIP(hipMalloc(&p, h.size() * sizeof(float) + 16384));   // + prefetch over-read slack (gemm_2x2)
        d->allocs.push_back(p);
        QSP_HIP(hipMemcpy(p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
        *dst = p;
        return QSP_OK;
    };
    for (int l = 0; l < 8; ++l) {
        const int in = in_dim[l], out = out_dim[l];
        int rc = QSP_OK;
        if (l == 0) {
            // layer 0 is evaluated directly (mlp_prepare + mlp_tile): code columns [k][unit], xyz columns per unit quad
            std::vector<float> wc((size_t)HID * CODE_LEN), wx((size_t)(HID / 4) * 3 * 4);
            for (int o = 0; o < HID; ++o)
                for (int k = 0; k < CODE_LEN; ++k) wc[(size_t)k * HID + o] = W[0][(size_t)o * in + k];     // [k][unit]: code_bias
            for (int q = 0; q < HID / 4; ++q)
                for (int a = 0; a < 3; ++a)
                    for (int e = 0; e < 4; ++e) wx[((size_t)q * 3 + a) * 4 + e] = W[0][(size_t)(4 * q + e) * in + CODE_LEN + a];
            rc = upload(wc, (const void**)&d->P.w0c);
            if (!rc) rc = upload(wx, (const void**)&d->P.w0x);
            d->P.wf[0] = nullptr;
            d->P.wf3[0] = nullptr;
            if (!rc) {   // split-fp16: the xyz columns as one slab of the forward product (gemm_l0_h2): k = 0..2 used of 16
                std::vector<_Float16> ph((size_t)16 * 2 * 64 * 8, (_Float16)0.f);
                for (int cb = 0; cb < 16; ++cb)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 8; ++j) {
                            const int o = 32 * cb + (lane & 31), k = 8 * (lane >> 5) + j;
                            float v = 0.f;
                            if (o < out && k < 3) v = W[0][(size_t)o * in + CODE_LEN + k];
                            if (!(fabsf(v) < 65000.f)) d->fp16_ok = false;
                            const _Float16 hi = (_Float16)v;
                            const size_t base = ((size_t)cb * 2) * 64 * 8 + (size_t)lane * 8 + j;
                            ph[base] = hi;
                            ph[base + 64 * 8] = (_Float16)((v - (float)hi) * 2048.f);
                        }
                void* phd = nullptr;
                QSP_HIP(hipMalloc(&phd, ph.size() * sizeof(_Float16) + 16384));
                d->allocs.push_back(phd);
                QSP_HIP(hipMemcpy(phd, ph.data(), ph.size() * sizeof(_Float16), hipMemcpyHostToDevice));
                d->P.wfh[0] = (const float4*)phd;
            }
        } else {
            // forward: B[k][o]; column blocks over o (16 blocks of 32), k-groups of 8 over K = 512.
            // Layer 4 (latent_in): K = 448 = [h3 (445) | xyz (3)]; its 64 code columns go to w4c (folded into a bias per
            // hypothesis by k_c0 / mlp_prepare).
            const int KG = (l == 4) ? KG4 : HID / 8;
            std::vector<float> pf((size_t)16 * KG * 64 * 4, 0.f);
            for (int cb = 0; cb < 16; ++cb)
                for (int kg = 0; kg < KG; ++kg)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int e = 0; e < 4; ++e) {
                            const int o = 32 * cb + (lane & 31);
                            int k = 8 * kg + 4 * (lane >> 5) + e;
                            if (l == 4 && k >= SKIP_COL) k += CODE_LEN;      // xyz columns 509..511
                            float v = 0.f;
                            if (o < out && k < in) v = W[l][(size_t)o * in + k];
                            pf[(((size_t)cb * KG + kg) * 64 + lane) * 4 + e] = v;
                        }
            rc = upload(pf, (const void**)&d->P.wf[l]);
            if (!rc) {
                // split-bf16 planes for mlp_tile_bf3: [col block][slab of 16 k][plane][lane][8 bf16]; lane (r, h) holds
                // W[unit 32 cb + r][k = 16 s + 8 h + j] (the A-operand map of v_mfma_f32_32x32x16_bf16)
                const int KS = KG / 2;
                std::vector<uint16_t> p3((size_t)16 * KS * 3 * 64 * 8, 0);
                for (int cb = 0; cb < 16; ++cb)
                    for (int ks = 0; ks < KS; ++ks)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int j = 0; j < 8; ++j) {
                                const int o = 32 * cb + (lane & 31);
                                int k = 16 * ks + 8 * (lane >> 5) + j;
                                if (l == 4 && k >= SKIP_COL) k += CODE_LEN;
                                float v = 0.f;
                                if (o < out && k < in) v = W[l][(size_t)o * in + k];
                                uint16_t hi, mid, lo;
                                bf16_split3(v, hi, mid, lo);
                                const size_t base = (((size_t)cb * KS + ks) * 3) * 64 * 8 + (size_t)lane * 8 + j;
                                p3[base] = hi;
                                p3[base + 64 * 8] = mid;
                                p3[base + 2 * 64 * 8] = lo;
                            }
                void* p3d = nullptr;
                QSP_HIP(hipMalloc(&p3d, p3.size() * sizeof(uint16_t) + 16384));
                d->allocs.push_back(p3d);
                QSP_HIP(hipMemcpy(p3d, p3.data(), p3.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
                d->P.wf3[l] = (const float4*)p3d;
            }
            if (!rc) {
                // split-fp16 planes for mlp_tile_h2: [col block][slab of 16 k][hi | lo' = (w - hi) 2^11][lane][8 fp16], same lane map
                const int KS = KG / 2;
                std::vector<_Float16> ph((size_t)16 * KS * 2 * 64 * 8, (_Float16)0.f);
                for (int cb = 0; cb < 16; ++cb)
                    for (int ks = 0; ks < KS; ++ks)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int j = 0; j < 8; ++j) {
                                const int o = 32 * cb + (lane & 31);
                                int k = 16 * ks + 8 * (lane >> 5) + j;
                                if (l == 4 && k >= SKIP_COL) k += CODE_LEN;
                                float v = 0.f;
                                if (o < out && k < in) v = W[l][(size_t)o * in + k];
                                if (!(fabsf(v) < 65000.f)) d->fp16_ok = false;
                                const _Float16 hi = (_Float16)v;
                                const _Float16 lo = (_Float16)((v - (float)hi) * 2048.f);
                                const size_t base = (((size_t)cb * KS + ks) * 2) * 64 * 8 + (size_t)lane * 8 + j;
                                ph[base] = hi;
                                ph[base + 64 * 8] = lo;
                            }
                void* phd = nullptr;
                QSP_HIP(hipMalloc(&phd, ph.size() * sizeof(_Float16) + 16384));
                d->allocs.push_back(phd);
                QSP_HIP(hipMemcpy(phd, ph.data(), ph.size() * sizeof(_Float16), hipMemcpyHostToDevice));
                d->P.wfh[l] = (const float4*)phd;
            }
            if (!rc && l == 4) {
                std::vector<float> wc((size_t)HID * CODE_LEN);
                for (int o = 0; o < HID; ++o)
                    for (int k = 0; k < CODE_LEN; ++k) wc[(size_t)k * HID + o] = W[4][(size_t)o * in + SKIP_COL + k];
                rc = upload(wc, (const void**)&d->P.w4c);
            }
        }
        if (rc) return rc;
        // backward: B[o][k]; column blocks over the layer's inputs k, groups of 8 over o (padded to 512)
        const int NCB = (l == 0) ? 3 : 16;
        const int OG = HID / 8;
        std::vector<float> pb((size_t)NCB * OG * 64 * 4, 0.f);
        for (int cb = 0; cb < NCB; ++cb)
            for (int og = 0; og < OG; ++og)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 4; ++e) {
                        const int k = 32 * cb + (lane & 31);
                        const int o = 8 * og + 4 * (lane >> 5) + e;
                        float v = 0.f;
                        if (o < out && k < in) v = W[l][(size_t)o * in + k];
                        pb[(((size_t)cb * OG + og) * 64 + lane) * 4 + e] = v;
                    }
        rc = upload(pb, (const void**)&d->P.wb[l]);
        if (rc) return rc;
        {   // split-bf16 planes of the same matrix: [col block over inputs k][slab of 16 outputs o][plane][lane][8 bf16]
            const int KS = HID / 16;
            std::vector<uint16_t> p3((size_t)NCB * KS * 3 * 64 * 8, 0);
            for (int cb = 0; cb < NCB; ++cb)
                for (int ks = 0; ks < KS; ++ks)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 8; ++j) {
                            const int k = 32 * cb + (lane & 31);
                            const int o = 16 * ks + 8 * (lane >> 5) + j;
                            float v = 0.f;
                            if (o < out && k < in) v = W[l][(size_t)o * in + k];
                            uint16_t hi, mid, lo;
                            bf16_split3(v, hi, mid, lo);
                            const size_t base = (((size_t)cb * KS + ks) * 3) * 64 * 8 + (size_t)lane * 8 + j;
                            p3[base] = hi;
                            p3[base + 64 * 8] = mid;
                            p3[base + 2 * 64 * 8] = lo;
                        }
            void* p3d = nullptr;
            QSP_HIP(hipMalloc(&p3d, p3.size() * sizeof(uint16_t) + 16384));
            d->allocs.push_back(p3d);
            QSP_HIP(hipMemcpy(p3d, p3.data(), p3.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
            d->P.wb3[l] = (const float4*)p3d;
        }
        {   // split-fp16 planes of the same matrix: [col block over inputs k][slab of 16 outputs o][hi | lo'][lane][8 fp16].
            // Layer 7's is diag(w8) W7: the split tile's backward seed is then the 0/1 ReLU mask of layer 7 (mlp_tile_h2).  (The gain
            // equalisation scales W7's rows by c and w8 by 1 / c, so this product is what it was; small products may land among
            // fp16 subnormals, where the split still bounds the absolute error by ~2^-36.)
            const int KS = HID / 16;
            std::vector<_Float16> ph((size_t)NCB * KS * 2 * 64 * 8, (_Float16)0.f);
            for (int cb = 0; cb < NCB; ++cb)
                for (int ks = 0; ks < KS; ++ks)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 8; ++j) {
                            const int k = 32 * cb + (lane & 31);
                            const int o = 16 * ks + 8 * (lane >> 5) + j;
                            float v = 0.f;
                            if (o < out && k < in) v = l == 7 ? (float)((double)W[8][o] * W[l][(size_t)o * in + k]) : W[l][(size_t)o * in + k];
                            if (!(fabsf(v) < 65000.f)) d->fp16_ok = false;
                            const _Float16 hi = (_Float16)v;
                            const size_t base = (((size_t)cb * KS + ks) * 2) * 64 * 8 + (size_t)lane * 8 + j;
                            ph[base] = hi;
                            ph[base + 64 * 8] = (_Float16)((v - (float)hi) * 2048.f);
                        }
            void* phd = nullptr;
            QSP_HIP(hipMalloc(&phd, ph.size() * sizeof(_Float16) + 16384));
            d->allocs.push_back(phd);
            QSP_HIP(hipMemcpy(phd, ph.data(), ph.size() * sizeof(_Float16), hipMemcpyHostToDevice));
            d->P.wbh[l] = (const float4*)phd;
        }
        std::vector<float> bias(HID, 0.f);
        for (int o = 0; o < out; ++o) bias[o] = Bias[l][o];
        rc = upload(bias, (const void**)&d->P.bias[l]);
        if (rc) return rc;
    }
    {   // layer 4's skip columns (inputs 445..511 = [code | xyz]) as their own backward matrix, packed like wbh[0]:
        // [col block over ci = input - 445 (3 blocks, 67 used)][slab of 16 outputs o][hi | lo'][lane][8 fp16]
        const int KS = HID / 16, in4 = in_dim[4], out4 = out_dim[4];
        std::vector<_Float16> ph((size_t)3 * KS * 2 * 64 * 8, (_Float16)0.f);
        for (int cb = 0; cb < 3; ++cb)
            for (int ks = 0; ks < KS; ++ks)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int ci = 32 * cb + (lane & 31);
                        const int o = 16 * ks + 8 * (lane >> 5) + j;
                        float v = 0.f;
                        if (o < out4 && ci < NIN) v = W[4][(size_t)o * in4 + SKIP_COL + ci];
                        const _Float16 hi = (_Float16)v;
                        const size_t base = (((size_t)cb * KS + ks) * 2) * 64 * 8 + (size_t)lane * 8 + j;
                        ph[base] = hi;
                        ph[base + 64 * 8] = (_Float16)((v - (float)hi) * 2048.f);
                    }
        void* phd = nullptr;
        QSP_HIP(hipMalloc(&phd, ph.size() * sizeof(_Float16) + 16384));
        d->allocs.push_back(phd);
        QSP_HIP(hipMemcpy(phd, ph.data(), ph.size() * sizeof(_Float16), hipMemcpyHostToDevice));
        d->P.wbh4s = (const float4*)phd;
    }
    std::vector<float> w8(W[8].begin(), W[8].end());
    int rc = upload(w8, (const void**)&d->P.w8);
    if (rc) return rc;
    d->P.b8 = Bias[8][0];
    QSP_HIP(hipHostMalloc((void**)&d->range_flag_h, sizeof(int), hipHostMallocMapped));
    *d->range_flag_h = 0;
    QSP_HIP(hipHostGetDevicePointer((void**)&d->P.range_flag, d->range_flag_h, 0));
    void* pd = nullptr;
    QSP_HIP(hipMalloc(&pd, sizeof(MlpParams)));
    d->allocs.push_back(pd);
    QSP_HIP(hipMemcpy(pd, &d->P, sizeof(MlpParams), hipMemcpyHostToDevice));
    d->Pd = (MlpParams*)pd;
    return QSP_OK;
}

// after a synchronisation of the decoder's stream: did a split-fp16 kernel meet a value it cannot represent?  (clears the flag)
static bool range_hit(qsp_decoder* d) {
    if (d->range_flag_h && *d->range_flag_h) {
        *d->range_flag_h = 0;
        return true;
    }
    return false;
}
static int range_error() {
    return qsp_fail(QSP_ERR_UNSUPPORTED, "split fp16: an activation or gradient of this decoder left fp16's range (65504); "
                                         "use the split-bf16 or f32 precision for it, or leave QSP_DEC_OPT_RANGE_FALLBACK on");
}
// What a call does when range_hit(): with the fallback on (default) and a split-fp16 pass in use, the caller repeats itself
// under an F32Override and counts it; otherwise the call fails.  The reference never fails a call for a numeric condition
// (reconstruct/optimizer.py:161-194 returns is_good = False at worst), so neither does the default configuration.
static bool range_should_fall_back(qsp_decoder* d) { return d->range_fallback && (d->fwd_bf3 == 2 || d->jac_bf3 == 2); }
static int check_range(qsp_decoder* d) { return range_hit(d) ? range_error() : QSP_OK; }

// Waves per workgroup of the split-fp16 Jacobian kernel: 4 (one 512-register wave per SIMD) or 8 (two 256-register waves per
// SIMD).  QSP_JTJ_WAVES overrides the default for same-box A/B measurements (tools/ab_bench.sh); likewise QSP_SCREEN_WAVES for the
// screening pass and QSP_JTJ_WAVES_T32 for the Jacobian kernel on 32-point tiles.  Each is read once per process.
static int env_waves(const char* name, int dflt) {
    const char* e = getenv(name);
    const int v = e ? atoi(e) : 0;
    return (v == 4 || v == 8) ? v : dflt;
}
static int jtj_waves() { static const int w = env_waves("QSP_JTJ_WAVES", QSP_JTJ_WAVES_DEFAULT); return w; }
static int screen_waves() { static const int w = env_waves("QSP_SCREEN_WAVES", QSP_SCREEN_WAVES_DEFAULT); return w; }
static int jtj_waves_t32() { static const int w = env_waves("QSP_JTJ_WAVES_T32", 4); return w; }

// A launch form: one instantiation of a decoder kernel together with the block size and the dynamic-LDS bytes it must be
// launched with.  The three are written down once, in the family helpers below -- the block size from the template arguments
// that fix it, the LDS bytes from the type the kernel body casts its dynamic LDS to -- and travel together from there:
// launch() is the only place that starts a decoder kernel, mlp_attr_once() the only one that raises an LDS limit.
template <class... A> struct Form { void (*fn)(A...); int threads; int lds; };
template <class Smem, class... A> static Form<A...> form(void (*fn)(A...), int threads) { return {fn, threads, (int)sizeof(Smem)}; }
template <class... A, class... B> static void launch(const Form<A...>& f, int grid, hipStream_t s, const B&... args) {
    hipLaunchKernelGGL(f.fn, dim3(grid), dim3(f.threads), f.lds, s, static_cast<A>(args)...);
}

// The instantiations that exist, each named once per family: its single-decoder form, or for a decoder group's batch (grp) the
// form that reads every work item's decoder from the group's parameter array.
template <bool BF3> static auto fwd_kernel(bool grp) { return form<MlpSmem>(grp ? k_mlp_fwd<BF3, true> : k_mlp_fwd<BF3, false>, MLP_THREADS); }
template <int NW> static auto fwd_h1_kernel(bool grp) { return form<MlpSmemH1>(grp ? k_mlp_fwd_h1<NW, true> : k_mlp_fwd_h1<NW, false>, 64 * NW); }
template <int NR, bool NARROW, int NW> static auto fwd_h2_kernel(bool grp) {
    return form<MlpSmem>(grp ? k_mlp_fwd_h2<NR, NARROW, NW, true> : k_mlp_fwd_h2<NR, NARROW, NW, false>, 64 * NW);
}
template <bool B3> static auto jtj_kernel(bool grp) { return form<MlpSmem>(grp ? k_mlp_jtj<B3, true> : k_mlp_jtj<B3, false>, MLP_THREADS); }
template <int NR, int NW, bool NARROW> static auto jtj_h2_kernel(bool grp) {
    return form<MlpSmem>(grp ? k_mlp_jtj_h2<NR, NW, NARROW, true> : k_mlp_jtj_h2<NR, NW, NARROW, false>, 64 * NW);
}
template <bool GRAD, bool BF3> static auto decode_kernel() { return form<MlpSmem>(k_decode<GRAD, BF3>, MLP_THREADS); }
template <bool GRAD, bool NARROW> static auto decode_h2_kernel() { return form<MlpSmem>(k_decode_h2<GRAD, NARROW>, H2_THREADS); }
template <int NW> static auto decode_screen_kernel() { return form<MlpSmemH1>(k_decode_screen<NW>, 64 * NW); }
template <bool BF3> static auto grid_decode_kernel() { return form<MlpSmem>(k_grid_decode<BF3>, MLP_THREADS); }
template <bool NARROW> static auto grid_decode_h2_kernel() { return form<MlpSmem>(k_grid_decode_h2<NARROW>, H2_THREADS); }
template <bool BF3> static auto group_grid_decode_kernel() { return form<MlpSmem>(k_group_grid_decode<BF3>, MLP_THREADS); }
template <bool NARROW> static auto group_grid_decode_h2_kernel() { return form<MlpSmem>(k_group_grid_decode_h2<NARROW>, H2_THREADS); }
static auto scan_kernel() { return form<float[SCAN_RAYS * SCAN_LD]>(k_scan, SCAN_RAYS); }

// The selectors: which form a pass takes, from the decoder's settings.  A selector returns one family's Form type, so the
// passes that span two families (exact-f32 / split-bf16 against split-fp16: different argument lists) have one per family and
// the caller asks `precision == 2` first.  mlp_attr_once() walks each selector's whole domain.
//
// one-pass forward
static auto fwd_form(int bf3, bool grp) { return bf3 ? fwd_kernel<true>(grp) : fwd_kernel<false>(grp); }
// split-fp16 forward: the one-pass kernel, and (narrow = false) the band pass of the screening pair
static auto fwd_h2_form(bool narrow, bool grp) { return narrow ? fwd_h2_kernel<2, true, 8>(grp) : fwd_h2_kernel<2, false, 4>(grp); }
// the one-product pass of the screening pair; waves = screen_waves()
static auto screen_form(int waves, bool grp) { return waves == 8 ? fwd_h1_kernel<8>(grp) : fwd_h1_kernel<4>(grp); }
static auto jtj_form(int bf3, bool grp) { return bf3 ? jtj_kernel<true>(grp) : jtj_kernel<false>(grp); }
// split-fp16 Jacobian: eight waves of 256 registers (two per SIMD) or four of 512 (one per SIMD): same arithmetic, same bits;
// waves = jtj_waves(), waves_t32 = jtj_waves_t32()
// (32-point tiles are the latency option -- one tile deep: there the four-wave form is the shorter chain, 180 us against 248 per
//  tile; QSP_JTJ_WAVES_T32=8 selects the other for measurements)
static auto jtj_h2_form(bool narrow, int tile_p, int waves, int waves_t32, bool grp) {
    if (narrow && tile_p == 32) return jtj_h2_kernel<1, 8, true>(grp);      // narrow decoders: eight waves, so that the column
    if (narrow) return jtj_h2_kernel<2, 8, true>(grp);                      // blocks that exist spread over all SIMDs
    if (tile_p == 32 && waves_t32 == 8) return jtj_h2_kernel<1, 8, false>(grp);
    if (tile_p == 32) return jtj_h2_kernel<1, 4, false>(grp);
    if (waves == 8) return jtj_h2_kernel<2, 8, false>(grp);
    return jtj_h2_kernel<2, 4, false>(grp);
}
// qsp_decode_sdf / qsp_sdf_value_grad; bf3 = the precision of the pass (Jacobian with grad, else forward)
static auto decode_form(bool grad, int bf3, bool narrow) {
    if (bf3 == 2 && narrow) return grad ? decode_h2_kernel<true, true>() : decode_h2_kernel<false, true>();
    if (bf3 == 2) return grad ? decode_h2_kernel<true, false>() : decode_h2_kernel<false, false>();
    if (bf3) return grad ? decode_kernel<true, true>() : decode_kernel<false, true>();
    return grad ? decode_kernel<true, false>() : decode_kernel<false, false>();
}
// the mesh extractor's volumes, one or many: the forward forms of decode_form, over one grid and n_vol codes; bf3 = the forward precision
static auto grid_decode_form(int bf3, bool narrow) {
    if (bf3 == 2) return narrow ? grid_decode_h2_kernel<true>() : grid_decode_h2_kernel<false>();
    return bf3 ? grid_decode_kernel<true>() : grid_decode_kernel<false>();
}
// the same over a decoder group: one class index per volume more in the argument list, so a selector of its own
static auto group_grid_decode_form(int bf3, bool narrow) {
    if (bf3 == 2) return narrow ? group_grid_decode_h2_kernel<true>() : group_grid_decode_h2_kernel<false>();
    return bf3 ? group_grid_decode_kernel<true>() : group_grid_decode_kernel<false>();
}
static auto decode_screen_form(int waves) { return waves == 8 ? decode_screen_kernel<8>() : decode_screen_kernel<4>(); }

// Raises the dynamic-LDS limit of every form a selector can return (once per process): a form that can be launched cannot be
// missing here.
static int mlp_attr_once() {
    static bool done = false;
    if (done) return QSP_OK;
    const auto raise = [](const auto& f) {
        return hipFuncSetAttribute((const void*)f.fn, hipFuncAttributeMaxDynamicSharedMemorySize, f.lds);
    };
    for (const bool grp : {false, true}) {
        for (const int bf3 : {0, 1}) {
            QSP_HIP(raise(fwd_form(bf3, grp)));
            QSP_HIP(raise(jtj_form(bf3, grp)));
        }
        for (const int waves : {4, 8}) QSP_HIP(raise(screen_form(waves, grp)));
        for (const bool narrow : {false, true}) {
            QSP_HIP(raise(fwd_h2_form(narrow, grp)));
            for (const int tile_p : {32, 64})
                for (const int waves : {4, 8})
                    for (const int waves_t32 : {4, 8}) QSP_HIP(raise(jtj_h2_form(narrow, tile_p, waves, waves_t32, grp)));
        }
    }
    QSP_HIP(raise(scan_kernel()));
    for (const bool grad : {false, true})
        for (const int bf3 : {0, 1, 2})
            for (const bool narrow : {false, true}) QSP_HIP(raise(decode_form(grad, bf3, narrow)));
    for (const int waves : {4, 8}) QSP_HIP(raise(decode_screen_form(waves)));
    for (const int bf3 : {0, 1, 2})
        for (const bool narrow : {false, true}) {
            QSP_HIP(raise(grid_decode_form(bf3, narrow)));
            QSP_HIP(raise(group_grid_decode_form(bf3, narrow)));
        }
    done = true;
    return QSP_OK;
}

extern "C" int qsp_decoder_create(const qsp_decoder_desc* desc, int device, qsp_decoder** out) {
    if (!desc || !out || !desc->in_dim || !desc->out_dim || !desc->weight || !desc->bias)
        return qsp_fail(QSP_ERR_INVALID, "qsp_decoder_create: null argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return qsp_fail(QSP_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n) return qsp_fail(QSP_ERR_INVALID, "device index out of range");
    QSP_HIP(hipSetDevice(device));
    qsp_decoder* d = new qsp_decoder();
    d->device = device;
    int rc = mlp_attr_once();
    if (!rc) rc = pack_weights(d, desc);
    if (!rc) {
        hipError_t e = hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking);
        if (e != hipSuccess) rc = qsp_fail(QSP_ERR_DEVICE, hipGetErrorString(e));
    }
    if (rc) {
        qsp_decoder_destroy(d);
        return rc;
    }
    *out = d;
    return QSP_OK;
}

extern "C" int qsp_decoder_set_option(qsp_decoder* d, int32_t option, int32_t value) {
    std::unique_lock<std::recursive_mutex> lk_d;
    if (d) lk_d = std::unique_lock<std::recursive_mutex>(d->mu);
    if (!d) return qsp_fail(QSP_ERR_INVALID, "qsp_decoder_set_option: null decoder");
    switch (option) {
        case QSP_DEC_OPT_FORWARD_PRECISION:
            if (value < 0 || value > 2) return qsp_fail(QSP_ERR_INVALID, "forward precision: 0 (f32 MFMA), 1 (split bf16) or 2 (split fp16)");
            if (value == 2 && !d->fp16_ok) return qsp_fail(QSP_ERR_UNSUPPORTED, "split fp16: a weight of this decoder is outside fp16's range");
            d->fwd_bf3 = value;
            if (value != 2) d->screen_margin = 0.f;      // (the screened forward pass exists on the split-fp16 pipe only)
            return QSP_OK;
        case QSP_DEC_OPT_JACOBIAN_PRECISION:
            if (value < 0 || value > 2) return qsp_fail(QSP_ERR_INVALID, "jacobian precision: 0 (f32 MFMA), 1 (split bf16) or 2 (split fp16)");
            if (value == 2 && !d->fp16_ok) return qsp_fail(QSP_ERR_UNSUPPORTED, "split fp16: a weight of this decoder is outside fp16's range");
            d->jac_bf3 = value;
            return QSP_OK;
        case QSP_DEC_OPT_TILE_POINTS:
            if (value != 32 && value != 64) return qsp_fail(QSP_ERR_INVALID, "tile points: 64 (default) or 32");
            d->tile_p = value;
            return QSP_OK;
        case QSP_DEC_OPT_RENDER_SCREENING:
            if (value < 0 || value > 50000) return qsp_fail(QSP_ERR_UNSUPPORTED, "render screening: margin in 1e-6 units, 0 (off) .. 50000");
            if (value > 0 && d->fwd_bf3 != 2)
                return qsp_fail(QSP_ERR_UNSUPPORTED, "render screening exists on the split-fp16 forward pass only: set "
                                                     "QSP_DEC_OPT_FORWARD_PRECISION to 2 first");
            d->screen_margin = 1e-6f * (float)value;
            return QSP_OK;
        case QSP_DEC_OPT_DEPTH_STAGING:
            if (value < 0 || value > 2) return qsp_fail(QSP_ERR_INVALID, "depth staging: 0 (off), 1 (large batches) or 2 (always)");
            d->depth_staging = (int32_t)value;
            return QSP_OK;
        case QSP_DEC_OPT_SCREEN_AUDIT:
            if (value < 0 || value > 1000000) return qsp_fail(QSP_ERR_INVALID, "screening audit: one in N out-of-band samples, N = 0 (off) .. 1e6");
            d->screen_audit = (int32_t)value;
            return QSP_OK;
        case QSP_DEC_OPT_SCREENING_MIN_SAMPLES:
            if (value < -1) return qsp_fail(QSP_ERR_INVALID, "screening threshold: -1 (automatic) or a sample count >= 0");
            d->screen_min_samples = value;
            return QSP_OK;
        case QSP_DEC_OPT_NARROW_TILE: {
            if (value != 0 && value != 1) return qsp_fail(QSP_ERR_INVALID, "narrow tile: 0 or 1");
            if (value && !d->narrow_capable) return qsp_fail(QSP_ERR_UNSUPPORTED, "narrow tile: this decoder fills most of the 8 x 512 shape");
            d->P.narrow = value;
            QSP_HIP(hipSetDevice(d->device));
            QSP_HIP(hipStreamSynchronize(d->stream));
            QSP_HIP(hipMemcpy(d->Pd, &d->P, sizeof(MlpParams), hipMemcpyHostToDevice));
            return QSP_OK;
        }
        case QSP_DEC_OPT_USE_TANH: {
            if (value != 0 && value != 1) return qsp_fail(QSP_ERR_INVALID, "use_tanh: 0 or 1");
            d->P.use_tanh = value;
            QSP_HIP(hipSetDevice(d->device));
            QSP_HIP(hipStreamSynchronize(d->stream));
            QSP_HIP(hipMemcpy(d->Pd, &d->P, sizeof(MlpParams), hipMemcpyHostToDevice));
            return QSP_OK;
        }
        case QSP_DEC_OPT_RANGE_FALLBACK:
            if (value != 0 && value != 1) return qsp_fail(QSP_ERR_INVALID, "range fallback: 0 or 1");
            d->range_fallback = value;
            return QSP_OK;
        default: return qsp_fail(QSP_ERR_INVALID, "qsp_decoder_set_option: unknown option");
    }
}

extern "C" int64_t qsp_decoder_get_counter(qsp_decoder* d, int32_t counter) {
    if (!d) return -1;
    switch (counter) {
        case QSP_DEC_CNT_RANGE_FALLBACKS: return d->n_range_fallbacks;
        case QSP_DEC_CNT_ARENA_REUSED: return d->n_arena_reuse;
        case QSP_DEC_CNT_ARENA_CREATED: return d->n_arena_create;
        case QSP_DEC_CNT_NARROW_TILE: return d->P.narrow ? 1 : 0;
        case QSP_DEC_CNT_SCREEN_FALLBACKS: return d->n_screen_fallbacks;
        default: return -1;
    }
}

static void batch_free(struct qsp_refine_batch* b);
extern "C" void qsp_decoder_destroy(qsp_decoder* d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    if (d->arena) batch_free(d->arena);
    d->arena = nullptr;
    for (void* p : d->allocs) (void)hipFree(p);
    if (d->range_flag_h) (void)hipHostFree(d->range_flag_h);
    if (d->stream) (void)hipStreamDestroy(d->stream);
    delete d;
}

// A device allocation owned by a scope: freed when the scope is left, on every path.
template <class T> struct DevBuf {
    T* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t n) { return hipMalloc((void**)&p, n * sizeof(T)); }
    operator T*() const { return p; }
};

// the decode kernel of the decoder's current settings over n points (device pointers; grad may be null), on the decoder's stream
static void launch_decode(qsp_decoder* d, const float* code, const float* xyz, int64_t n, float* y, float* grad) {
    const int64_t tiles = (n + TILE_P - 1) / TILE_P;
    const int grid = (int)std::min<int64_t>(tiles, 4096);
    launch(decode_form(grad != nullptr, grad ? d->jac_bf3 : d->fwd_bf3, d->P.narrow), grid, d->stream, code, xyz, n, d->Pd, y, grad);
}

// the forward decode of n_vol codes (device, n_vol x CODE_LEN) over the same n points: y (n_vol, n).  Every workgroup gets the
// same number of consecutive (volume, tile) pairs, see k_grid_decode.
static void launch_grid_decode(qsp_decoder* d, const float* codes, const float* xyz, int64_t n, int n_vol, float* y) {
    const int64_t tiles = (n + TILE_P - 1) / TILE_P * n_vol;
    const int chunk = (int)((tiles + 4095) / 4096);
    const int grid = (int)((tiles + chunk - 1) / chunk);
    launch(grid_decode_form(d->fwd_bf3, d->P.narrow), grid, d->stream, codes, xyz, n, n_vol, chunk, d->Pd, y);
}

// the same over a decoder group (callers hold its locks, group_check has passed): volume v with the parameters of member cls[v]
// (device, n_vol class indices in [0, members)).  The first member lends stream and settings, as to every group call.
static void launch_grid_decode_group(qsp_decoder_group* g, const float* codes, const int32_t* cls, const float* xyz, int64_t n, int n_vol,
                                     float* y) {
    const qsp_decoder* d = g->m[0];
    const int64_t tiles = (n + TILE_P - 1) / TILE_P * n_vol;
    const int chunk = (int)((tiles + 4095) / 4096);
    const int grid = (int)((tiles + chunk - 1) / chunk);
    launch(group_grid_decode_form(d->fwd_bf3, d->P.narrow), grid, d->stream, codes, xyz, n, n_vol, chunk, g->Pd, cls, y);
}

static int decode_once(qsp_decoder* d, const float* code, const float* xyz, int64_t n, float* y, float* grad, bool* hit) {
    QSP_HIP(hipSetDevice(d->device));
    DevBuf<float> dc, dx, dy, dg;
    QSP_HIP(dc.alloc(CODE_LEN));
    QSP_HIP(dx.alloc(n * 3));
    QSP_HIP(dy.alloc(n));
    if (grad) QSP_HIP(dg.alloc(n * NIN));
    float code64[CODE_LEN] = {};                       // the caller's code has d->code_len entries
    memcpy(code64, code, sizeof(float) * d->code_len);
    QSP_HIP(hipMemcpyAsync(dc, code64, CODE_LEN * sizeof(float), hipMemcpyHostToDevice, d->stream));
    QSP_HIP(hipMemcpyAsync(dx, xyz, n * 3 * sizeof(float), hipMemcpyHostToDevice, d->stream));
    launch_decode(d, dc, dx, n, dy, dg);
    QSP_HIP(hipGetLastError());
    QSP_HIP(hipMemcpyAsync(y, dy, n * sizeof(float), hipMemcpyDeviceToHost, d->stream));
    std::vector<float> g67;
    if (grad) {
        if (d->code_len == CODE_LEN) {
            QSP_HIP(hipMemcpyAsync(grad, dg, n * NIN * sizeof(float), hipMemcpyDeviceToHost, d->stream));
        } else {
            g67.resize((size_t)n * NIN);
            QSP_HIP(hipMemcpyAsync(g67.data(), dg, n * NIN * sizeof(float), hipMemcpyDeviceToHost, d->stream));
        }
    }
    QSP_HIP(hipStreamSynchronize(d->stream));
    if (range_hit(d)) {
        *hit = true;
        return QSP_OK;
    }
    if (grad && d->code_len != CODE_LEN) {               // [code 64 | xyz] -> [code L | xyz]
        const int L = d->code_len;
        for (int64_t i = 0; i < n; ++i) {
            memcpy(grad + i * (L + 3), g67.data() + i * NIN, sizeof(float) * L);
            memcpy(grad + i * (L + 3) + L, g67.data() + i * NIN + CODE_LEN, sizeof(float) * 3);
        }
    }
    return QSP_OK;
}

static int decode_common(qsp_decoder* d, const float* code, const float* xyz, int64_t n, float* y, float* grad) {
    if (!d || !code || !xyz || n < 0 || !y) return qsp_fail(QSP_ERR_INVALID, "decode: bad argument");
    if (n == 0) return QSP_OK;
    bool hit = false;
    int rc = decode_once(d, code, xyz, n, y, grad, &hit);
    if (rc || !hit) return rc;
    if (!range_should_fall_back(d)) return range_error();
    F32Override f32(d);
    d->n_range_fallbacks++;
    hit = false;
    return decode_once(d, code, xyz, n, y, grad, &hit);
}

extern "C" int qsp_decode_sdf(qsp_decoder* d, const float* code, const float* xyz, int64_t n, float* sdf_out) {
    std::unique_lock<std::recursive_mutex> lk_d;
    if (d) lk_d = std::unique_lock<std::recursive_mutex>(d->mu);
    return decode_common(d, code, xyz, n, sdf_out, nullptr);
}

// The screening tile's values on explicit points (diagnostic: tests and tools/screen_margin.py measure |s1 - s3| with it).
extern "C" int qsp_decode_sdf_screen(qsp_decoder* d, const float* code, const float* xyz, int64_t n, float* s1_out) {
    std::unique_lock<std::recursive_mutex> lk_d;
    if (d) lk_d = std::unique_lock<std::recursive_mutex>(d->mu);
    if (!d || !code || !xyz || n < 0 || !s1_out) return qsp_fail(QSP_ERR_INVALID, "decode_screen: bad argument");
    if (n == 0) return QSP_OK;
    if (!d->fp16_ok) return qsp_fail(QSP_ERR_UNSUPPORTED, "split fp16: a weight of this decoder is outside fp16's range");
    QSP_HIP(hipSetDevice(d->device));
    DevBuf<float> dc, dx, dy;
    QSP_HIP(dc.alloc(CODE_LEN));
    QSP_HIP(dx.alloc(n * 3));
    QSP_HIP(dy.alloc(n));
    float code64[CODE_LEN] = {};
    memcpy(code64, code, sizeof(float) * d->code_len);
    QSP_HIP(hipMemcpyAsync(dc, code64, CODE_LEN * sizeof(float), hipMemcpyHostToDevice, d->stream));
    QSP_HIP(hipMemcpyAsync(dx, xyz, n * 3 * sizeof(float), hipMemcpyHostToDevice, d->stream));
    const int grid = (int)std::min<int64_t>((n + H1_ROWS - 1) / H1_ROWS, 4096);
    launch(decode_screen_form(screen_waves()), grid, d->stream, dc, dx, n, d->Pd, dy);
    QSP_HIP(hipGetLastError());
    QSP_HIP(hipMemcpyAsync(s1_out, dy, n * sizeof(float), hipMemcpyDeviceToHost, d->stream));
    QSP_HIP(hipStreamSynchronize(d->stream));
    return check_range(d);
}

extern "C" int qsp_sdf_value_grad(qsp_decoder* d, const float* code, const float* xyz, int64_t n, float* y, float* grad) {
    std::unique_lock<std::recursive_mutex> lk_d;
    if (d) lk_d = std::unique_lock<std::recursive_mutex>(d->mu);
    if (!grad) return qsp_fail(QSP_ERR_INVALID, "qsp_sdf_value_grad: grad is null");
    return decode_common(d, code, xyz, n, y, grad);
}

// ---------------------------------------------------------------------------------------------------------------
// refinement batch
// ---------------------------------------------------------------------------------------------------------------
struct qsp_refine_batch {
    qsp_decoder* dec = nullptr;     // a group's batch: its first member (stream, options -- the same for every member, group_check)
    qsp_decoder_group* grp = nullptr;   // set: the decoder kernels look up each object's decoder (ObjView::dec) in grp->Pd
    int device = 0;                 // of the decoder, cached: destroy must not touch a decoder that may already be gone
    RefineCfg cfg{};
    int code_len = CODE_LEN;        // dec->code_len, cached like `device`
    int n_iter_cfg = 5;
    int n_obj = 0, n_hyp = 0;
    int max_pts = 0, max_rays = 0;
    // capacities the device buffers were allocated for (qsp_refine_batch_reload refills a batch whose capacities suffice)
    int cap_obj = 0, cap_hyp = 0;
    int64_t cap_pts_total = 0, cap_rays_total = 0;
    int tile_p_created = 64;
    int nw_sdf = 1;
    int64_t rk_stride = 0, ray_stride = 0, act_stride = 0;
    std::vector<ObjView> objs_h;
    std::vector<int32_t> hyp_obj;
    // device
    HypState* st = nullptr;
    ObjView* objs = nullptr;
    float *pts = nullptr, *rays = nullptr, *depth = nullptr;
    int32_t *valid_rk = nullptr, *ray_voff = nullptr, *rend_rk = nullptr;
    float *sdf_valid = nullptr, *rend_deds = nullptr, *rend_res = nullptr, *partials = nullptr;
    float *trH = nullptr, *trb = nullptr, *trdx = nullptr, *trrot = nullptr;
    uint8_t* pt_active = nullptr;   // pose-only mode
    float* res_buf = nullptr;       // pose-only mode: per-point residual of the current iteration
    unsigned long long* counters = nullptr;   // [4] points/tiles processed (fwd+bwd, fwd-only)
    int2 *work_fwd = nullptr, *work_jtj = nullptr;   // work-queue items (k_plan)
    int* qctl = nullptr;            // [4] item counts / next-item counters
    float last_screen_dmax = 0.f;   // the last screened pass: largest |s1 - s3| seen, audited out-of-band samples, how many of them wrong
    int32_t last_audit_wrong = 0;
    int64_t last_audited = 0;
    int32_t* band_idx = nullptr;    // screened forward pass: per hypothesis, indices into its valid-sample list (k_mlp_fwd_h1)
    int32_t* stage_idx = nullptr;   // depth-staged forward: the current stage's samples, as positions in the valid list (k_stage_list)
    uint8_t* ray_open = nullptr;    //   per (hypothesis, ray): no opaque sample in the stages so far
    HypState* st_snap = nullptr;    // the hypotheses as a run found them (restored when the run is repeated on the f32 pipe)
    uint8_t* act_snap = nullptr;    // pose-only mode: pt_active likewise
    float* c0_all = nullptr;        // [n_hyp][2][512] code part of layers 0 and 4 (bias included) per hypothesis (k_c0)
    int n_cu = 256;
    float* rows = nullptr;          // optional tap of the Jacobian rows (qsp_refine_batch_rows)
    int64_t rows_stride = 0;
    // What the host provides per call -- hypothesis states, object table, depth, rays, surface points -- lives in ONE device arena
    // [st | objs | depth | rays | pts] (parts packed to what the fill holds, 256-byte aligned) with a pinned host mirror: fill and
    // set_state write the mirror, the next consumer (run, get, ...) uploads what changed as ONE asynchronous copy on the
    // decoder's stream.  (They were five blocking copies from pageable memory: 0.25 ms of idle GPU in front of every one-object
    // call of 2.7 ms, profiles/r04_call_timeline.txt.)
    char* in_dev = nullptr;
    char* in_host = nullptr;        // pinned
    HypState* out_host = nullptr;   // pinned: the states on their way back (get, trace)
    size_t in_bytes = 0;
    size_t st_bytes = 0;            // this fill's states
    size_t obs_lo = 0, obs_hi = 0;  // the part of the mirror behind the states that waits for its upload
    bool st_dirty = false;
    // profiling
    bool prof = false;
    qsp_refine_profile profile{};
    std::vector<hipEvent_t> ev;
};

static size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// The locks of a call: its decoder's, or every member's of its group in one fixed order (by address), so that a group call
// cannot deadlock against single-decoder calls or other group calls on other threads.
struct CallLock {
    std::vector<std::unique_lock<std::recursive_mutex>> l;
    explicit CallLock(qsp_decoder* d) {
        if (d) l.emplace_back(d->mu);
    }
    explicit CallLock(qsp_decoder_group* g) {
        if (g)
            for (qsp_decoder* d : g->lock_order) l.emplace_back(d->mu);
    }
    explicit CallLock(qsp_refine_batch* b) {
        if (b && b->grp) *this = CallLock(b->grp);
        else if (b && b->dec) l.emplace_back(b->dec->mu);
    }
};

// Checks, at every group call, that the members still agree on everything the group's launches share, and brings the device
// copy of their parameters up to date.  Callers hold the group's locks.
static int group_options(const qsp_decoder_group* g) {
    const qsp_decoder* a = g->m[0];
    for (size_t i = 1; i < g->m.size(); ++i) {
        const qsp_decoder* d = g->m[i];
        const char* what = nullptr;
        if (d->device != a->device) what = "device";
        else if (d->code_len != a->code_len) what = "code_len";
        else if (d->fwd_bf3 != a->fwd_bf3) what = "QSP_DEC_OPT_FORWARD_PRECISION";
        else if (d->jac_bf3 != a->jac_bf3) what = "QSP_DEC_OPT_JACOBIAN_PRECISION";
        else if (d->tile_p != a->tile_p) what = "QSP_DEC_OPT_TILE_POINTS";
        else if (d->P.narrow != a->P.narrow) what = "QSP_DEC_OPT_NARROW_TILE";
        else if (d->screen_margin != a->screen_margin) what = "QSP_DEC_OPT_RENDER_SCREENING";
        else if (d->screen_audit != a->screen_audit) what = "QSP_DEC_OPT_SCREEN_AUDIT";
        else if (d->screen_min_samples != a->screen_min_samples) what = "QSP_DEC_OPT_SCREENING_MIN_SAMPLES";
        else if (d->depth_staging != a->depth_staging) what = "QSP_DEC_OPT_DEPTH_STAGING";
        else if (d->range_fallback != a->range_fallback) what = "QSP_DEC_OPT_RANGE_FALLBACK";
        if (what) {
            const std::string msg = std::string("decoder group: member ") + std::to_string(i) + " differs from member 0 in " + what +
                                    " (the members of a group share it)";
            return qsp_fail(QSP_ERR_UNSUPPORTED, msg.c_str());
        }
    }
    return QSP_OK;
}
static int group_check(qsp_decoder_group* g) {
    const int rc = group_options(g);
    if (rc) return rc;
    bool stale = g->Ph.size() != g->m.size();
    g->Ph.resize(g->m.size());
    for (size_t i = 0; i < g->m.size(); ++i)
        if (memcmp(&g->Ph[i], &g->m[i]->P, sizeof(MlpParams)) != 0) {
            memcpy(&g->Ph[i], &g->m[i]->P, sizeof(MlpParams));
            stale = true;
        }
    if (stale) {
        QSP_HIP(hipSetDevice(g->device));
        QSP_HIP(hipStreamSynchronize(g->m[0]->stream));
        QSP_HIP(hipMemcpy(g->Pd, g->Ph.data(), sizeof(MlpParams) * g->m.size(), hipMemcpyHostToDevice));
    }
    return QSP_OK;
}

// a group call's class index per object: [0, n) of the group
static int group_classes(const qsp_decoder_group* g, int32_t n_obj, const int32_t* cls) {
    if (!cls) return qsp_fail(QSP_ERR_INVALID, "decoder group: class index array is null");
    for (int o = 0; o < n_obj; ++o)
        if (cls[o] < 0 || cls[o] >= (int32_t)g->m.size())
            return qsp_fail(QSP_ERR_INVALID, "decoder group: class index out of range [0, number of members)");
    return QSP_OK;
}

// uploads what fill / set_state left in the mirror (one copy; nothing when nothing changed)
static int batch_upload(qsp_refine_batch* b) {
    size_t lo = 0, hi = 0;
    if (b->st_dirty && b->obs_hi > b->obs_lo) lo = 0, hi = b->obs_hi;
    else if (b->st_dirty) lo = 0, hi = b->st_bytes;
    else if (b->obs_hi > b->obs_lo) lo = b->obs_lo, hi = b->obs_hi;
    b->st_dirty = false;
    b->obs_lo = b->obs_hi = 0;
    if (hi > lo) QSP_HIP(hipMemcpyAsync(b->in_dev + lo, b->in_host + lo, hi - lo, hipMemcpyHostToDevice, b->dec->stream));
    return QSP_OK;
}

static void batch_free(qsp_refine_batch* b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->in_host) (void)hipHostFree(b->in_host);
    if (b->out_host) (void)hipHostFree(b->out_host);
    void* ptrs[] = {b->in_dev, b->valid_rk, b->ray_voff, b->rend_rk, b->sdf_valid,
                    b->rend_deds, b->rend_res, b->partials, b->trH, b->trb, b->trdx, b->trrot, b->pt_active, b->res_buf, b->rows, b->counters,
                    b->work_fwd, b->work_jtj, b->c0_all, b->band_idx, b->stage_idx, b->ray_open, b->st_snap, b->act_snap};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    for (hipEvent_t e : b->ev) (void)hipEventDestroy(e);
    delete b;
    (void)hipGetLastError();   // errors are ignored here; do not leave one behind for the next call's launch check
}

// Capacities of a batch: what its device buffers are allocated for.  A batch created for given inputs has exactly their extents;
// the resident batch of qsp_reconstruct_objects (the decoder's arena) is created with head-room and refilled by batch_fill.
struct BatchCaps {
    int obj = 0, hyp = 0, max_pts = 0, max_rays = 0;
    int64_t pts_total = 0, rays_total = 0;
};

static int batch_validate(const RefineCfg& cfg, int32_t n_obj, const int32_t* n_pts, const int32_t* n_rays, const int32_t* n_fg,
                          int32_t n_hyp, const int32_t* hyp_obj, BatchCaps* need) {
    BatchCaps c;
    c.obj = n_obj;
    c.hyp = n_hyp;
    for (int o = 0; o < n_obj; ++o) {
        const int nr = cfg.pose_only ? 0 : n_rays[o];
        const int nf = cfg.pose_only ? 0 : n_fg[o];
        if (n_pts[o] < 0 || nr < 0 || nf < 0 || nf > nr || nr >= (1 << 25)) return qsp_fail(QSP_ERR_INVALID, "refine batch: bad per-object counts");
        c.pts_total += n_pts[o];
        c.rays_total += nr;
        c.max_pts = std::max(c.max_pts, (int)n_pts[o]);
        c.max_rays = std::max(c.max_rays, nr);
    }
    for (int h = 0; h < n_hyp; ++h)
        if (hyp_obj[h] < 0 || hyp_obj[h] >= n_obj) return qsp_fail(QSP_ERR_INVALID, "refine batch: hyp_obj out of range");
    *need = c;
    return QSP_OK;
}

// (re)fills a batch whose capacities suffice: object extents, observations, hypothesis -> object map.  Strides, slot counts
// and buffer sizes stay those of the capacities; every per-object quantity the kernels use comes from the ObjView table.
static int batch_fill(qsp_refine_batch* b, int32_t n_obj, const float* const* pts, const int32_t* n_pts, const float* const* rays,
                      const int32_t* n_rays, const float* const* depth, const int32_t* n_fg, int32_t n_hyp, const int32_t* hyp_obj,
                      bool device_fill, const int32_t* obj_class = nullptr) {
    const RefineCfg& cfg = b->cfg;
    b->n_obj = n_obj;
    b->n_hyp = n_hyp;
    b->objs_h.resize(n_obj);
    int64_t po = 0, ro = 0;
    for (int o = 0; o < n_obj; ++o) {
        const int nr = cfg.pose_only ? 0 : n_rays[o];
        const int nf = cfg.pose_only ? 0 : n_fg[o];
        b->objs_h[o] = ObjView{po, ro, n_pts[o], nr, nf, obj_class ? obj_class[o] : 0};
        po += n_pts[o];
        ro += nr;
    }
    b->hyp_obj.assign(hyp_obj, hyp_obj + n_hyp);
    // this fill's layout of the input arena (sizes <= the capacities it was allocated for, part by part)
    const size_t n_ray_f = (size_t)std::max<int64_t>(ro, 1), n_pt_f = (size_t)std::max<int64_t>(po, 1);
    b->st_bytes = sizeof(HypState) * (size_t)n_hyp;
    const size_t o_objs = align256(b->st_bytes), o_depth = o_objs + align256(sizeof(ObjView) * (size_t)n_obj);
    const size_t o_rays = o_depth + align256(sizeof(float) * n_ray_f), o_pts = o_rays + align256(sizeof(float) * 3 * n_ray_f);
    const size_t o_end = o_pts + sizeof(float) * 3 * n_pt_f;
    if (o_end > b->in_bytes) return qsp_fail(QSP_ERR_INVALID, "refine batch: inputs exceed the batch's capacities");
    b->objs = (ObjView*)(b->in_dev + o_objs);
    b->depth = (float*)(b->in_dev + o_depth);
    b->rays = (float*)(b->in_dev + o_rays);
    b->pts = (float*)(b->in_dev + o_pts);
    memcpy(b->in_host + o_objs, b->objs_h.data(), sizeof(ObjView) * (size_t)n_obj);
    b->obs_lo = o_objs;
    b->obs_hi = o_depth;
    if (device_fill) {        // (the observation arrays are written by a kernel; depth entries beyond a ray's foreground stay 0)
        QSP_HIP(hipMemsetAsync(b->depth, 0, sizeof(float) * n_ray_f, b->dec->stream));
        return QSP_OK;
    }
    float* hp = (float*)(b->in_host + o_pts);
    float* hr = (float*)(b->in_host + o_rays);
    float* hd = (float*)(b->in_host + o_depth);
    memset(hd, 0, sizeof(float) * n_ray_f);
    for (int o = 0; o < n_obj; ++o) {
        const ObjView& v = b->objs_h[o];
        if (v.n_pts) memcpy(hp + 3 * v.pts_off, pts[o], sizeof(float) * 3 * v.n_pts);
        if (v.n_rays) memcpy(hr + 3 * v.ray_off, rays[o], sizeof(float) * 3 * v.n_rays);
        if (v.n_fg) memcpy(hd + v.ray_off, depth[o], sizeof(float) * v.n_fg);
    }
    b->obs_hi = o_end;
    return QSP_OK;
}

static bool batch_fits(const qsp_refine_batch* b, const BatchCaps& need) {
    return need.obj <= b->cap_obj && need.hyp <= b->cap_hyp && need.max_pts <= b->max_pts && need.max_rays <= b->max_rays &&
           need.pts_total <= b->cap_pts_total && need.rays_total <= b->cap_rays_total;
}

static int batch_create(qsp_decoder* dec, const RefineCfg& cfg, int n_iter, int32_t n_obj, const float* const* pts,
                        const int32_t* n_pts, const float* const* rays, const int32_t* n_rays,
                        const float* const* depth, const int32_t* n_fg, int32_t n_hyp, const int32_t* hyp_obj,
                        qsp_refine_batch** out, bool device_fill = false, const BatchCaps* caps_in = nullptr,
                        qsp_decoder_group* grp = nullptr, const int32_t* obj_class = nullptr) {
    // device_fill: only the extents are given, the observation arrays are written by a kernel (detections.hpp)
    if (!dec || !out || n_obj <= 0 || n_hyp <= 0 || (!pts && !device_fill) || !n_pts || !hyp_obj)
        return qsp_fail(QSP_ERR_INVALID, "refine batch: bad argument");
    if (!cfg.pose_only && ((!device_fill && (!rays || !depth)) || !n_rays || !n_fg))
        return qsp_fail(QSP_ERR_INVALID, "refine batch: rays missing");
    if (cfg.n_depth < 2 || cfg.n_depth > MAX_DEPTH) return qsp_fail(QSP_ERR_INVALID, "n_depth must be in [2, 64]");
    if (dec->tile_p == 32 && (dec->fwd_bf3 != 2 || dec->jac_bf3 != 2))
        return qsp_fail(QSP_ERR_UNSUPPORTED, "32-point tiles (QSP_DEC_OPT_TILE_POINTS) exist on the split-fp16 pipe only: set both "
                                             "precisions to 2 first");
    BatchCaps need;
    {
        const int rc = batch_validate(cfg, n_obj, n_pts, n_rays, n_fg, n_hyp, hyp_obj, &need);
        if (rc) return rc;
    }
    BatchCaps caps = caps_in ? *caps_in : need;      // (caps_in >= need, the caller's business)
    const int tile_p = dec->tile_p;
    QSP_HIP(hipSetDevice(dec->device));
    qsp_refine_batch* b = new qsp_refine_batch();
    b->dec = dec;
    b->grp = grp;
    b->device = dec->device;
    b->code_len = dec->code_len;
    b->cfg = cfg;
    b->cfg.code_len = dec->code_len;
    b->cfg.tile_p = dec->tile_p;
    b->tile_p_created = dec->tile_p;
    b->n_iter_cfg = n_iter;
    b->cap_obj = caps.obj;
    b->cap_hyp = caps.hyp;
    b->cap_pts_total = caps.pts_total;
    b->cap_rays_total = caps.rays_total;
    b->max_pts = caps.max_pts;
    b->max_rays = caps.max_rays;
    const int64_t cp = std::max<int64_t>(caps.pts_total, 1), cr = std::max<int64_t>(caps.rays_total, 1);
    const int cap_hyp = caps.hyp;
    b->nw_sdf = std::max(1, std::min(NW_SDF_MAX, (b->max_pts + tile_p - 1) / tile_p));
    b->rk_stride = (int64_t)std::max(1, b->max_rays) * cfg.n_depth;
    b->ray_stride = b->max_rays + 1;
    b->act_stride = std::max(1, b->max_pts);
    const int nw_total = b->nw_sdf + (cfg.pose_only ? 0 : NW_REND);
    int rc = QSP_OK;
#define QSP_ALLOC(ptr, bytes)                                                                 \
    if (!rc) {                                                                                \
        hipError_t e_ = hipMalloc((void**)&(ptr), (size_t)(bytes));                           \
        if (e_ != hipSuccess) rc = qsp_fail(QSP_ERR_DEVICE, hipGetErrorString(e_));           \
    }
    b->in_bytes = align256(sizeof(HypState) * (size_t)cap_hyp) + align256(sizeof(ObjView) * (size_t)caps.obj) +
                  align256(sizeof(float) * (size_t)cr) + align256(sizeof(float) * 3 * (size_t)cr) + align256(sizeof(float) * 3 * (size_t)cp);
    QSP_ALLOC(b->in_dev, b->in_bytes);
    b->st = (HypState*)b->in_dev;
    if (!rc) {
        hipError_t e_ = hipHostMalloc((void**)&b->in_host, b->in_bytes, hipHostMallocDefault);
        if (e_ == hipSuccess) e_ = hipHostMalloc((void**)&b->out_host, sizeof(HypState) * (size_t)cap_hyp, hipHostMallocDefault);
        if (e_ != hipSuccess) rc = qsp_fail(QSP_ERR_DEVICE, hipGetErrorString(e_));
    }
    QSP_ALLOC(b->partials, sizeof(float) * (size_t)cap_hyp * nw_total * PART_FLOATS);
    QSP_ALLOC(b->trH, sizeof(float) * (size_t)cap_hyp * NH * NH);
    QSP_ALLOC(b->trb, sizeof(float) * (size_t)cap_hyp * NH);
    QSP_ALLOC(b->trdx, sizeof(float) * (size_t)cap_hyp * NH);
    QSP_ALLOC(b->trrot, sizeof(float) * (size_t)cap_hyp * 4);
    QSP_ALLOC(b->counters, sizeof(unsigned long long) * 8 + sizeof(int) * 8);      // [counters | qctl]: one fill clears both
    if (!rc) b->qctl = (int*)(b->counters + 8);
    QSP_ALLOC(b->st_snap, sizeof(HypState) * cap_hyp);
    // qctl: [0..3] the two queues, [4], [5] the done counters of the plans in k_sample's / k_scan's tail
    QSP_ALLOC(b->c0_all, sizeof(float) * (size_t)cap_hyp * 2 * HID);
    QSP_ALLOC(b->work_jtj, sizeof(int2) * (size_t)cap_hyp * nw_total);
    if (!cfg.pose_only) QSP_ALLOC(b->work_fwd, sizeof(int2) * (size_t)cap_hyp * ((b->rk_stride + TILE_P - 1) / TILE_P));
    {
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dec->device) == hipSuccess && ncu > 0) b->n_cu = ncu;
    }
    if (!cfg.pose_only) {
        QSP_ALLOC(b->valid_rk, sizeof(int32_t) * (size_t)cap_hyp * b->rk_stride);
        QSP_ALLOC(b->ray_voff, sizeof(int32_t) * (size_t)cap_hyp * b->ray_stride);
        QSP_ALLOC(b->rend_rk, sizeof(int32_t) * (size_t)cap_hyp * b->rk_stride);
        QSP_ALLOC(b->sdf_valid, sizeof(float) * (size_t)cap_hyp * b->rk_stride);
        QSP_ALLOC(b->rend_deds, sizeof(float) * (size_t)cap_hyp * b->rk_stride);
        QSP_ALLOC(b->rend_res, sizeof(float) * (size_t)cap_hyp * b->rk_stride);
        QSP_ALLOC(b->band_idx, sizeof(int32_t) * (size_t)cap_hyp * b->rk_stride);
        QSP_ALLOC(b->stage_idx, sizeof(int32_t) * (size_t)cap_hyp * b->rk_stride);
        QSP_ALLOC(b->ray_open, (size_t)cap_hyp * b->ray_stride);
    } else {
        QSP_ALLOC(b->pt_active, (size_t)cap_hyp * b->act_stride);
        QSP_ALLOC(b->act_snap, (size_t)cap_hyp * b->act_stride);
        QSP_ALLOC(b->res_buf, sizeof(float) * (size_t)cap_hyp * b->act_stride);
    }
#undef QSP_ALLOC
    if (!rc) {
        hipError_t e = hipMemset(b->trH, 0, sizeof(float) * (size_t)cap_hyp * NH * NH);
        if (e == hipSuccess) e = hipMemset(b->trb, 0, sizeof(float) * (size_t)cap_hyp * NH);
        if (e == hipSuccess) e = hipMemset(b->trdx, 0, sizeof(float) * (size_t)cap_hyp * NH);
        if (e == hipSuccess) e = hipMemset(b->trrot, 0, sizeof(float) * (size_t)cap_hyp * 4);
        if (e != hipSuccess) rc = qsp_fail(QSP_ERR_DEVICE, hipGetErrorString(e));
    }
    if (!rc) rc = batch_fill(b, n_obj, pts, n_pts, rays, n_rays, depth, n_fg, n_hyp, hyp_obj, device_fill, obj_class);
    if (rc) {
        batch_free(b);
        return rc;
    }
    *out = b;
    return QSP_OK;
}

extern "C" int qsp_refine_batch_create(qsp_decoder* dec, const qsp_joint_cfg* cfg, int32_t n_obj, const float* const* pts,
                                       const int32_t* n_pts, const float* const* rays, const int32_t* n_rays,
                                       const float* const* depth, const int32_t* n_fg, int32_t n_hyp,
                                       const int32_t* hyp_obj, qsp_refine_batch** out) {
    if (!cfg) return qsp_fail(QSP_ERR_INVALID, "cfg is null");
    if (cfg->code_len != dec->code_len) return qsp_fail(QSP_ERR_INVALID, "code_len of the optimizer config differs from the decoder's");
    RefineCfg c{cfg->k1, cfg->k2, cfg->k3, cfg->k4, cfg->b1, cfg->b2, cfg->lr, cfg->s_damp, cfg->cut_off, cfg->n_depth, 0, 0,
                dec->code_len};
    return batch_create(dec, c, cfg->n_iter, n_obj, pts, n_pts, rays, n_rays, depth, n_fg, n_hyp, hyp_obj, out);
}

extern "C" void qsp_refine_batch_destroy(qsp_refine_batch* b) { batch_free(b); }

extern "C" int qsp_refine_batch_set_state(qsp_refine_batch* b, const float* t_cam_obj, const float* code) {
    const CallLock lk(b);
    if (!b || !t_cam_obj) return qsp_fail(QSP_ERR_INVALID, "set_state: bad argument");
    QSP_HIP(hipSetDevice(b->dec->device));
    HypState* hs = (HypState*)b->in_host;      // (the mirror; uploaded by the next run / get)
    for (int h = 0; h < b->n_hyp; ++h) {
        HypState& S = hs[h];
        memset(&S, 0, sizeof(S));
        inv4_gj(t_cam_obj + 16 * h, S.T_oc);   // t_obj_cam = inverse(t_cam_obj)  (optimizer.py:123)
        if (code) memcpy(S.code, code + (size_t)h * b->code_len, sizeof(float) * b->code_len);   // rest stays 0
        S.alive = 1;
        S.obj = b->hyp_obj[h];
    }
    b->st_dirty = true;
    if (b->pt_active) QSP_HIP(hipMemsetAsync(b->pt_active, 1, (size_t)b->n_hyp * b->act_stride, b->dec->stream));
    return QSP_OK;
}

static hipEvent_t next_event(qsp_refine_batch* b, size_t& cursor) {
    if (cursor >= b->ev.size()) {
        hipEvent_t e;
        (void)hipEventCreate(&e);
        b->ev.push_back(e);
    }
    hipEvent_t e = b->ev[cursor++];
    (void)hipEventRecord(e, b->dec->stream);
    return e;
}

// the screened forward is trusted while the largest |s1 - s3| it sees on a band sample stays below this share of the margin
constexpr float SCREEN_TRUST = 0.5f;

// The profiling marks of run_once(): every pass of an iteration sits between one begin() and one end(kind), which record events
// on the decoder's stream while profiling is on and do nothing otherwise.  kind: 0 = Jacobian pass, 1 = forward pass, 2 = other.
struct PassMarks {
    struct Span { hipEvent_t a, b; int kind; };
    qsp_refine_batch* b;
    size_t cur = 0;
    hipEvent_t a = nullptr;
    std::vector<Span> spans;
    hipEvent_t mark() { return b->prof ? next_event(b, cur) : nullptr; }
    void begin() { a = mark(); }
    void end(int kind) {
        if (b->prof) spans.push_back({a, next_event(b, cur), kind});
    }
};

// one pass over n_iter Gauss-Newton iterations on the decoder's current pipes; *hit = a split-fp16 kernel left fp16's range,
// *screen_hit = the screened forward saw |s1 - s3| above half its margin on a band sample (the margin's premise is in doubt)
static int run_once(qsp_refine_batch* b, int32_t n_iter, bool* hit, bool* screen_hit) {
    bool screened_any = false;
    const qsp_decoder* d = b->dec;
    hipStream_t s = d->stream;
    const bool grp = b->grp != nullptr;      // a decoder group's batch: the GRP forms of the decoder kernels
    const MlpParams* Pm = grp ? b->grp->Pd : d->Pd;      // (a group's: one entry per member)
    const int nH = b->n_hyp;
    const int nw_total = b->nw_sdf + (b->cfg.pose_only ? 0 : NW_REND);
    PassMarks pm{b};
    // (the work counters, and with them the queue words: the done counters of the plan tails may be left over from a run cut short)
    QSP_HIP(hipMemsetAsync(b->counters, 0, sizeof(unsigned long long) * 8 + sizeof(int) * 8, s));
    const hipEvent_t e_begin = pm.mark();
    for (int it = 0; it < n_iter; ++it) {
        RefineCfg cfg = b->cfg;
        cfg.iter = it;
        if (d->jac_bf3 != 2) cfg.tile_p = TILE_P;      // (32-point tiles exist on the split-fp16 pipe only: the f32 repeat of a
                                                       //  batch created for them runs 64-point tiles over the same slots)
        if (cfg.pose_only)
            hipLaunchKernelGGL(grp ? k_c0<true> : k_c0<false>, dim3(nH), dim3(MLP_THREADS), 0, s, b->st, b->objs, Pm, b->c0_all);
        if (!cfg.pose_only) {      // (k_sample also forms the bias vectors k_c0 forms in pose-only mode)
            pm.begin();
            // Two passes pay when the one-pass kernel would need more than one round of 64-point tiles over the chip; a batch that
            // fits one round (a single object per call) is faster in one pass: one tile deep either way, without the second
            // launch.  Both give the same bits, so the choice is free.  (~half of the ray samples are inside the unit ball.)
            int64_t ub_samples = 0;
            for (int h = 0; h < nH; ++h) ub_samples += (int64_t)b->objs_h[b->hyp_obj[h]].n_rays * cfg.n_depth;
            const int64_t min_samples = d->screen_min_samples >= 0 ? d->screen_min_samples : 2 * (int64_t)b->n_cu * TILE_P;
            // (a narrow decoder's one-pass forward on the NARROW tile is cheaper than the full-width screening pass: not screened)
            const bool screen = d->fwd_bf3 == 2 && d->screen_margin > 0.f && ub_samples > min_samples && !d->P.narrow;
            // the forward kernel's item list is built in k_sample's tail (plan_tail; the forward pass keeps 64-point tiles: tens of
            // thousands of ray samples fill the chip either way) -- or, when the screened pass runs in depth stages, in the tail of
            // each stage's k_stage_list
            // (a stage costs a list kernel, a plan and a band pass that is one tile deep whatever its size: it pays once the screening
            //  pass is tens of tile rounds over the chip -- C4 and C5; measured break-even around C2, 0.7 M samples: 18.1 against
            //  19.1 ms per step; four yaw flips of one object: 3.8 against 4.8 ms per call)
            const bool staged = screen && cfg.n_depth >= 4 &&
                                (d->depth_staging == 2 || (d->depth_staging == 1 && ub_samples > 64 * (int64_t)b->n_cu * H1_ROWS));
            const PlanTail pt_fwd{staged ? nullptr : b->work_fwd, b->qctl, b->qctl + 4, nH, b->nw_sdf, nw_total - b->nw_sdf,
                                  screen ? H1_ROWS : TILE_P, 0};
            hipLaunchKernelGGL(grp ? k_sample<true> : k_sample<false>, dim3(nH), dim3(SAMPLE_THREADS), 0, s, b->st, b->objs, b->rays, cfg,
                               b->valid_rk, b->rk_stride, b->ray_voff, b->ray_stride, Pm, b->c0_all, pt_fwd);
            pm.end(2);
            pm.begin();
            // every forward kernel takes this argument list; `more` = what its family takes behind it
            const auto forward = [&](const auto& f, const auto&... more) {
                launch(f, b->n_cu, s, b->st, b->objs, b->rays, cfg, Pm, b->valid_rk, b->rk_stride, b->sdf_valid, b->work_fwd, b->qctl,
                       b->c0_all, more...);
            };
            if (screen) {
                // two passes (QSP_DEC_OPT_RENDER_SCREENING): every sample on the one-product tile, then the band around the
                // surface on the split-fp16 tile; the queue's control words and item list are reused behind the first pass.
                // Depth-staged (QSP_DEC_OPT_DEPTH_STAGING): that pair once for the depth indices [0, D/2) of every ray and once
                // for [D/2, D) of the rays that have no opaque sample yet (k_stage_list).
                const int n_stage = staged ? 2 : 1, k_mid = cfg.n_depth / 2;
                for (int sg = 0; sg < n_stage; ++sg) {
                    const int32_t* stage_list = nullptr;
                    if (staged) {
                        const PlanTail pt_st{b->work_fwd, b->qctl, b->qctl + 4, nH, b->nw_sdf, nw_total - b->nw_sdf, H1_ROWS, 3};
                        hipLaunchKernelGGL(k_stage_list, dim3(nH), dim3(256), 0, s, b->st, b->objs, cfg, b->valid_rk, b->rk_stride, b->ray_voff,
                                           b->ray_stride, b->sdf_valid, b->ray_open, b->stage_idx, 0, sg == 0 ? 0 : k_mid,
                                           sg == 0 ? k_mid : cfg.n_depth, pt_st);
                        stage_list = b->stage_idx;
                    }
                    forward(screen_form(screen_waves(), grp), b->band_idx, cfg.cut_off + d->screen_margin, d->screen_audit, stage_list);
                    hipLaunchKernelGGL(k_plan, dim3(1), dim3(1024), 0, s, 2, b->st, b->objs, nH, b->nw_sdf, nw_total - b->nw_sdf,
                                       b->work_fwd, b->qctl, TILE_P);
                    forward(fwd_h2_form(false, grp), b->band_idx, (unsigned int*)(b->counters + 5));
                }
                screened_any = true;
            } else if (d->fwd_bf3 == 2)
                forward(fwd_h2_form(d->P.narrow, grp), nullptr, nullptr);      // (no band list, no screening statistics)
            else
                forward(fwd_form(d->fwd_bf3, grp));
            pm.end(1);
            pm.begin();
            // (the Jacobian kernel's item list is built in k_scan's tail)
            const PlanTail pt_jtj{b->work_jtj, b->qctl, b->qctl + 5, nH, b->nw_sdf, nw_total - b->nw_sdf, cfg.tile_p, 1};
            launch(scan_kernel(), nH, s, b->st, b->objs, b->depth, cfg, b->valid_rk, b->rk_stride, b->ray_voff, b->ray_stride, b->sdf_valid,
                   b->rend_rk, b->rend_deds, b->rend_res, pt_jtj);
            pm.end(2);
        }
        pm.begin();
        if (cfg.pose_only)      // (no render pass in front of it: the plan is a launch of its own)
            hipLaunchKernelGGL(k_plan, dim3(1), dim3(1024), 0, s, 1, b->st, b->objs, nH, b->nw_sdf, nw_total - b->nw_sdf,
                               b->work_jtj, b->qctl, cfg.tile_p);
        if (d->jac_bf3 == 2)
            launch(jtj_h2_form(d->P.narrow, cfg.tile_p, jtj_waves(), jtj_waves_t32(), grp), b->n_cu, s,
                   JtjArgs{b->st, b->objs, b->pts, b->rays, cfg, Pm, b->nw_sdf, nw_total, b->rend_rk, b->rend_deds, b->rend_res,
                           b->rk_stride, b->pt_active, b->act_stride, b->res_buf, b->rows, b->rows_stride, b->partials, b->work_jtj,
                           b->qctl, b->c0_all});
        else
            launch(jtj_form(d->jac_bf3, grp), b->n_cu, s, b->st, b->objs, b->pts, b->rays, cfg, Pm, b->nw_sdf, b->rend_rk, b->rend_deds,
                   b->rend_res, b->rk_stride, b->pt_active, b->act_stride, b->res_buf, b->rows, b->rows_stride, b->partials, nw_total,
                   b->work_jtj, b->qctl, b->c0_all);
        pm.end(0);
        pm.begin();
        hipLaunchKernelGGL(k_solve, dim3(nH), dim3(SOLVE_THREADS), 0, s, b->st, b->objs, cfg, b->partials, b->nw_sdf, nw_total,
                           b->pt_active, b->act_stride, b->trH, b->trb, b->trdx, b->counters, b->trrot);
        pm.end(2);
        if (cfg.pose_only && it == 4 && b->max_pts > 0)   // optimizer.py:80-82
            hipLaunchKernelGGL(k_inlier_filter, dim3((b->max_pts + 255) / 256, nH), dim3(256), 0, s, b->st, b->objs,
                               b->res_buf, b->act_stride, b->pt_active);
    }
    const hipEvent_t e_end = pm.mark();
    QSP_HIP(hipGetLastError());
    QSP_HIP(hipStreamSynchronize(s));
    if (range_hit(b->dec)) {
        *hit = true;
        return QSP_OK;
    }
    float dmax = 0.f;
    if (screened_any) {      // (16 bytes, behind the synchronisation above; a one-object call is never screened and skips it)
        unsigned long long w[2] = {0, 0};
        QSP_HIP(hipMemcpy(w, b->counters + 5, sizeof(w), hipMemcpyDeviceToHost));
        const unsigned int bits = (unsigned int)w[0];
        memcpy(&dmax, &bits, sizeof(dmax));
        b->last_screen_dmax = dmax;
        b->last_audit_wrong = (int32_t)(w[0] >> 32);      // audited out-of-band samples the screening pass clamped wrongly
        b->last_audited = (int64_t)w[1];
        if (!(dmax <= SCREEN_TRUST * b->dec->screen_margin) || b->last_audit_wrong > 0) {
            *screen_hit = true;
            return QSP_OK;
        }
    }
    if (b->prof) {
        qsp_refine_profile& p = b->profile;
        memset(&p, 0, sizeof(p));
        p.screen_max_diff = dmax;
        p.pts_audit = screened_any ? b->last_audited : 0;
        (void)hipEventElapsedTime(&p.ms_total, e_begin, e_end);
        for (const PassMarks::Span& sp : pm.spans) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, sp.a, sp.b);
            if (sp.kind == 0) { p.ms_mlp_jtj += ms; p.n_launch_jtj++; }
            else if (sp.kind == 1) { p.ms_mlp_fwd += ms; p.n_launch_fwd++; }
            else p.ms_other += ms;
        }
        unsigned long long c[8];
        QSP_HIP(hipMemcpy(c, b->counters, sizeof(c), hipMemcpyDeviceToHost));
        p.pts_jtj = (int64_t)c[0];
        p.pts_fwd = (int64_t)c[1];
        p.tiles_jtj = (int64_t)c[2];
        p.tiles_fwd = (int64_t)c[3];
        p.pts_band = (int64_t)c[4];
    }
    return QSP_OK;
}

extern "C" int qsp_refine_batch_run(qsp_refine_batch* b, int32_t n_iter) {
    const CallLock lk(b);
    if (!b) return qsp_fail(QSP_ERR_INVALID, "run: null batch");
    if (b->grp) {      // (a member's options may have changed since the batch was created)
        const int rc_g = group_check(b->grp);
        if (rc_g) return rc_g;
    }
    QSP_HIP(hipSetDevice(b->dec->device));
    if (n_iter <= 0) n_iter = b->n_iter_cfg;
    qsp_decoder* d = b->dec;
    {
        const int rc_up = batch_upload(b);
        if (rc_up) return rc_up;
    }
    // The state this run starts from (n_hyp x 432 bytes), in case it has to be repeated: on the f32 pipe after a value left fp16's
    // range, or in one pass after the self-check of the screened forward (a split-fp16 feature) failed.
    const bool may_fall_back = range_should_fall_back(d);
    const bool may_screen = d->fwd_bf3 == 2 && d->screen_margin > 0.f;
    if (may_fall_back || may_screen) {
        QSP_HIP(hipMemcpyAsync(b->st_snap, b->st, sizeof(HypState) * b->n_hyp, hipMemcpyDeviceToDevice, d->stream));
        if (b->pt_active) QSP_HIP(hipMemcpyAsync(b->act_snap, b->pt_active, (size_t)b->n_hyp * b->act_stride, hipMemcpyDeviceToDevice, d->stream));
    }
    auto restore = [&]() -> int {
        QSP_HIP(hipMemcpyAsync(b->st, b->st_snap, sizeof(HypState) * b->n_hyp, hipMemcpyDeviceToDevice, d->stream));
        if (b->pt_active) QSP_HIP(hipMemcpyAsync(b->pt_active, b->act_snap, (size_t)b->n_hyp * b->act_stride, hipMemcpyDeviceToDevice, d->stream));
        return QSP_OK;
    };
    // (what the last run reported must not outlive it -- with profiling off nothing else resets these)
    b->profile.range_fallbacks = b->profile.screen_fallbacks = b->profile.screen_audit_failures = 0;
    b->profile.screen_max_diff = 0.f;
    b->profile.pts_audit = 0;
    b->last_screen_dmax = 0.f;
    b->last_audit_wrong = 0;
    b->last_audited = 0;
    bool hit = false, screen_hit = false;
    int rc = run_once(b, n_iter, &hit, &screen_hit);
    if (rc || (!hit && !screen_hit)) return rc;
    int screen_fallbacks = 0, audit_failures = 0;
    float failed_dmax = 0.f;
    int64_t failed_audited = 0;
    if (screen_hit) {
        audit_failures = b->last_audit_wrong;
        failed_dmax = b->last_screen_dmax;
        failed_audited = b->last_audited;
        // The band samples' two values differ by more than half the margin: the premise "no sample outside the band could have
        // crossed the cut-off" no longer has its safety factor.  Repeat from the starting state in one pass (the path the
        // screened one is bit-identical to when the premise holds).
        if ((rc = restore())) return rc;
        const float margin = d->screen_margin;
        d->screen_margin = 0.f;
        d->n_screen_fallbacks++;
        screen_fallbacks = 1;
        hit = screen_hit = false;
        rc = run_once(b, n_iter, &hit, &screen_hit);
        d->screen_margin = margin;
        b->profile.screen_fallbacks = 1;
        b->profile.screen_audit_failures = audit_failures;      // what the screened attempt saw (the repeat is one-pass: it sees nothing)
        b->profile.screen_max_diff = failed_dmax;
        b->profile.pts_audit = failed_audited;
        if (rc || !hit) return rc;
    }
    if (!may_fall_back) return range_error();
    // A value left fp16's range.  The reference accepts such a decoder (it computes in float32) and never raises for a numeric
    // condition (reconstruct/optimizer.py:161-194), so the run is repeated from its starting state on the exact-f32 pipe.
    if ((rc = restore())) return rc;
    F32Override f32(d);
    d->n_range_fallbacks++;
    hit = screen_hit = false;
    rc = run_once(b, n_iter, &hit, &screen_hit);
    b->profile.range_fallbacks = 1;
    b->profile.screen_fallbacks = screen_fallbacks;
    b->profile.screen_audit_failures = audit_failures;
    return rc;
}


extern "C" int qsp_refine_batch_profile(qsp_refine_batch* b, int enable, qsp_refine_profile* out) {
    if (!b) return qsp_fail(QSP_ERR_INVALID, "profile: null batch");
    b->prof = enable != 0;
    if (out) *out = b->profile;
    return QSP_OK;
}

// the hypothesis states as the device holds them (pending uploads first), through the pinned buffer; valid until the next call
static int batch_states(qsp_refine_batch* b, const HypState** out) {
    const int rc = batch_upload(b);
    if (rc) return rc;
    QSP_HIP(hipMemcpyAsync(b->out_host, b->st, sizeof(HypState) * b->n_hyp, hipMemcpyDeviceToHost, b->dec->stream));
    QSP_HIP(hipStreamSynchronize(b->dec->stream));
    *out = b->out_host;
    return QSP_OK;
}

extern "C" int qsp_refine_batch_get(qsp_refine_batch* b, float* t_cam_obj_out, float* code_out, float* loss_out,
                                    uint8_t* is_good_out) {
    const CallLock lk(b);
    if (!b) return qsp_fail(QSP_ERR_INVALID, "get: null batch");
    QSP_HIP(hipSetDevice(b->dec->device));
    const HypState* hs = nullptr;
    {
        const int rc = batch_states(b, &hs);
        if (rc) return rc;
    }
    for (int h = 0; h < b->n_hyp; ++h) {
        const HypState& S = hs[h];
        if (t_cam_obj_out) {
            inv4_gj(S.T_oc, t_cam_obj_out + 16 * h);   // t_cam_obj = inverse(t_obj_cam)  (optimizer.py:273)
        }
        if (code_out) memcpy(code_out + (size_t)h * b->code_len, S.code, sizeof(float) * b->code_len);
        if (loss_out) loss_out[h] = S.loss;
        if (is_good_out) is_good_out[h] = S.alive ? 1 : 0;
    }
    return QSP_OK;
}

extern "C" int qsp_refine_batch_trace(qsp_refine_batch* b, float* H, float* rhs, float* dx, int32_t* n_valid,
                                      int32_t* n_render, float* loss_terms) {
    const CallLock lk(b);
    if (!b) return qsp_fail(QSP_ERR_INVALID, "trace: null batch");
    QSP_HIP(hipSetDevice(b->dec->device));
    if (H) QSP_HIP(hipMemcpy(H, b->trH, sizeof(float) * (size_t)b->n_hyp * NH * NH, hipMemcpyDeviceToHost));
    if (rhs) QSP_HIP(hipMemcpy(rhs, b->trb, sizeof(float) * (size_t)b->n_hyp * NH, hipMemcpyDeviceToHost));
    if (dx) QSP_HIP(hipMemcpy(dx, b->trdx, sizeof(float) * (size_t)b->n_hyp * NH, hipMemcpyDeviceToHost));
    if (n_valid || n_render || loss_terms) {
        const HypState* hs = nullptr;
        {
            const int rc = batch_states(b, &hs);
            if (rc) return rc;
        }
        for (int h = 0; h < b->n_hyp; ++h) {
            if (n_valid) n_valid[h] = hs[h].n_valid;
            if (n_render) n_render[h] = hs[h].n_render;
            if (loss_terms) {
                loss_terms[2 * h] = hs[h].loss_sdf;
                loss_terms[2 * h + 1] = hs[h].loss_render;
            }
        }
    }
    return QSP_OK;
}

extern "C" int qsp_refine_batch_trace_rot(qsp_refine_batch* b, float* rot4) {
    if (!b || !rot4) return qsp_fail(QSP_ERR_INVALID, "trace_rot: bad argument");
    QSP_HIP(hipSetDevice(b->dec->device));
    QSP_HIP(hipMemcpy(rot4, b->trrot, sizeof(float) * (size_t)b->n_hyp * 4, hipMemcpyDeviceToHost));
    return QSP_OK;
}

extern "C" int qsp_refine_batch_rows(qsp_refine_batch* b, int enable, int32_t hyp, float* rows_sdf, float* rows_render) {
    const CallLock lk(b);
    if (!b) return qsp_fail(QSP_ERR_INVALID, "rows: null batch");
    QSP_HIP(hipSetDevice(b->dec->device));
    if (enable && !b->rows) {
        b->rows_stride = b->act_stride + b->rk_stride;
        QSP_HIP(hipMalloc((void**)&b->rows, sizeof(float) * (size_t)b->cap_hyp * b->rows_stride * NJ));
    }
    if (!enable && b->rows) {
        (void)hipFree(b->rows);
        b->rows = nullptr;
    }
    if (enable && (rows_sdf || rows_render)) {
        if (hyp < 0 || hyp >= b->n_hyp) return qsp_fail(QSP_ERR_INVALID, "rows: hyp out of range");
        const HypState* hs = nullptr;
        {
            const int rc = batch_states(b, &hs);
            if (rc) return rc;
        }
        const ObjView& ov = b->objs_h[b->hyp_obj[hyp]];
        const float* base = b->rows + (size_t)hyp * b->rows_stride * NJ;
        if (rows_sdf && ov.n_pts)
            QSP_HIP(hipMemcpy(rows_sdf, base, sizeof(float) * (size_t)ov.n_pts * NJ, hipMemcpyDeviceToHost));
        if (rows_render && hs[hyp].n_render > 0)
            QSP_HIP(hipMemcpy(rows_render, base + (size_t)ov.n_pts * NJ, sizeof(float) * (size_t)hs[hyp].n_render * NJ,
                              hipMemcpyDeviceToHost));
    }
    return QSP_OK;
}

// qsp_reconstruct_objects on a decoder (grp == nullptr, the decoder's resident batch) or on a decoder group (dec = its first
// member, the group's resident batch; obj_class = the member per object).  The caller holds the locks.
static int reconstruct_objects(qsp_decoder* dec, qsp_decoder_group* grp, const int32_t* obj_class, const qsp_joint_cfg* cfg,
                               int32_t n_obj, const float* const* pts, const int32_t* n_pts, const float* const* rays,
                               const int32_t* n_rays, const float* const* depth, const int32_t* n_fg, int32_t n_hyp,
                               const int32_t* hyp_obj, const float* t_cam_obj, const float* code, float* t_cam_obj_out,
                               float* code_out, float* loss_out, uint8_t* is_good_out) {
    if (!dec || !cfg) return qsp_fail(QSP_ERR_INVALID, "qsp_reconstruct_objects: null argument");
    if (cfg->code_len != dec->code_len) return qsp_fail(QSP_ERR_INVALID, "code_len of the optimizer config differs from the decoder's");
    if (n_obj <= 0 || n_hyp <= 0 || !pts || !n_pts || !rays || !n_rays || !depth || !n_fg || !hyp_obj)
        return qsp_fail(QSP_ERR_INVALID, "refine batch: bad argument");
    const RefineCfg c{cfg->k1, cfg->k2, cfg->k3, cfg->k4, cfg->b1, cfg->b2, cfg->lr, cfg->s_damp, cfg->cut_off, cfg->n_depth, 0, 0,
                      dec->code_len};
    BatchCaps need;
    int rc = batch_validate(c, n_obj, n_pts, n_rays, n_fg, n_hyp, hyp_obj, &need);
    if (rc) return rc;
    // The decoder's resident batch: reused when the call fits its capacities and the quantities its strides were derived from
    // (depth samples, tile size) are the same; the weights of the cost terms are launch arguments and simply replaced.  Otherwise
    // it is rebuilt with a quarter of head-room over the larger of (this call, what it held): a high-water mark, so a sequence
    // of objects of varying size settles after a few calls.  Results do not depend on the capacities (tests/test_gpu_latency.py).
    qsp_refine_batch*& arena = grp ? grp->arena : dec->arena;
    int64_t& n_arena_create = grp ? grp->n_arena_create : dec->n_arena_create;
    int64_t& n_arena_reuse = grp ? grp->n_arena_reuse : dec->n_arena_reuse;
    qsp_refine_batch* b = arena;
    if (b && (b->cfg.n_depth != c.n_depth || b->tile_p_created != dec->tile_p || b->cfg.pose_only || !batch_fits(b, need))) {
        BatchCaps grow = need;
        grow.obj = std::max(need.obj, b->cap_obj);
        grow.hyp = std::max(need.hyp, b->cap_hyp);
        grow.max_pts = std::max(need.max_pts, b->max_pts);
        grow.max_rays = std::max(need.max_rays, b->max_rays);
        grow.pts_total = std::max(need.pts_total, b->cap_pts_total);
        grow.rays_total = std::max(need.rays_total, b->cap_rays_total);
        need = grow;
        batch_free(b);
        b = arena = nullptr;
    }
    if (!b) {
        BatchCaps caps = need;
        caps.hyp = std::max(caps.hyp, 4);           // (one object x its four yaw flips: the other call shape of the reference)
        caps.max_pts += caps.max_pts / 4;
        caps.max_rays += caps.max_rays / 4;
        caps.pts_total += caps.pts_total / 4;
        caps.rays_total += caps.rays_total / 4;
        caps.pts_total = std::max<int64_t>(caps.pts_total, (int64_t)caps.max_pts);
        caps.rays_total = std::max<int64_t>(caps.rays_total, (int64_t)caps.max_rays);
        rc = batch_create(dec, c, cfg->n_iter, n_obj, pts, n_pts, rays, n_rays, depth, n_fg, n_hyp, hyp_obj, &b, false, &caps, grp,
                          obj_class);
        if (rc) return rc;
        arena = b;
        n_arena_create++;
    } else {
        QSP_HIP(hipSetDevice(dec->device));
        const int tile_p = b->cfg.tile_p;
        b->cfg = c;
        b->cfg.code_len = dec->code_len;
        b->cfg.tile_p = tile_p;
        b->n_iter_cfg = cfg->n_iter;
        rc = batch_fill(b, n_obj, pts, n_pts, rays, n_rays, depth, n_fg, n_hyp, hyp_obj, false, obj_class);
        if (rc) return rc;
        n_arena_reuse++;
    }
    rc = qsp_refine_batch_set_state(b, t_cam_obj, code);
    if (!rc) rc = qsp_refine_batch_run(b, 0);
    if (!rc) rc = qsp_refine_batch_get(b, t_cam_obj_out, code_out, loss_out, is_good_out);
    return rc;
}

extern "C" int qsp_reconstruct_objects(qsp_decoder* dec, const qsp_joint_cfg* cfg, int32_t n_obj, const float* const* pts,
                                       const int32_t* n_pts, const float* const* rays, const int32_t* n_rays,
                                       const float* const* depth, const int32_t* n_fg, int32_t n_hyp,
                                       const int32_t* hyp_obj, const float* t_cam_obj, const float* code,
                                       float* t_cam_obj_out, float* code_out, float* loss_out, uint8_t* is_good_out) {
    const CallLock lk(dec);
    return reconstruct_objects(dec, nullptr, nullptr, cfg, n_obj, pts, n_pts, rays, n_rays, depth, n_fg, n_hyp, hyp_obj, t_cam_obj,
                               code, t_cam_obj_out, code_out, loss_out, is_good_out);
}

// qsp_estimate_pose on a decoder or a decoder group (see reconstruct_objects); the caller holds the locks
static int estimate_pose(qsp_decoder* dec, qsp_decoder_group* grp, const int32_t* obj_class, int32_t n, const float* t_co_se3,
                         const float* scale, const float* const* pts, const int32_t* n_pts, const float* code, int32_t n_iter,
                         float* t_co_out) {
    if (!dec || n <= 0 || !t_co_se3 || !scale || !pts || !n_pts || !code || !t_co_out)
        return qsp_fail(QSP_ERR_INVALID, "qsp_estimate_pose: bad argument");
    for (int i = 0; i < n; ++i)
        if (n_pts[i] < 0 || (n_pts[i] > 0 && !pts[i])) return qsp_fail(QSP_ERR_INVALID, "qsp_estimate_pose: bad points of an item");
    if (std::all_of(n_pts, n_pts + n, [](int32_t m) { return m == 0; })) {      // no item has a point: nothing to launch (see below)
        std::fill(t_co_out, t_co_out + (size_t)n * 16, std::numeric_limits<float>::quiet_NaN());
        return QSP_OK;
    }
    if (n_iter <= 0) n_iter = 5;
    RefineCfg c{};
    c.n_depth = 2;
    c.pose_only = 1;
    std::vector<int32_t> hyp(n);
    for (int i = 0; i < n; ++i) hyp[i] = i;
    qsp_refine_batch* b = nullptr;
    int rc = batch_create(dec, c, n_iter, n, pts, n_pts, nullptr, nullptr, nullptr, nullptr, n, hyp.data(), &b, false, nullptr, grp,
                          obj_class);
    if (rc) return rc;
    // bake the scale into the pose: t_cam_obj[:3,:3] *= scale   (optimizer.py:57-58)
    std::vector<float> T((size_t)n * 16);
    for (int i = 0; i < n; ++i) {
        memcpy(&T[16 * i], t_co_se3 + 16 * i, 16 * sizeof(float));
        for (int r = 0; r < 3; ++r)
            for (int q = 0; q < 3; ++q) T[16 * i + 4 * r + q] *= scale[i];
    }
    rc = qsp_refine_batch_set_state(b, T.data(), code);
    if (!rc) rc = qsp_refine_batch_run(b, n_iter);
    std::vector<float> To((size_t)n * 16);
    std::vector<uint8_t> good(n);
    if (!rc) rc = qsp_refine_batch_get(b, To.data(), nullptr, nullptr, good.data());
    if (!rc)
        for (int i = 0; i < n; ++i) {
            memcpy(t_co_out + 16 * i, &To[16 * i], 16 * sizeof(float));
            for (int r = 0; r < 3; ++r)
                for (int q = 0; q < 3; ++q) t_co_out[16 * i + 4 * r + q] /= scale[i];   // optimizer.py:88
            // An item without a point left (none given, or all removed by the inlier filter): the reference divides H and b by
            // zero and hands back a matrix of NaNs.  k_solve stops such a hypothesis at the pose it had; that pose is not a result.
            if (!good[i])
                for (int e = 0; e < 16; ++e) t_co_out[16 * i + e] = std::numeric_limits<float>::quiet_NaN();
        }
    qsp_refine_batch_destroy(b);
    return rc;
}

extern "C" int qsp_estimate_pose(qsp_decoder* dec, int32_t n, const float* t_co_se3, const float* scale,
                                 const float* const* pts, const int32_t* n_pts, const float* code, int32_t n_iter,
                                 float* t_co_out) {
    const CallLock lk(dec);
    return estimate_pose(dec, nullptr, nullptr, n, t_co_se3, scale, pts, n_pts, code, n_iter, t_co_out);
}

// ---------------------------------------------------------------------------------------------------------------
// decoder groups
// ---------------------------------------------------------------------------------------------------------------
extern "C" int qsp_decoder_group_create(qsp_decoder* const* decs, int32_t n, qsp_decoder_group** out) {
    if (!decs || !out) return qsp_fail(QSP_ERR_INVALID, "qsp_decoder_group_create: null argument");
    if (n < 1 || n > QSP_GROUP_MAX) return qsp_fail(QSP_ERR_INVALID, "decoder group: 1..16 members");
    for (int i = 0; i < n; ++i)
        if (!decs[i]) return qsp_fail(QSP_ERR_INVALID, "decoder group: null member");
    qsp_decoder_group* g = new qsp_decoder_group();
    g->m.assign(decs, decs + n);
    g->lock_order = g->m;
    std::sort(g->lock_order.begin(), g->lock_order.end(), std::less<qsp_decoder*>());
    g->lock_order.erase(std::unique(g->lock_order.begin(), g->lock_order.end()), g->lock_order.end());
    g->device = decs[0]->device;
    int rc = QSP_OK;
    {
        const CallLock lk(g);
        rc = group_options(g);
        if (!rc) {
            hipError_t e = hipSetDevice(g->device);
            if (e == hipSuccess) e = hipMalloc((void**)&g->Pd, sizeof(MlpParams) * n);
            if (e != hipSuccess) rc = qsp_fail(QSP_ERR_DEVICE, hipGetErrorString(e));
        }
        if (!rc) rc = group_check(g);
    }
    if (rc) {
        qsp_decoder_group_destroy(g);
        return rc;
    }
    *out = g;
    return QSP_OK;
}

extern "C" void qsp_decoder_group_destroy(qsp_decoder_group* g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    if (g->arena) batch_free(g->arena);
    if (g->Pd) (void)hipFree(g->Pd);
    delete g;
}

extern "C" int qsp_refine_batch_create_group(qsp_decoder_group* g, const qsp_joint_cfg* cfg, int32_t n_obj, const float* const* pts,
                                             const int32_t* n_pts, const float* const* rays, const int32_t* n_rays,
                                             const float* const* depth, const int32_t* n_fg, const int32_t* obj_class, int32_t n_hyp,
                                             const int32_t* hyp_obj, qsp_refine_batch** out) {
    if (!g || !cfg) return qsp_fail(QSP_ERR_INVALID, "qsp_refine_batch_create_group: null argument");
    const CallLock lk(g);
    int rc = group_check(g);
    if (!rc && n_obj > 0) rc = group_classes(g, n_obj, obj_class);
    if (rc) return rc;
    qsp_decoder* dec = g->m[0];
    if (cfg->code_len != dec->code_len) return qsp_fail(QSP_ERR_INVALID, "code_len of the optimizer config differs from the decoders'");
    RefineCfg c{cfg->k1, cfg->k2, cfg->k3, cfg->k4, cfg->b1, cfg->b2, cfg->lr, cfg->s_damp, cfg->cut_off, cfg->n_depth, 0, 0,
                dec->code_len};
    return batch_create(dec, c, cfg->n_iter, n_obj, pts, n_pts, rays, n_rays, depth, n_fg, n_hyp, hyp_obj, out, false, nullptr, g,
                        obj_class);
}

extern "C" int qsp_reconstruct_objects_group(qsp_decoder_group* g, const qsp_joint_cfg* cfg, int32_t n_obj, const float* const* pts,
                                             const int32_t* n_pts, const float* const* rays, const int32_t* n_rays,
                                             const float* const* depth, const int32_t* n_fg, const int32_t* obj_class, int32_t n_hyp,
                                             const int32_t* hyp_obj, const float* t_cam_obj, const float* code,
                                             float* t_cam_obj_out, float* code_out, float* loss_out, uint8_t* is_good_out) {
    if (!g) return qsp_fail(QSP_ERR_INVALID, "qsp_reconstruct_objects_group: null group");
    const CallLock lk(g);
    int rc = group_check(g);
    if (!rc && n_obj > 0) rc = group_classes(g, n_obj, obj_class);
    if (rc) return rc;
    return reconstruct_objects(g->m[0], g, obj_class, cfg, n_obj, pts, n_pts, rays, n_rays, depth, n_fg, n_hyp, hyp_obj, t_cam_obj,
                               code, t_cam_obj_out, code_out, loss_out, is_good_out);
}

extern "C" int qsp_estimate_pose_group(qsp_decoder_group* g, int32_t n, const float* t_co_se3, const float* scale,
                                       const float* const* pts, const int32_t* n_pts, const float* code, const int32_t* obj_class,
                                       int32_t n_iter, float* t_co_out) {
    if (!g) return qsp_fail(QSP_ERR_INVALID, "qsp_estimate_pose_group: null group");
    const CallLock lk(g);
    int rc = group_check(g);
    if (!rc && n > 0) rc = group_classes(g, n, obj_class);
    if (rc) return rc;
    return estimate_pose(g->m[0], g, obj_class, n, t_co_se3, scale, pts, n_pts, code, n_iter, t_co_out);
}

#if (QSP_EXP_VARIANT & 16)
// timing experiment only (tools/phase_times.py): the stamps of the last launch
extern "C" int qsp_debug_timestamps(unsigned long long* out /*96*/, int* n, unsigned long long* rt /*96*/) {
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(qsp::qsp_dbg_ts), sizeof(unsigned long long) * 96);
    if (rt) (void)hipMemcpyFromSymbol(rt, HIP_SYMBOL(qsp::qsp_dbg_rt), sizeof(unsigned long long) * 96);
    (void)hipMemcpyFromSymbol(n, HIP_SYMBOL(qsp::qsp_dbg_n), sizeof(int));
    return 0;
}
#endif

#if QSP_PHASE_CLOCK
// timing experiment only (tools/phase_clock.py): ticks of the 100 MHz counter between the marks of k_sample / k_scan / k_solve, summed
// over the launches since the last call (which clears them)
extern "C" int qsp_debug_phase_ticks(unsigned long long* out /*48*/) {
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(qsp::qsp_phase_ticks), sizeof(unsigned long long) * 48);
    static const unsigned long long zero[48] = {};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(qsp::qsp_phase_ticks), zero, sizeof(zero));
    return 0;
}
#endif

#include "mesh_extract.hpp"
#include "detections.hpp"
