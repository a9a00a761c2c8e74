// sdf_body_mlp_fwd_h1.inc: the body of k_mlp_fwd_h1 and of its decoder-group twin k_grp_mlp_fwd_h1 (sdf_kernels.hpp), included inside both.  QSP_GRP = 0: the
// single-decoder kernel, exactly as it was written before the twin existed.  QSP_GRP = 1: P is a decoder group's parameter
// array and every work item uses the entry of its object's decoder (ObjView::dec).
    // stage_idx != nullptr: the tiles run over the hypothesis's stage list (positions in its valid-sample list, k_stage_list)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    MlpSmemH1& s = *reinterpret_cast<MlpSmemH1*>(smem_raw);
    __shared__ float Tsh[16];
    __shared__ int s_item;
    const int n_items = qctl[0];
    float amax = 0.f;
    int h_cached = -1;
#if QSP_GRP
    int dec_staged = -1;                   // the decoder whose constants are in LDS (staged per item, below)
#else
    {   // the decoder's constants, once per workgroup
        const MlpParams& Pp = *P;
        for (int i = threadIdx.x; i < HID; i += 64 * NW) s.w8[i] = Pp.w8[i];
#pragma unroll
        for (int l = 1; l < 8; ++l)
            for (int i = threadIdx.x; i < HID; i += 64 * NW) s.bias[(l - 1) * HID + i] = Pp.bias[l][i];
    }
#endif
    for (;;) {
        if (threadIdx.x == 0) s_item = atomicAdd(&qctl[1], 1);
        __syncthreads();                       // also: everybody is done with the previous item's LDS
        const int item = s_item;
        if (item >= n_items) break;            // the queue only grows towards n_items: every workgroup gets here
        const int h = work[item].x, t = work[item].y;
        HypState& S = st[h];
        const int n = stage_idx ? S.n_stage : S.n_valid;
        const int32_t* stg = stage_idx ? stage_idx + h * rk_stride : nullptr;
        const ObjView ov = objs[S.obj];
        const float* R = rays + 3 * ov.ray_off;
        const int32_t* rk = valid_rk + h * rk_stride;
        float* out = sdf_valid + h * rk_stride;
        if (h != h_cached) {                   // per-hypothesis staging: pose, code parts of layers 0 and 4
            if (threadIdx.x >= 64 && threadIdx.x < 80) Tsh[threadIdx.x - 64] = S.T_oc[threadIdx.x - 64];
            for (int i = threadIdx.x; i < HID; i += 64 * NW) {
                s.c0[i] = c0_all[(size_t)h * 2 * HID + i];
                s.c4[i] = c0_all[(size_t)h * 2 * HID + HID + i];
            }
            h_cached = h;
        }
#if QSP_GRP
        if (ov.dec != dec_staged) {            // the item's decoder's constants (everybody is done with the previous item's LDS)
            const MlpParams& Pp = P[ov.dec];
            for (int i = threadIdx.x; i < HID; i += 64 * NW) s.w8[i] = Pp.w8[i];
#pragma unroll
            for (int l = 1; l < 8; ++l)
                for (int i = threadIdx.x; i < HID; i += 64 * NW) s.bias[(l - 1) * HID + i] = Pp.bias[l][i];
            dec_staged = ov.dec;
        }
#endif
        const float d_min = S.d_min, d_max = S.d_max;
        __syncthreads();
        if (threadIdx.x < H1_ROWS) {
            const int v = t * H1_ROWS + threadIdx.x;
            float x = 0, y = 0, z = 0;
            if (v < n) {
                const int e = rk[stg ? stg[v] : v];
                const int r = e >> 6, k = e & 63;
                const float d = depth_at(d_min, d_max, k, cfg.n_depth);
                xform(Tsh, R[3 * r] * d, R[3 * r + 1] * d, R[3 * r + 2] * d, x, y, z);
            }
            s.xin[4 * threadIdx.x + 0] = x;
            s.xin[4 * threadIdx.x + 1] = y;
            s.xin[4 * threadIdx.x + 2] = z;
            s.xin[4 * threadIdx.x + 3] = 0.f;
        }
        __syncthreads();
#if QSP_GRP
        mlp_tile_h1<2, NW>(s, P + ov.dec, amax);
#else
        mlp_tile_h1<2, NW>(s, P, amax);
#endif
        if (threadIdx.x < H1_ROWS) {           // (waves 0 and 1, all lanes)
            int v = t * H1_ROWS + threadIdx.x;
            bool in = false, audit = false;
            if (v < n) {
                if (stg) v = stg[v];           // (from here on v is the sample's position in the valid list)
                const float y = s.y[threadIdx.x];
                out[v] = y;
                in = !(fabsf(y) >= band_th);   // (a NaN goes to the second pass as well)
                audit = !in && screen_audit_pick(h, v, cfg.iter, audit_one_in);      // a sample of the OUT-of-band ones (above)
            }
            const unsigned long long m = __ballot(in || audit);
            const int lane = threadIdx.x & 63;
            int base = 0;
            if (lane == 0 && m) base = atomicAdd(&S.n_band, __popcll(m));
            base = __builtin_amdgcn_readfirstlane(base);
            if (in || audit) band_idx[h * rk_stride + base + __popcll(m & ((1ull << lane) - 1ull))] = audit ? (v | BAND_AUDIT_BIT) : v;
        }
    }
    if (!(amax <= H2_MAX)) *P->range_flag = 1;
