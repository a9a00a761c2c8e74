// sdf_body_mlp_fwd_h2.inc: the body of k_mlp_fwd_h2 and of its decoder-group twin k_grp_mlp_fwd_h2 (sdf_kernels.hpp), included inside both.  QSP_GRP = 0: the
// single-decoder kernel, exactly as it was written before the twin existed.  QSP_GRP = 1: P is a decoder group's parameter
// array and every work item uses the entry of its object's decoder (ObjView::dec).
    // band_idx != nullptr: second pass of the screened forward -- the tiles run over the hypothesis's band list (indices into
    // its valid-sample list written by k_mlp_fwd_h1) and overwrite those samples' screening values.  On the way the largest
    // |s1 - s3| over the band samples is kept (*screen_dmax, the bits of a non-negative float): the quantity the screening margin
    // has to cover, measured on every run -- the host repeats a run unscreened if it ever comes near the margin.  Entries flagged
    // BAND_AUDIT_BIT are out-of-band samples under audit (above): screen_dmax[1] counts those the screening pass clamped wrongly,
    // (unsigned long long*)(screen_dmax + 2) how many were audited.
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    MlpSmem& s = *reinterpret_cast<MlpSmem*>(smem_raw);
    __shared__ float Tsh[16];
    __shared__ int s_item;
    const int n_items = qctl[0];
    constexpr int TP = 32 * NR;
    bool staged = false;
    float amax = 0.f, dmax = 0.f;
    int h_cached = -1;
#if QSP_GRP
    int dec_staged = -1;                   // the decoder whose constants the tile has staged
#endif
    for (;;) {
        if (threadIdx.x == 0) s_item = atomicAdd(&qctl[1], 1);
        __syncthreads();                       // also: everybody is done with the previous item's LDS
        const int item = s_item;
        if (item >= n_items) break;            // the queue only grows towards n_items: every workgroup gets here
        const int h = work[item].x, t = work[item].y;
        const HypState& S = st[h];
        const int n = band_idx ? S.n_band : S.n_valid;
        const ObjView ov = objs[S.obj];
        const float* R = rays + 3 * ov.ray_off;
        const int32_t* rk = valid_rk + h * rk_stride;
        const int32_t* sel = band_idx ? band_idx + h * rk_stride : nullptr;
        float* out = sdf_valid + h * rk_stride;
        if (h != h_cached) {                   // per-hypothesis staging: code, pose, layer-0 code part
            stage_code_T(s, S, Tsh);
            for (int i = threadIdx.x; i < HID; i += 64 * NW) {
                s.c0[i] = c0_all[(size_t)h * 2 * HID + i];
                s.c4[i] = c0_all[(size_t)h * 2 * HID + HID + i];
            }
            h_cached = h;
        }
        const float d_min = S.d_min, d_max = S.d_max;
        __syncthreads();
        if (threadIdx.x < TP) {
            const int v = t * TP + threadIdx.x;
            float x = 0, y = 0, z = 0;
            if (v < n) {
                const int e = rk[sel ? (sel[v] & ~BAND_AUDIT_BIT) : v];
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
        mlp_tile_h2<false, 2, !NARROW, NR, NW, NARROW>(s, P + ov.dec, amax, ov.dec != dec_staged);   // (constants: again when the decoder changes)
        dec_staged = ov.dec;
        (void)staged;
#else
        mlp_tile_h2<false, 2, !NARROW, NR, NW, NARROW>(s, P, amax, !staged);      // (the decoder's constants: staged by the first tile of the workgroup)
        staged = true;
#endif
        if (threadIdx.x < TP) {
            const int v = t * TP + threadIdx.x;
            bool audited = false, wrong = false;
            if (v < n) {
                const int ent = sel ? sel[v] : v;
                const int idx = ent & ~BAND_AUDIT_BIT;
                const float y = s.y[threadIdx.x];
                if (sel) {
                    const float s1 = out[idx];                         // (out[idx] still holds the screening value s1)
                    dmax = fmaxf(dmax, fabsf(s1 - y));
                    audited = (ent & BAND_AUDIT_BIT) != 0;
                    wrong = audited && (!(fabsf(y) >= cfg.cut_off) || (s1 < 0.f) != (y < 0.f));
                }
                out[idx] = y;
            }
            if (sel && screen_dmax && threadIdx.x < 64) {              // (counted per tile: nothing stays live across the tile loop)
                const unsigned long long ma = __ballot(audited), mw = __ballot(wrong);
                if (threadIdx.x == 0 && ma) atomicAdd(reinterpret_cast<unsigned long long*>(screen_dmax + 2), (unsigned long long)__popcll(ma));
                if (threadIdx.x == 0 && mw) atomicAdd(screen_dmax + 1, (unsigned int)__popcll(mw));
            }
        }
    }
    if (band_idx && screen_dmax && threadIdx.x < 64) {      // the first wave holds every row's difference (TP <= 64)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) dmax = fmaxf(dmax, __shfl_xor(dmax, o, 64));
        if (threadIdx.x == 0 && dmax > 0.f) atomicMax(screen_dmax, __float_as_uint(dmax));
    }
    if (!(amax <= H2_MAX)) *P->range_flag = 1;
