// sdf_body_mlp_fwd.inc: the body of k_mlp_fwd and of its decoder-group twin k_grp_mlp_fwd (sdf_kernels.hpp), included inside both.  QSP_GRP = 0: the
// single-decoder kernel, exactly as it was written before the twin existed.  QSP_GRP = 1: P is a decoder group's parameter
// array and every work item uses the entry of its object's decoder (ObjView::dec).
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    MlpSmem& s = *reinterpret_cast<MlpSmem*>(smem_raw);
    __shared__ float Tsh[16];
    __shared__ int s_item;
    const int n_items = qctl[0];
    int h_cached = -1;
    for (;;) {
        if (threadIdx.x == 0) s_item = atomicAdd(&qctl[1], 1);
        __syncthreads();                       // also: everybody is done with the previous item's LDS
        const int item = s_item;
        if (item >= n_items) break;            // the queue only grows towards n_items: every workgroup gets here
        const int h = work[item].x, t = work[item].y;
        const HypState& S = st[h];
        const int n = S.n_valid;
        const ObjView ov = objs[S.obj];
        const float* R = rays + 3 * ov.ray_off;
        const int32_t* rk = valid_rk + h * rk_stride;
        float* out = sdf_valid + h * rk_stride;
        if (h != h_cached) {                   // per-hypothesis staging: code, pose, layer-0 code part
            stage_code_T(s, S, Tsh);
            s.c0[threadIdx.x] = c0_all[(size_t)h * 2 * HID + threadIdx.x];
            s.c4[threadIdx.x] = c0_all[(size_t)h * 2 * HID + HID + threadIdx.x];
            h_cached = h;
        }
        const float d_min = S.d_min, d_max = S.d_max;
        __syncthreads();
        if (threadIdx.x < TILE_P) {
            const int v = t * TILE_P + threadIdx.x;
            float x = 0, y = 0, z = 0;
            if (v < n) {
                const int e = rk[v];
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
        if (BF3) mlp_tile_bf3<QSP_BF3_PF>(s, P + ov.dec);      // (the item's decoder)
        else mlp_tile<false, 4>(s, P + ov.dec);
#else
        if (BF3) mlp_tile_bf3<QSP_BF3_PF>(s, P);
        else mlp_tile<false, 4>(s, P);
#endif
        if (threadIdx.x < TILE_P) {
            const int v = t * TILE_P + threadIdx.x;
            if (v < n) out[v] = s.y[threadIdx.x];
        }
    }
