// sdf_body_mlp_jtj.inc: the body of k_mlp_jtj and of its decoder-group twin k_grp_mlp_jtj (sdf_kernels.hpp), included inside both.  QSP_GRP = 0: the
// single-decoder kernel, exactly as it was written before the twin existed.  QSP_GRP = 1: P is a decoder group's parameter
// array and every work item uses the entry of its object's decoder (ObjView::dec).
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    MlpSmem& s = *reinterpret_cast<MlpSmem*>(smem_raw);
    __shared__ float Tsh[16];
    __shared__ int s_item;
    const int n_items = qctl[2];
    bool tsk_first = true;
    (void)tsk_first;
  for (;;) {                                   // work queue, see k_plan
    QSP_TSK(0)
    if (threadIdx.x == 0) s_item = atomicAdd(&qctl[3], 1);
    __syncthreads();                           // also: everybody is done with the previous item's LDS
    const int item = s_item;
    if (item >= n_items) break;                // the queue only grows towards n_items: every workgroup gets here
    QSP_TSK(1)
    const int h = work[item].x, slot = work[item].y;
    const HypState& S = st[h];
    const ObjView ov = objs[S.obj];
    const bool is_sdf = slot < nw_sdf;
    const int stride = is_sdf ? nw_sdf : nw_total - nw_sdf;
    const int j0 = is_sdf ? slot : slot - nw_sdf;
    const int n = is_sdf ? ov.n_pts : S.n_render;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;

    // J~^T J~ accumulator of this wave's upper-triangular tile (waves 0..5)
    f32x16 hacc;
#pragma unroll
    for (int i = 0; i < 16; ++i) hacc[i] = 0.f;
    const int ta = (wave < 3) ? 0 : (wave < 5 ? 1 : 2);
    const int tb = (wave < 3) ? wave : (wave < 5 ? wave - 2 : 2);

    stage_code_T(s, S, Tsh);
    s.c0[threadIdx.x] = c0_all[(size_t)h * 2 * HID + threadIdx.x];
    s.c4[threadIdx.x] = c0_all[(size_t)h * 2 * HID + HID + threadIdx.x];
    const float* Pc = pts + 3 * ov.pts_off;
    const float* R = rays + 3 * ov.ray_off;
    const int32_t* rk = rend_rk + h * rk_stride;
    const float* deds = rend_deds + h * rk_stride;
    const float* rres = rend_res + h * rk_stride;
    const uint8_t* active = pt_active ? pt_active + h * act_stride : nullptr;
    const float d_min = S.d_min, d_max = S.d_max;
    const float hub = is_sdf ? cfg.b2 : cfg.b1;

    for (int t = j0; t * TILE_P < n; t += stride) {
        __syncthreads();
        if (tid < TILE_P) {
            const int v = t * TILE_P + tid;
            float x = 0, y = 0, z = 0, sc = 0.f, rr = 0.f;
            if (v < n) {
                if (is_sdf) {
                    xform(Tsh, Pc[3 * v], Pc[3 * v + 1], Pc[3 * v + 2], x, y, z);
                    sc = (active && !active[v]) ? 0.f : 1.f;
                } else {
                    const int e = rk[v];
                    const int r = e >> 6, k = e & 63;
                    const float d = depth_at(d_min, d_max, k, cfg.n_depth);
                    xform(Tsh, R[3 * r] * d, R[3 * r + 1] * d, R[3 * r + 2] * d, x, y, z);
                    sc = deds[v];
                    rr = rres[v];
                }
            }
            s.xin[4 * tid + 0] = x;
            s.xin[4 * tid + 1] = y;
            s.xin[4 * tid + 2] = z;
            s.xin[4 * tid + 3] = (v < n) ? 1.f : 0.f;   // row-valid flag
            s.rscale[tid] = sc;
            s.rres[tid] = rr;
        }
        __syncthreads();
        QSP_TSK(2)
#if QSP_GRP
        mlp_tile<true, 4, !B3, B3>(s, P + ov.dec);      // (the item's decoder)
#else
        mlp_tile<true, 4, !B3, B3>(s, P);      // (AccVGPR accumulators leave the split-bf16 tile too few ArchVGPRs)
#endif
        QSP_TSK(3)
        // ---- Jacobian rows: J~[p] = [ s*(g_x . [I | -x^ | x]) (7) | s*g_z (64) | r~ ] -------------------------------
        // G (gradient w.r.t. [code | xyz]) sits in s.act with row stride LDG; J~ goes behind it.
        float* G = s.act;
        float* Jt = s.act + TILE_P * LDG;     // [64][LDJ]
        {
            const int p = tid >> 3, sub = tid & 7;
            const float valid = s.xin[4 * p + 3];
            const float sc = s.rscale[p] * valid;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int c = sub + 8 * q;           // code column 0..63
                Jt[p * LDJ + 7 + c] = cfg.pose_only ? 0.f : sc * G[p * LDG + c];
            }
            if (sub == 0) {
                const float gx = sc * G[p * LDG + 64], gy = sc * G[p * LDG + 65], gz = sc * G[p * LDG + 66];
                const float x = s.xin[4 * p], y = s.xin[4 * p + 1], z = s.xin[4 * p + 2];
                // [I | -x^ | x]: columns t(3), omega(3), scale(1)   (loss_utils.py:166-185)
                Jt[p * LDJ + 0] = gx;
                Jt[p * LDJ + 1] = gy;
                Jt[p * LDJ + 2] = gz;
                Jt[p * LDJ + 3] = gz * y - gy * z;
                Jt[p * LDJ + 4] = gx * z - gz * x;
                Jt[p * LDJ + 5] = gy * x - gx * y;
                Jt[p * LDJ + 6] = cfg.pose_only ? 0.f : (gx * x + gy * y + gz * z);
                float r = is_sdf ? s.y[p] : s.rres[p];
                float w = cfg.pose_only ? 1.f : huber_w(r, hub);
                if (is_sdf && s.rscale[p] == 0.f) w = 0.f;      // filtered-out point (pose-only inlier mask)
                Jt[p * LDJ + 71] = valid * (w * r);
                if (res_out && is_sdf && valid != 0.f) res_out[h * act_stride + t * TILE_P + p] = r;
            }
            if (sub == 1) {
#pragma unroll
                for (int c = NJ; c < LDJ; ++c) Jt[p * LDJ + c] = 0.f;
            }
        }
        __syncthreads();
        if (rows_out) {   // parity-test tap: the augmented Jacobian rows exactly as the MFMA below consumes them
            float* ro = rows_out + (int64_t)h * rows_stride * NJ + (int64_t)(is_sdf ? 0 : ov.n_pts) * NJ;
            for (int e = tid; e < TILE_P * NJ; e += MLP_THREADS) {
                const int p = e / NJ, c = e - p * NJ;
                const int v = t * TILE_P + p;
                if (v < n) ro[(int64_t)v * NJ + c] = Jt[p * LDJ + c];
            }
        }
        if (wave < 6) {
            const float* A = Jt + (lane >> 5) * LDJ + 32 * ta + (lane & 31);
            const float* B = Jt + (lane >> 5) * LDJ + 32 * tb + (lane & 31);
#pragma unroll 8
            for (int ks = 0; ks < TILE_P / 2; ++ks) hacc = mfma32t<!B3>(A[2 * ks * LDJ], B[2 * ks * LDJ], hacc);
            mfma_acc_settle<!B3>(hacc);
        }
        QSP_TSK(4)
    }
    // partial slot [h][slot][packed upper triangle of 72 x 72]
    if (wave < 6) part_store(partials + ((int64_t)h * nw_total + slot) * PART_FLOATS, ta, tb, lane, hacc);
    QSP_TSK(5)
    tsk_first = false;
  }
