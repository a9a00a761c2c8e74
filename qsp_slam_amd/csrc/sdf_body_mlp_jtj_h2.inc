// sdf_body_mlp_jtj_h2.inc: the body of k_mlp_jtj_h2 and of its decoder-group twin k_grp_mlp_jtj_h2 (sdf_kernels.hpp), included inside both.  QSP_GRP = 0: the
// single-decoder kernel, exactly as it was written before the twin existed.  QSP_GRP = 1: P is a decoder group's parameter
// array and every work item uses the entry of its object's decoder (ObjView::dec).
    constexpr int NT = 64 * NW;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    MlpSmem& s = *reinterpret_cast<MlpSmem*>(smem_raw);
    __shared__ float Tsh[16];
    __shared__ int s_item;
    constexpr int TP = 32 * NR, SUBS = NT / TP;      // threads per Jacobian row
    bool staged = false;
    float amax = 0.f;
    int item = -1, t = 0;       // the work item in hand and its current tile; item < 0: pop the next one (see k_plan)
#if QSP_GRP
    int dec = 0, dec_staged = -1;      // the item's decoder (one scalar more across the tile), the decoder whose constants are in LDS
#endif
    for (;;) {
        // ---- phase 1: pop / stage.  Nothing computed here is used behind the tile. ------------------------------------------
        {
            const jtj_kargs_t A = jtj_kernargs();
            int tid = threadIdx.x;
            asm volatile("" : "+v"(tid));     // opaque per phase: otherwise every LDS address that depends on the lane is computed once
                                              // per kernel, ahead of the item loop, and held (spilled) across the tile
            const bool fresh = item < 0;
            if (fresh) {
                if (tid == 0) s_item = atomicAdd(&A->qctl[3], 1);
                __syncthreads();                       // also: everybody is done with the previous item's LDS
                item = __builtin_amdgcn_readfirstlane(s_item);
                if (item >= A->qctl[2]) break;         // the queue only grows towards its length: every workgroup gets here
            } else {
                __syncthreads();                       // the previous tile's epilogue has read its Jacobian rows
            }
            const int2 wk = A->work[item];
            const int h = wk.x, slot = wk.y;
            const HypState& S = A->st[h];
            const ObjView ov = A->objs[S.obj];
            const int nw_sdf = A->nw_sdf;
            const bool is_sdf = slot < nw_sdf;
            const int n = is_sdf ? ov.n_pts : S.n_render;
#if QSP_GRP
            dec = __builtin_amdgcn_readfirstlane(ov.dec);
#endif
            if (fresh) {
                t = is_sdf ? slot : slot - nw_sdf;
                if (tid < CODE_LEN) s.code[tid] = S.code[tid];
                if (tid >= 64 && tid < 80) Tsh[tid - 64] = S.T_oc[tid - 64];
                const float* c0 = A->c0_all + (size_t)h * 2 * HID;
                for (int i = tid; i < HID; i += NT) {
                    s.c0[i] = c0[i];
                    s.c4[i] = c0[HID + i];
                }
                __syncthreads();                       // Tsh is read below
            }
            if (tid < TP) {
                const int v = t * TP + tid;
                float x = 0, y = 0, z = 0, sc = 0.f, rr = 0.f;
                if (v < n) {
                    if (is_sdf) {
                        const float* Pc = A->pts + 3 * ov.pts_off;
                        const uint8_t* active = A->pt_active ? A->pt_active + h * A->act_stride : nullptr;
                        xform(Tsh, Pc[3 * v], Pc[3 * v + 1], Pc[3 * v + 2], x, y, z);
                        sc = (active && !active[v]) ? 0.f : 1.f;
                    } else {
                        const float* R = A->rays + 3 * ov.ray_off;
                        const int64_t ro = h * A->rk_stride;
                        const int e = A->rend_rk[ro + v];
                        const int r = e >> 6, k = e & 63;
                        const float d = depth_at(S.d_min, S.d_max, k, A->cfg.n_depth);
                        xform(Tsh, R[3 * r] * d, R[3 * r + 1] * d, R[3 * r + 2] * d, x, y, z);
                        sc = A->rend_deds[ro + v];
                        rr = A->rend_res[ro + v];
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
        }
        // ---- the tile: live across it are item, t, staged (scalars) and amax ---------------------------------------------------
        {
#if QSP_GRP
            const MlpParams* Pm = jtj_kernargs()->P + dec;
            mlp_tile_h2<true, 2, false, NR, NW, NARROW>(s, Pm, amax, dec != dec_staged);    // (constants: again when the decoder changes)
            dec_staged = dec;
            (void)staged;
#else
            const MlpParams* Pm = jtj_kernargs()->P;
            mlp_tile_h2<true, 2, false, NR, NW, NARROW>(s, Pm, amax, !staged);
            staged = true;
#endif
        }
        // ---- phase 2: Jacobian rows  J~[p] = [ s*(g_x . [I | -x^ | x]) (7) | s*g_z (64) | r~ ],  J~^T J~ -----------------------
        // G (gradient w.r.t. [code | xyz]) sits in s.act with row stride LDG; J~ goes behind it.
        {
            asm volatile("" : "+s"(item), "+s"(t));
            const jtj_kargs_t A = jtj_kernargs();
            int tid = threadIdx.x;
            asm volatile("" : "+v"(tid));
            const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
            const int2 wk = A->work[item];
            const int h = wk.x, slot = wk.y;
            const HypState& S = A->st[h];
            const ObjView ov = A->objs[S.obj];
            const int nw_sdf = A->nw_sdf, nw_total = A->nw_total;
            const bool is_sdf = slot < nw_sdf;
            const int n = is_sdf ? ov.n_pts : S.n_render;
            const int j0 = is_sdf ? slot : slot - nw_sdf;
            const int stride = is_sdf ? nw_sdf : nw_total - nw_sdf;
            const int pose_only = A->cfg.pose_only;
            const float hub = is_sdf ? A->cfg.b2 : A->cfg.b1;
            float* G = s.act;
            float* Jt = s.act + TILE_P * LDG;   /* (behind the 64-row G image whatever the tile size) */     // [64][LDJ]
            {
                const int p = tid / SUBS, sub = tid % SUBS;
                const float valid = s.xin[4 * p + 3];
                const float sc = s.rscale[p] * valid;
#pragma unroll
                for (int q = 0; q < CODE_LEN / SUBS; ++q) {
                    const int c = sub + SUBS * q;        // code column 0..63
                    Jt[p * LDJ + 7 + c] = pose_only ? 0.f : sc * G[p * LDG + c];
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
                    Jt[p * LDJ + 6] = pose_only ? 0.f : (gx * x + gy * y + gz * z);
                    float r = is_sdf ? s.y[p] : s.rres[p];
                    float w = pose_only ? 1.f : huber_w(r, hub);
                    if (is_sdf && s.rscale[p] == 0.f) w = 0.f;      // filtered-out point (pose-only inlier mask)
                    Jt[p * LDJ + 71] = valid * (w * r);
                    float* res_out = A->res_out;
                    if (res_out && is_sdf && valid != 0.f) res_out[h * A->act_stride + t * TP + p] = r;
                }
                if (sub == 1) {
#pragma unroll
                    for (int c = NJ; c < LDJ; ++c) Jt[p * LDJ + c] = 0.f;
                }
            }
            __syncthreads();
            if (A->rows_out) {   // parity-test tap: the augmented Jacobian rows exactly as the MFMA below consumes them
                float* ro = A->rows_out + (int64_t)h * A->rows_stride * NJ + (int64_t)(is_sdf ? 0 : ov.n_pts) * NJ;
                for (int e = tid; e < TP * NJ; e += NT) {
                    const int p = e / NJ, c = e - p * NJ;
                    const int v = t * TP + p;
                    if (v < n) ro[(int64_t)v * NJ + c] = Jt[p * LDJ + c];
                }
            }
            // upper-triangular 32x32 tiles in the order (0,0) (0,1) (0,2) (1,1) (1,2) (2,2).  Four waves: tile w on every wave, tile
            // w + 4 on waves 0, 1; eight waves: tile w on waves 0..5.  Partial slot [h][slot][packed upper triangle].
            float* out = A->partials + ((int64_t)h * nw_total + slot) * PART_FLOATS;
            const bool first = t == j0;
            if (NW == 4 || wave < 6) {
                const int ta0 = wave < 3 ? 0 : (wave < 5 ? 1 : 2), tb0 = wave < 3 ? wave : (wave < 5 ? wave - 2 : 2);
                f32x16 hacc;
                part_load(out, ta0, tb0, lane, first, hacc);
                const float* Aj = Jt + (lane >> 5) * LDJ + 32 * ta0 + (lane & 31);
                const float* Bj = Jt + (lane >> 5) * LDJ + 32 * tb0 + (lane & 31);
#pragma unroll 8
                for (int ks = 0; ks < TP / 2; ++ks) hacc = mfma32t<false>(Aj[2 * ks * LDJ], Bj[2 * ks * LDJ], hacc);
                part_store(out, ta0, tb0, lane, hacc);
            }
            if (NW == 4 && wave < 2) {
                const int ta1 = wave == 0 ? 1 : 2, tb1 = 2;
                f32x16 hacc;
                part_load(out, ta1, tb1, lane, first, hacc);
                const float* Aj = Jt + (lane >> 5) * LDJ + 32 * ta1 + (lane & 31);
                const float* Bj = Jt + (lane >> 5) * LDJ + 32 * tb1 + (lane & 31);
#pragma unroll 8
                for (int ks = 0; ks < TP / 2; ++ks) hacc = mfma32t<false>(Aj[2 * ks * LDJ], Bj[2 * ks * LDJ], hacc);
                part_store(out, ta1, tb1, lane, hacc);
            }
            // the item's next tile (more than nw_sdf x TP surface points, or more than 16 x TP render rows), or the next item
            t += stride;
            if (t * TP >= n) item = -1;
        }
    }
    if (!(amax <= H2_MAX)) *jtj_kernargs()->P->range_flag = 1;
