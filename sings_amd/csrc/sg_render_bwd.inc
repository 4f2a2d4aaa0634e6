// Backward composite kernels of sg_render.hip, included there twice: SG_BWD_AUX 0 defines sg_render_bwd_kernel and
// sg_render_bwd_sparse_kernel, SG_BWD_AUX 1 sg_render_bwd_aux_kernel and sg_render_bwd_sparse_aux_kernel, which also take the
// depth / alpha adjoints (`ax`: SG_BWD_PASS) and write the dL/dz plane, frame blockIdx.y's (SG_BWD_AUX_FRAME_OFFSETS).  In the plain
// kernels every AUX branch is dead.
// (no include guard: included once per variant)

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8)))
#if SG_BWD_AUX
sg_render_bwd_aux_kernel(SG_BWD_PARAMS, SgAuxBwd ax)
#else
sg_render_bwd_kernel(SG_BWD_PARAMS)
#endif
{
    constexpr bool AUX = SG_BWD_AUX;
#if !SG_BWD_AUX
    const SgAuxBwd ax = { };
#endif
    __shared__ float4 sR[SG_BCH][3];           // staged entry: (mean x, mean y, A', B') (C', opacity, colour 0, 1) (colour 2, z [AUX], -, -)
    __shared__ uint32_t sM[SG_BCH];
    __shared__ uint16_t sList[4][SG_BB];
    __shared__ float sG[4][SG_BB][9 + AUX];    // per-quadrant reduced partials of the batch; [8] = SG_UNSET: quadrant w wrote nothing
    __shared__ uint32_t smax[4];
    SG_STAMP_SCOPE
    SG_BWD_FRAME_OFFSETS;
#if SG_BWD_AUX
    SG_BWD_AUX_FRAME_OFFSETS;
#endif
    // one workgroup per work item (tile, depth segment); the item list is in tile order, so the XCD-aware map
    // over the ACTUAL item count keeps neighbouring tiles on one L2.  The grid is an upper bound.
    (void)T; (void)nblocks;
    const int nitems = header[1] ? 0 : (int)header[5];             // nothing to do after a capacity overflow
    const int it = sg_tile_of_block(blockIdx.x);
    if (it >= nitems) return;
    const uint32_t item = items[it];
    const int tile = (int)(item & 0xfffffu), seg = (int)(item >> 20);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int tx = tile % gx, ty = tile / gx;
    const int X0 = tx * 16, Y0 = ty * 16;
    const int px = X0 + 8 * (wave & 1) + (lane & 7), py = Y0 + 8 * (wave >> 1) + (lane >> 3);
    const bool inside = px < W && py < H;
    const float pxf = (float)px, pyf = (float)py;
    const uint2 range = ranges[tile];
    const int n = (int)(range.y - range.x);
    const uint32_t cks = ck_start[tile];
    const int lo = seg * SG_SEG;                                   // this item: entries [lo, hi)
    const int hi = cks != 0xffffffffu && lo + SG_SEG < n ? lo + SG_SEG : n;
    if (lo >= n) return;
    const size_t pid = (size_t)py * W + px, hw = (size_t)H * W;
    // per-pixel state: running T, colour accumulated BEHIND the current entry, dL/dpixel, T_final <bg, dL/dpixel>
    const float Tfin = inside ? final_T[pid] : 0.0f;
    const uint32_t ncq = inside ? n_contrib[pid] : 0u;
    const float d0 = inside ? dL_dpix[pid] : 0.0f, d1 = inside ? dL_dpix[hw + pid] : 0.0f, d2 = inside ? dL_dpix[2 * hw + pid] : 0.0f;
    const float dD = AUX && inside && ax.dL_ddepth ? ax.dL_ddepth[pid] : 0.0f, dA = AUX && inside && ax.dL_dalpha ? ax.dL_dalpha[pid] : 0.0f;
    const float tb = AUX ? Tfin * (bg[0] * d0 + bg[1] * d1 + bg[2] * d2 - dA) : Tfin * (bg[0] * d0 + bg[1] * d1 + bg[2] * d2);
    // (the colour behind enters the gradient only through <S, dL/dpixel>: ONE running scalar Sd instead of three channels)
    float Tr = Tfin, Sd = 0.0f;
    // Not the last segment, and this pixel has contributors behind it: start from the forward checkpoint at `hi`.
    // T in front of entry hi; S = colour composited behind it, normalised by that T.  (A pixel with ncq <= hi has
    // nothing behind: final state.  ncq > hi implies the forward reached that boundary with this pixel live.)
    if (hi < n && ncq > (uint32_t)hi && cks + (uint32_t)(hi / SG_SEG) < ck_cap) {
        const float4 cb = ckpt[(size_t)(cks + (uint32_t)(hi / SG_SEG)) * 256 + tid];
        const float4 cf = ckpt[(size_t)cks * 256 + tid];
        const float rT = 1.0f / cb.x;
        Tr = cb.x;
        Sd = fmaf((cf.w - cb.w) * rT, d2, fmaf((cf.z - cb.z) * rT, d1, (cf.y - cb.y) * rT * d0));
        if (AUX) {                                                     // + D_behind dL/ddepth, normalised like the colour
            const float Db = ax.ckD[(size_t)(cks + (uint32_t)(hi / SG_SEG)) * 256 + tid], Df = ax.ckD[(size_t)cks * 256 + tid];
            Sd = fmaf((Df - Db) * rT, dD, Sd);
        }
    }
    uint32_t m = ncq;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { uint32_t u = __shfl_xor(m, o, 64); m = u > m ? u : m; }
    const int maxq = (int)__builtin_amdgcn_readfirstlane(m);          // this quadrant's deepest contributor
    if (lane == 0) smax[wave] = m;
    if (tid < SG_BB) {
#pragma unroll
        for (int w = 0; w < 4; w++) sG[w][tid][8] = __uint_as_float(SG_UNSET);
    }
    __syncthreads();
    const int max_contrib = (int)max(max(smax[0], smax[1]), max(smax[2], smax[3]));
    const float ddelx_dx = 0.5f * (float)W, ddely_dy = 0.5f * (float)H;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const int cslot = lane == 63 ? 8 : sg_red_idx(lane);
    for (int ch = (hi - 1) / SG_BCH; ch >= lo / SG_BCH; ch--) {
        const int cbase = ch * SG_BCH;
        const int ccnt = hi - cbase < SG_BCH ? hi - cbase : SG_BCH;
        // ---- stage the chunk (threads 0..SG_BCH-1): records, quadrant mask, gradient-record slot
        uint32_t rslot = 0xffffffffu;
        float opac = 0.0f, cA = 0.0f, cB = 0.0f, cC = 0.0f;
        if (tid < ccnt) {
            const int e = cbase + tid;
            const uint32_t gid = point_list[range.x + e];
            // quadrants the forward composited this entry in: nothing else can carry a gradient, so neither the
            // rectangle tests nor the two record gathers are repeated for the rest
            // (a long tile of a few-tile frame was composited by four workgroups, one mask plane each: sg_render_fwd_body)
            uint32_t mk = 0u;
            if (e < max_contrib) {
                mk = pair_mask[range.x + e];
                if (split_long && n > SG_WSORT_MAX)
                    mk = (mk & 1u) | (pair_mask[(size_t)mask_plane + range.x + e] & 2u) | (pair_mask[2 * (size_t)mask_plane + range.x + e] & 4u) |
                         (pair_mask[3 * (size_t)mask_plane + range.x + e] & 8u);
            }
            const float4 c4 = recC[SG_REC_STRIDE * (size_t)gid];
            if (mk) {
                const float4 a = recA[SG_REC_STRIDE * (size_t)gid], b = recB[SG_REC_STRIDE * (size_t)gid];
                opac = b.y; cA = a.z; cB = a.w; cC = b.x;
                sR[tid][0] = make_float4(a.x, a.y, SG_KA * a.z, SG_KB * a.w);
                sR[tid][1] = make_float4(SG_KA * b.x, b.y, b.z, b.w);
                sR[tid][2].x = c4.x;
                if (AUX) sR[tid][2].y = ax.depth[gid];
            }
            const uint32_t goff = __float_as_uint(c4.y), mn = __float_as_uint(c4.z), wh = __float_as_uint(c4.w);
            const int x0 = mn & 0xffff, y0 = mn >> 16, rw = wh & 0xffff;
            rslot = goff + (uint32_t)((ty - y0) * rw + (tx - x0));
            sM[tid] = mk;
        }
        __syncthreads();
        for (int kb = (ccnt - 1) / SG_BB; kb >= 0; kb--) {
            const int b0 = kb * SG_BB, base = cbase + b0;                  // the batch inside the chunk / inside the list
            const int cnt = ccnt - b0 < SG_BB ? ccnt - b0 : SG_BB;
            // ---- each wave: the entries that can reach its quadrant, back to front
            if (base < maxq) {
                uint16_t *list = sList[wave];
                const int lim = maxq - base < cnt ? maxq - base : cnt;         // entries >= maxq touch no pixel here
                const int nl = sg_compact_quadrant<1>(sM + b0, lim, wave, lane, lt, list, SG_BB);
                const uint32_t ncq_b = ncq > (uint32_t)base ? ncq - (uint32_t)base : 0u;   // contributors of this pixel inside the batch
                for (int i = nl - 1; i >= 0; i--) {
                    const uint32_t k = list[i];
                    const float4 ga = sR[b0 + k][0], gb = sR[b0 + k][1];
                    const float gc = sR[b0 + k][2].x;
                    const float gz = AUX ? sR[b0 + k][2].y : 0.0f;
                    SG_BWD_PASS(k, k);
                }
            }
            __syncthreads();
            // ---- combine the quadrants in a fixed order, store the record, re-arm the slots (the thread that staged the entry)
            if (tid >= b0 && tid < b0 + cnt) {
                const int q0 = tid - b0;
                float s[9 + AUX] = { };
#pragma unroll
                for (int w = 0; w < 4; w++)
                    if (__float_as_uint(sG[w][q0][8]) != SG_UNSET) {
#pragma unroll
                        for (int q = 0; q < 9 + AUX; q++) s[q] += sG[w][q0][q];
                        sG[w][q0][8] = __uint_as_float(SG_UNSET);
                    }
                if (rslot < cap) {
                    const float no = -opac, nh = 0.5f * no;              // -opacity, -opacity / 2
                    const float m0 = fmaf(cA, s[0], cB * s[1]), m1 = fmaf(cB, s[0], cC * s[1]);   // conic . first moments
                    grec_a[2 * (size_t)rslot] = make_float4(no * ddelx_dx * m0, no * ddely_dy * m1, nh * s[2], nh * s[3]);
                    grec_a[2 * (size_t)rslot + 1] = make_float4(nh * s[4], s[5], s[6], s[7]);
                    grec_b[rslot] = s[8];
                    if (AUX) ax.dz[rslot] = s[9];
                }
            }
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6, 6)))
#if SG_BWD_AUX
sg_render_bwd_sparse_aux_kernel(SG_BWD_PARAMS, const uint32_t *__restrict__ perm, uint8_t *__restrict__ rec_valid, SgAuxBwd ax)
#else
sg_render_bwd_sparse_kernel(SG_BWD_PARAMS, const uint32_t *__restrict__ perm, uint8_t *__restrict__ rec_valid)
#endif
{
    constexpr bool AUX = SG_BWD_AUX;
#if !SG_BWD_AUX
    const SgAuxBwd ax = { };
#endif
    __shared__ float4 sR[SG_BS][3];            // staged entry: (mean x, mean y, A', B') (C', opacity, colour 0, 1) (colour 2, z [AUX], -, -)
    __shared__ uint32_t sM[SG_BS];
    __shared__ uint16_t sList[4][SG_BB];
    __shared__ float sG[4][SG_BB][9 + AUX];    // per-quadrant reduced partials of the sub-batch; [8] = SG_UNSET: quadrant w wrote nothing
    __shared__ uint32_t smax[4];
    (void)T; (void)nblocks;
    SG_BWD_FRAME_OFFSETS;
#if SG_BWD_AUX
    SG_BWD_AUX_FRAME_OFFSETS;
#endif
    perm = sg_at(perm, (size_t)blockIdx.y * bt.bin); rec_valid = sg_at(rec_valid, (size_t)blockIdx.y * bt.bin);
    const int nitems = header[1] ? 0 : (int)header[5];
    if ((int)blockIdx.x >= nitems) return;
    const uint32_t pit = perm[blockIdx.x];
    const uint32_t item = items[pit];                               // dispatch order = heaviest first
    const int tile = (int)(item & 0xfffffu), seg = (int)(item >> 20);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int tx = tile % gx, ty = tile / gx;
    const int X0 = tx * 16, Y0 = ty * 16;
    const int px = X0 + 8 * (wave & 1) + (lane & 7), py = Y0 + 8 * (wave >> 1) + (lane >> 3);
    const bool inside = px < W && py < H;
    const float pxf = (float)px, pyf = (float)py;
    const uint2 range = ranges[tile];
    const int n = (int)(range.y - range.x);
    const uint32_t cks = ck_start[tile];
    const int lo = seg * SG_SEG;                                   // this item: entries [lo, hi)
    const int hi = cks != 0xffffffffu && lo + SG_SEG < n ? lo + SG_SEG : n;
    if (lo >= n) return;
    const size_t pid = (size_t)py * W + px, hw = (size_t)H * W;
    const uint32_t ncq = inside ? n_contrib[pid] : 0u;
    uint32_t m = ncq;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { uint32_t u = __shfl_xor(m, o, 64); m = u > m ? u : m; }
    const int maxq = (int)__builtin_amdgcn_readfirstlane(m);          // this quadrant's deepest contributor
    if (lane == 0) smax[wave] = m;
    __syncthreads();
    const int max_contrib = (int)max(max(smax[0], smax[1]), max(smax[2], smax[3]));
    if (lo >= max_contrib) return;                                     // nothing of this segment reached a pixel: its records stay zero
    // ---- stage the segment: one entry per thread
    const int cnt = hi - lo;                                           // <= SG_BS
    uint32_t rslot = 0xffffffffu;
    float opac = 0.0f, cA = 0.0f, cB = 0.0f, cC = 0.0f;
    {
        uint32_t mk = 0u, gid = 0u;
        const int e = lo + tid;
        if (tid < cnt && e < max_contrib) {
            gid = point_list[range.x + e];
            mk = pair_mask[range.x + e];
            if (split_long && n > SG_WSORT_MAX)
                mk = (mk & 1u) | (pair_mask[(size_t)mask_plane + range.x + e] & 2u) | (pair_mask[2 * (size_t)mask_plane + range.x + e] & 4u) |
                     (pair_mask[3 * (size_t)mask_plane + range.x + e] & 8u);
            mk &= 15u;
        }
        if (mk) {
            const float4 c4 = recC[SG_REC_STRIDE * (size_t)gid], a = recA[SG_REC_STRIDE * (size_t)gid], b = recB[SG_REC_STRIDE * (size_t)gid];
            const uint32_t goff = __float_as_uint(c4.y), mn = __float_as_uint(c4.z), wh = __float_as_uint(c4.w);
            const int x0 = mn & 0xffff, y0 = mn >> 16, rw = wh & 0xffff;
            rslot = goff + (uint32_t)((ty - y0) * rw + (tx - x0));
            opac = b.y; cA = a.z; cB = a.w; cC = b.x;
            sR[tid][0] = make_float4(a.x, a.y, SG_KA * a.z, SG_KB * a.w);
            sR[tid][1] = make_float4(SG_KA * b.x, b.y, b.z, b.w);
            sR[tid][2].x = c4.x;
            if (AUX) sR[tid][2].y = ax.depth[gid];
        }
        sM[tid] = mk;
    }
    // per-pixel state (requested while the gathers above are in flight)
    const float Tfin = inside ? final_T[pid] : 0.0f;
    const float d0 = inside ? dL_dpix[pid] : 0.0f, d1 = inside ? dL_dpix[hw + pid] : 0.0f, d2 = inside ? dL_dpix[2 * hw + pid] : 0.0f;
    const float dD = AUX && inside && ax.dL_ddepth ? ax.dL_ddepth[pid] : 0.0f, dA = AUX && inside && ax.dL_dalpha ? ax.dL_dalpha[pid] : 0.0f;
    const float tb = AUX ? Tfin * (bg[0] * d0 + bg[1] * d1 + bg[2] * d2 - dA) : Tfin * (bg[0] * d0 + bg[1] * d1 + bg[2] * d2);
    float Tr = Tfin, Sd = 0.0f;
    if (hi < n && ncq > (uint32_t)hi && cks + (uint32_t)(hi / SG_SEG) < ck_cap) {       // (see sg_render_bwd_kernel)
        const float4 cb = ckpt[(size_t)(cks + (uint32_t)(hi / SG_SEG)) * 256 + tid];
        const float4 cf = ckpt[(size_t)cks * 256 + tid];
        const float rT = 1.0f / cb.x;
        Tr = cb.x;
        Sd = fmaf((cf.w - cb.w) * rT, d2, fmaf((cf.z - cb.z) * rT, d1, (cf.y - cb.y) * rT * d0));
        if (AUX) {                                                     // + D_behind dL/ddepth, normalised like the colour
            const float Db = ax.ckD[(size_t)(cks + (uint32_t)(hi / SG_SEG)) * 256 + tid], Df = ax.ckD[(size_t)cks * 256 + tid];
            Sd = fmaf((Df - Db) * rT, dD, Sd);
        }
    }
    const float ddelx_dx = 0.5f * (float)W, ddely_dy = 0.5f * (float)H;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const int cslot = lane == 63 ? 8 : sg_red_idx(lane);
    if (tid < SG_BB) {                                                  // armed once; the combine step re-arms what it consumed (round 5:
#pragma unroll                                                          //  one barrier per sub-batch less)
        for (int w = 0; w < 4; w++) sG[w][tid][8] = __uint_as_float(SG_UNSET);
    }
    __syncthreads();
    // ---- the sub-batches, back to front, out of LDS
    for (int sb = (cnt - 1) / SG_BB; sb >= 0; sb--) {
        const int b0 = sb * SG_BB, base = lo + b0;                      // staged index / list position of the sub-batch's first entry
        const int bc = cnt - b0 < SG_BB ? cnt - b0 : SG_BB;
        if (base < maxq) {
            uint16_t *list = sList[wave];
            const int lim = maxq - base < bc ? maxq - base : bc;          // entries >= maxq touch no pixel here
            const int nl = sg_compact_quadrant<1>(sM + b0, lim, wave, lane, lt, list, SG_BB);
            const uint32_t ncq_b = ncq > (uint32_t)base ? ncq - (uint32_t)base : 0u;   // contributors of this pixel inside the sub-batch
            for (int i = nl - 1; i >= 0; i--) {
                const uint32_t k = list[i];
                const float4 ga = sR[b0 + k][0], gb = sR[b0 + k][1];
                const float gc = sR[b0 + k][2].x;
                const float gz = AUX ? sR[b0 + k][2].y : 0.0f;
                SG_BWD_PASS(k, k);
            }
        }
        __syncthreads();
        // ---- combine the quadrants in a fixed order and store the record (the thread that staged the entry)
        if (tid >= b0 && tid < b0 + bc) {
            const int q0 = tid - b0;
            float s9[9 + AUX] = { };
#pragma unroll
            for (int w = 0; w < 4; w++)
                if (__float_as_uint(sG[w][q0][8]) != SG_UNSET) {
#pragma unroll
                    for (int q = 0; q < 9 + AUX; q++) s9[q] += sG[w][q0][q];
                    sG[w][q0][8] = __uint_as_float(SG_UNSET);
                }
            if (rslot < cap) {
            const float no = -opac, nh = 0.5f * no;
            const float m0 = fmaf(cA, s9[0], cB * s9[1]), m1 = fmaf(cB, s9[0], cC * s9[1]);
            grec_a[2 * (size_t)rslot] = make_float4(no * ddelx_dx * m0, no * ddely_dy * m1, nh * s9[2], nh * s9[3]);
            grec_a[2 * (size_t)rslot + 1] = make_float4(nh * s9[4], s9[5], s9[6], s9[7]);
            grec_b[rslot] = s9[8];
            if (AUX) ax.dz[rslot] = s9[9];                         // (read only where rec_valid is set, like the record)
            rec_valid[rslot] = 1;                                  // (every other record of the frame is never read: sg_sum_records_coop)
            }
        }
        __syncthreads();
    }
}
