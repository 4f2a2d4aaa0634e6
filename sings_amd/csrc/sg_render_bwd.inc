// Backward composite kernels of sg_render.hip, included there twice: SG_BWD_AUX 0 defines sg_render_bwd_kernel and
// sg_render_bwd_sparse_kernel, SG_BWD_AUX 1 sg_render_bwd_aux_kernel and sg_render_bwd_sparse_aux_kernel, which also take the
// depth / alpha adjoints (`ax`: SG_BWD_PASS) and write the dL/dz plane, frame blockIdx.y's (SG_BWD_AUX_FRAME_OFFSETS).  In the plain
// kernels every AUX branch is dead.
// (no include guard: included once per variant)

// Quadrant Q of the current entry in the dense kernels: SG_BWD_EVAL on the quadrant's pixel state, then the per-lane partials go into the
// entry's accumulators.  The entry's first accumulating quadrant ASSIGNS them -- nine instructions (SG_BWD_FIRST): the two first moments,
// the three second moments from them, a move of `w`, the three colour products; what the registers held, the previous entry's
// sums, is never read -- and every later one ADDS -- eleven (SG_BWD_LATER): `wx`, `wy`, an add for each of them and for `w`, one
// v_fmac per second moment and colour (ONE rounding of acc + a b; the three adds round the sum of a rounded product, as ever).
// Quadrant 0, when it accumulates, is always the first: the assigning form, statically.  Quadrants 1-3 hold BOTH forms in one asm
// statement behind a scalar branch on `some` (wave-uniform, a scalar register): in C++ every form of that choice costs copies or
// selects -- as `first ? v : acc + v` a select per value, as a branch 18 register copies where its sides meet -- and inside the
// statement the compiler sees one instruction that updates the accumulators in place.  Every instruction in the strings is a plain
// VALU operation on interlocked registers and their first reads `w` (a v_cndmask result) and `dchan` (a v_mul result): no wait state.
#define SG_BWD_FIRST(A0, A1, A2, A3, A4, A5, A6, A7, A8, Wv, DX, DY, DC, C0, C1, C2)                                   \
    "v_mul_f32 " A0 ", " Wv ", " DX "\n\tv_mul_f32 " A1 ", " Wv ", " DY "\n\t"                                          \
    "v_mul_f32 " A2 ", " A0 ", " DX "\n\tv_mul_f32 " A3 ", " A0 ", " DY "\n\tv_mul_f32 " A4 ", " A1 ", " DY "\n\t"       \
    "v_mov_b32 " A5 ", " Wv "\n\t"                                                                                    \
    "v_mul_f32 " A6 ", " DC ", " C0 "\n\tv_mul_f32 " A7 ", " DC ", " C1 "\n\tv_mul_f32 " A8 ", " DC ", " C2 "\n\t"
#define SG_BWD_LATER(A0, A1, A2, A3, A4, A5, A6, A7, A8, T0, T1, Wv, DX, DY, DC, C0, C1, C2)                           \
    "v_mul_f32 " T0 ", " Wv ", " DX "\n\tv_mul_f32 " T1 ", " Wv ", " DY "\n\t"                                          \
    "v_add_f32 " A0 ", " A0 ", " T0 "\n\tv_add_f32 " A1 ", " A1 ", " T1 "\n\t"                                          \
    "v_fmac_f32 " A2 ", " T0 ", " DX "\n\tv_fmac_f32 " A3 ", " T0 ", " DY "\n\tv_fmac_f32 " A4 ", " T1 ", " DY "\n\t"    \
    "v_add_f32 " A5 ", " A5 ", " Wv "\n\t"                                                                            \
    "v_fmac_f32 " A6 ", " DC ", " C0 "\n\tv_fmac_f32 " A7 ", " DC ", " C1 "\n\tv_fmac_f32 " A8 ", " DC ", " C2 "\n\t"
#define SG_BWD_ACC9 "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]), "+v"(acc[6]), "+v"(acc[7]), "+v"(acc[8])
// quadrant 0.  Operands: %0-%8 acc (AUX: %9 acc[9]), then w, dx, dy, dchan, d0, d1, d2 (AUX: dD)
#define SG_BWD_ASSIGN()                                                                                               \
    do {                                                                                                              \
        if (AUX)                                                                                                      \
            asm volatile(SG_BWD_FIRST("%0", "%1", "%2", "%3", "%4", "%5", "%6", "%7", "%8", "%10", "%11", "%12", "%13", "%14", "%15", "%16") \
                         "v_mul_f32 %9, %13, %17"                                                                     \
                         : SG_BWD_ACC9, "+v"(acc[9]) : "v"(w), "v"(dx), "v"(dy), "v"(dchan), "v"(d0), "v"(d1), "v"(d2), "v"(dD)); \
        else                                                                                                          \
            asm volatile(SG_BWD_FIRST("%0", "%1", "%2", "%3", "%4", "%5", "%6", "%7", "%8", "%9", "%10", "%11", "%12", "%13", "%14", "%15") \
                         : SG_BWD_ACC9 : "v"(w), "v"(dx), "v"(dy), "v"(dchan), "v"(d0), "v"(d1), "v"(d2));             \
    } while (0)
// quadrants 1-3.  Operands: %0-%8 acc, two temporaries, w, dx, dy, dchan, d0, d1, d2, `some` (AUX: acc[9] behind acc[8], dD behind d2)
#define SG_BWD_ASSIGN_OR_ADD()                                                                                        \
    do {                                                                                                              \
        float t0, t1;                                                                                                 \
        if (AUX)                                                                                                      \
            asm volatile("s_cmp_lg_u32 %20, 0\n\ts_cbranch_scc0 1f\n\t"                                              \
                         SG_BWD_LATER("%0", "%1", "%2", "%3", "%4", "%5", "%6", "%7", "%8", "%10", "%11", "%12", "%13", "%14", "%15", "%16", "%17", "%18") \
                         "v_fmac_f32 %9, %15, %19\n\ts_branch 2f\n1:\n\t"                                            \
                         SG_BWD_FIRST("%0", "%1", "%2", "%3", "%4", "%5", "%6", "%7", "%8", "%12", "%13", "%14", "%15", "%16", "%17", "%18") \
                         "v_mul_f32 %9, %15, %19\n2:"                                                                  \
                         : SG_BWD_ACC9, "+v"(acc[9]), "=&v"(t0), "=&v"(t1)                                             \
                         : "v"(w), "v"(dx), "v"(dy), "v"(dchan), "v"(d0), "v"(d1), "v"(d2), "v"(dD), "s"(some) : "scc"); \
        else                                                                                                          \
            asm volatile("s_cmp_lg_u32 %18, 0\n\ts_cbranch_scc0 1f\n\t"                                              \
                         SG_BWD_LATER("%0", "%1", "%2", "%3", "%4", "%5", "%6", "%7", "%8", "%9", "%10", "%11", "%12", "%13", "%14", "%15", "%16", "%17") \
                         "s_branch 2f\n1:\n\t"                                                                        \
                         SG_BWD_FIRST("%0", "%1", "%2", "%3", "%4", "%5", "%6", "%7", "%8", "%11", "%12", "%13", "%14", "%15", "%16", "%17") \
                         "\n2:"                                                                                       \
                         : SG_BWD_ACC9, "=&v"(t0), "=&v"(t1)                                                          \
                         : "v"(w), "v"(dx), "v"(dy), "v"(dchan), "v"(d0), "v"(d1), "v"(d2), "s"(some) : "scc");        \
    } while (0)
#define SG_BWD_QUAD(Q)                                                                                                \
    do {                                                                                                              \
        const float pxf = ((Q) & 1) ? pxf0 + 8.0f : pxf0, pyf = ((Q) >> 1) ? pyf0 + 8.0f : pyf0;                      \
        const float d0 = d04[Q], d1 = d14[Q], d2 = d24[Q], dD = dD4[Q], tb = tb4[Q];                                  \
        const uint32_t ncq_b = ncq4[Q];                                                                               \
        float &Tr = Tr4[Q], &Sd = Sd4[Q];                                                                             \
        SG_BWD_EVAL((uint32_t)pos, break);          /* (no pixel valid: `some` stays what it was) */                  \
        if ((Q) == 0) SG_BWD_ASSIGN(); else SG_BWD_ASSIGN_OR_ADD();                                                   \
        some = 1u;                                                                                                    \
    } while (0)
// Dense backward (frames of many tiles): ONE WAVE per work item (tile, depth segment), four consecutive items per workgroup.  Lane l
// owns pixel (l & 7, l >> 3) of EACH of the tile's four 8x8 quadrants and keeps that pixel's state four times, statically indexed.
// An entry is evaluated in the quadrants the forward composited it in (its mask bits: wave-uniform branches, the quadrant loop fully
// unrolled), its per-lane partials are added over those quadrants in registers -- the first assigns (SG_BWD_QUAD), the others add, in
// the order 0, 1, 2, 3 -- and ONE lane butterfly per (tile, entry) sums them; with a wave per quadrant an entry that reached q quadrants paid q
// butterflies and an LDS combine behind two workgroup barriers.  The waves of a workgroup share nothing: no __syncthreads at all.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SG_BWD_TW_WAVES, SG_BWD_TW_WAVES)))
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
    // per wave: its staged batch -- (mean x, mean y, A', B') (C', opacity, colour 0, 1) (colour 2, z [AUX], -, opacity) and, for the
    // record store, (A, B, C, record slot): kept here, not in registers, across the walk.  Row as 16 floats: 0-3 `ga`, 4-7 `gb`, 8 `gc`,
    // 9 `gz`, 10 unused (the batch's quadrant masks are lane masks in scalar registers), 11 the opacity once more, 12-15 (A, B, C, slot).  An entry's nine (AUX: ten) sums are filed over floats 0-8
    // (9) of its OWN row (SG_BWD_FILE through `sG`): the walk has read them by then and every other entry reads only its own row.
    // Floats 10-15 are never overwritten; the record store takes the opacity from float 11.  A row nobody filed still holds staged
    // floats (or an earlier batch's): `filed` keeps the store from reading it.
    __shared__ float4 sR[4][SG_BB][4];
    float (*sG)[SG_BB][16] = (float (*)[SG_BB][16])sR;
    SG_STAMP_SCOPE
    SG_BWD_FRAME_OFFSETS;
#if SG_BWD_AUX
    SG_BWD_AUX_FRAME_OFFSETS;
#endif
    // the item list is in tile order, so the XCD-aware map over groups of four items keeps neighbouring tiles on one L2.  The grid is
    // an upper bound; the last workgroup's waves past the item count have nothing to do.
    (void)T; (void)nblocks;
    const int nitems = header[1] ? 0 : (int)header[5];             // nothing to do after a capacity overflow
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int it = 4 * sg_tile_of_block(blockIdx.x) + wave;
    if (it >= nitems) return;
    const uint32_t item = items[it];
    const int tile = (int)(item & 0xfffffu), seg = (int)(item >> 20);
    const int tx = tile % gx, ty = tile / gx;
    const int X0 = tx * 16, Y0 = ty * 16;
    const uint2 range = ranges[tile];
    const int n = (int)(range.y - range.x);
    const uint32_t cks = ck_start[tile];
    const int lo = seg * SG_SEG;                                   // this item: entries [lo, hi)
    const int hi = cks != 0xffffffffu && lo + SG_SEG < n ? lo + SG_SEG : n;
    if (lo >= n) return;
    const size_t hw = (size_t)H * W;
    // per-pixel state, once per quadrant: running T, <colour accumulated BEHIND the current entry, dL/dpixel> (ONE running scalar
    // instead of three channels), dL/dpixel, T_final <bg, dL/dpixel>, the contributor count
    const float pxf0 = (float)(X0 + (lane & 7)), pyf0 = (float)(Y0 + (lane >> 3));     // quadrant 0's pixel; the others' are + 8, exactly
    float Tr4[4], Sd4[4], d04[4], d14[4], d24[4], dD4[4], tb4[4];
    uint32_t ncq4[4];
    int maxq4[4];                                                  // the quadrants' deepest contributors (wave-uniform)
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int px = X0 + 8 * (q & 1) + (lane & 7), py = Y0 + 8 * (q >> 1) + (lane >> 3);
        const bool inside = px < W && py < H;
        const size_t pid = (size_t)py * W + px;
        const float Tfin = inside ? final_T[pid] : 0.0f;
        const uint32_t ncq = inside ? n_contrib[pid] : 0u;
        const float d0 = inside ? dL_dpix[pid] : 0.0f, d1 = inside ? dL_dpix[hw + pid] : 0.0f, d2 = inside ? dL_dpix[2 * hw + pid] : 0.0f;
        const float dD = AUX && inside && ax.dL_ddepth ? ax.dL_ddepth[pid] : 0.0f, dA = AUX && inside && ax.dL_dalpha ? ax.dL_dalpha[pid] : 0.0f;
        tb4[q] = AUX ? Tfin * (bg[0] * d0 + bg[1] * d1 + bg[2] * d2 - dA) : Tfin * (bg[0] * d0 + bg[1] * d1 + bg[2] * d2);
        float Tr = Tfin, Sd = 0.0f;
        // Not the last segment, and this pixel has contributors behind it: start from the forward checkpoint at `hi`.
        // T in front of entry hi; S = colour composited behind it, normalised by that T.  (A pixel with ncq <= hi has
        // nothing behind: final state.  ncq > hi implies the forward reached that boundary with this pixel live.)
        if (hi < n && ncq > (uint32_t)hi && cks + (uint32_t)(hi / SG_SEG) < ck_cap) {
            const float4 cb = ckpt[(size_t)(cks + (uint32_t)(hi / SG_SEG)) * 256 + q * 64 + lane];
            const float4 cf = ckpt[(size_t)cks * 256 + q * 64 + lane];
            const float rT = 1.0f / cb.x;
            Tr = cb.x;
            Sd = fmaf((cf.w - cb.w) * rT, d2, fmaf((cf.z - cb.z) * rT, d1, (cf.y - cb.y) * rT * d0));
            if (AUX) {                                                     // + D_behind dL/ddepth, normalised like the colour
                const float Db = ax.ckD[(size_t)(cks + (uint32_t)(hi / SG_SEG)) * 256 + q * 64 + lane], Df = ax.ckD[(size_t)cks * 256 + q * 64 + lane];
                Sd = fmaf((Df - Db) * rT, dD, Sd);
            }
        }
        Tr4[q] = Tr; Sd4[q] = Sd; d04[q] = d0; d14[q] = d1; d24[q] = d2; dD4[q] = dD; ncq4[q] = ncq;
        uint32_t m = ncq;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { uint32_t u = __shfl_xor(m, o, 64); m = u > m ? u : m; }
        maxq4[q] = (int)__builtin_amdgcn_readfirstlane(m);
    }
    const int max_contrib = max(max(maxq4[0], maxq4[1]), max(maxq4[2], maxq4[3]));
    // Wave-uniform and read only at the record store: scalar registers, not two vector registers held across the walk.  (As an asm
    // statement: hipcc folds the builtin away on a value it knows to be uniform and keeps the v_cvt's result where it is.  The
    // s_nop is the wait state between a VALU write of a vector register and a lane read of it.)
    float ddelx_dx, ddely_dy;
    asm volatile("s_nop 0\n\tv_readfirstlane_b32 %0, %2\n\tv_readfirstlane_b32 %1, %3"
                 : "=&s"(ddelx_dx), "=s"(ddely_dy) : "v"(0.5f * (float)W), "v"(0.5f * (float)H));
    const int cslot = lane == 63 ? 8 : sg_red_idx(lane);
    float acc[10] = { };                                           // the current entry's partials, summed over its quadrants ([9]: AUX, dL/dz)
    // ---- the segment in batches of 64 entries, one entry per lane, back to front
    for (int base = lo + (hi - 1 - lo) / SG_BB * SG_BB; base >= lo; base -= SG_BB) {
        const int cnt = hi - base < SG_BB ? hi - base : SG_BB;
        // ---- stage the batch: list id -> record C -> record slot; the quadrant mask; records A and B of entries composited somewhere
        uint32_t mk = 0u;
        if (lane < cnt) {
            const int e = base + lane;
            const uint32_t gid = point_list[range.x + e];
            // quadrants the forward composited this entry in: nothing else can carry a gradient, so neither the
            // rectangle tests nor the two record gathers are repeated for the rest
            if (e < max_contrib) {
                mk = pair_mask[range.x + e];
                if (split_long && n > SG_WSORT_MAX)
                    mk = (mk & 1u) | (pair_mask[(size_t)mask_plane + range.x + e] & 2u) | (pair_mask[2 * (size_t)mask_plane + range.x + e] & 4u) |
                         (pair_mask[3 * (size_t)mask_plane + range.x + e] & 8u);
                mk &= 15u;
            }
            const float4 c4 = recC[SG_REC_STRIDE * (size_t)gid];
            if (mk) {
                const float4 a = recA[SG_REC_STRIDE * (size_t)gid], b = recB[SG_REC_STRIDE * (size_t)gid];
                sR[wave][lane][0] = make_float4(a.x, a.y, SG_KA * a.z, SG_KB * a.w);
                sR[wave][lane][1] = make_float4(SG_KA * b.x, b.y, b.z, b.w);
                sR[wave][lane][2] = make_float4(c4.x, AUX ? ax.depth[gid] : 0.0f, 0.0f, b.y);
                sR[wave][lane][3] = make_float4(a.z, a.w, b.x, 0.0f);
            }
            const uint32_t goff = __float_as_uint(c4.y), mn = __float_as_uint(c4.z), wh = __float_as_uint(c4.w);
            const int x0 = mn & 0xffff, y0 = mn >> 16, rw = wh & 0xffff;
            sR[wave][lane][3].w = __uint_as_float(goff + (uint32_t)((ty - y0) * rw + (tx - x0)));
        }
        // the batch's masks, one lane mask per quadrant in scalar registers: bit k of mq[q] = the forward composited entry base + k in
        // quadrant q and the entry is not behind the quadrant's deepest contributor (base + k < maxq4[q]: the lanes below maxq4[q] - base,
        // formed on the scalar unit).  The walk tests them on the scalar unit.
        const unsigned long long mq0 = __ballot(mk & 1u) & sg_lanes_below(maxq4[0] - base), mq1 = __ballot(mk & 2u) & sg_lanes_below(maxq4[1] - base),
                                 mq2 = __ballot(mk & 4u) & sg_lanes_below(maxq4[2] - base), mq3 = __ballot(mk & 8u) & sg_lanes_below(maxq4[3] - base);
        unsigned long long todo = mq0 | mq1 | mq2 | mq3;               // entries still to walk
        unsigned long long filed = 0ull;                               // entries whose row of sums was written
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();
        while (todo) {
            const int k = 63 - __builtin_clzll(todo);
            todo &= ~(1ull << k);
            const int pos = base + k;                                   // the entry's position in the tile's list
            const float4 ga = sR[wave][k][0], gb = sR[wave][k][1];
            const float gc = sR[wave][k][2].x, gz = AUX ? sR[wave][k][2].y : 0.0f;
            // the entry's partials, added over its quadrants in the order 0, 1, 2, 3
            uint32_t some = 0u;                                         // some pixel of the tile took a gradient from this entry (a scalar register)
            if ((mq0 >> k) & 1ull) SG_BWD_QUAD(0);
            if ((mq1 >> k) & 1ull) SG_BWD_QUAD(1);
            if ((mq2 >> k) & 1ull) SG_BWD_QUAD(2);
            if ((mq3 >> k) & 1ull) SG_BWD_QUAD(3);
            __builtin_amdgcn_wave_barrier();                           // (no instruction: keeps the paths above from being threaded into the tail, with copies)
            if (some) {                                                // (else no pixel of the tile: the row reads as zero)
                SG_BWD_FILE(acc, acc[9], k);
                filed |= 1ull << k;
            }
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();
        // ---- store the record (the lane that staged the entry): every entry of the segment gets one, zero where nothing was filed
        const float4 cn = sR[wave][lane][3];
        const uint32_t rslot = lane < cnt ? __float_as_uint(cn.w) : 0xffffffffu;
        if (rslot < cap) {
            float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0;
            float r2 = 0.0f, r3 = 0.0f;
            if ((filed >> lane) & 1ull) {                         // (an entry nobody filed has no staged record either)
                const float4 s03 = sR[wave][lane][0], s47 = sR[wave][lane][1], s8o = sR[wave][lane][2];    // the sums, (8, 9 [AUX], -, opacity)
                const float s[10] = { s03.x, s03.y, s03.z, s03.w, s47.x, s47.y, s47.z, s47.w, s8o.x, s8o.y };
                const float no = -s8o.w, nh = 0.5f * no;                            // -opacity, -opacity / 2
                const float m0 = fmaf(cn.x, s[0], cn.y * s[1]), m1 = fmaf(cn.y, s[0], cn.z * s[1]);   // conic . first moments
                r0 = make_float4(no * ddelx_dx * m0, no * ddely_dy * m1, nh * s[2], nh * s[3]);
                r1 = make_float4(nh * s[4], s[5], s[6], s[7]);
                r2 = s[8];
                if (AUX) r3 = s[9];
            }
            grec_a[2 * (size_t)rslot] = r0;
            grec_a[2 * (size_t)rslot + 1] = r1;
            grec_b[rslot] = r2;
            if (AUX) ax.dz[rslot] = r3;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

#undef SG_BWD_QUAD
#undef SG_BWD_ASSIGN_OR_ADD
#undef SG_BWD_ASSIGN
#undef SG_BWD_ACC9
#undef SG_BWD_LATER
#undef SG_BWD_FIRST

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
