// Dense forward composite of sg_render.hip (frames of many tiles): ONE WAVE per tile, four consecutive tiles per 256-thread
// workgroup, the forward counterpart of sg_render_bwd_kernel.  Lane l owns pixel (l & 7, l >> 3) of EACH of the tile's four 8x8
// quadrants and keeps that pixel's state four times, statically indexed.  The wave sorts its tile's keys itself, stages 64 entries
// per batch (one per lane: the three record gathers, the quadrant mask against the four live boxes), and walks the entries that
// reach some quadrant front to back through a ballot: the record is read ONCE per entry (three LDS reads), its mask goes to
// the scalar unit and the quadrants of the mask are evaluated under wave-uniform branches.  With a wave per quadrant (the cooperative
// body, still the few-tile kernels') an entry that reached q quadrants was read q times out of q compacted lists, and every batch
// paid three workgroup barriers at which a wave waited for the three others of its tile.  The waves of a workgroup share nothing on
// this path: no __syncthreads, no cross-wave LDS traffic.
// What a pixel sees is what it saw: the same entries in the same order through the same expression (SG_FWD_TW_QUAD is SG_FWD_PASS),
// the live boxes refreshed, the "all pixels done" exit taken and the checkpoints written at multiples of SG_FB = 256 entries, so the
// images, masks, checkpoints and contributor counts are the cooperative body's, bit for bit.

#define SG_TW_BATCH 64          // entries staged per batch: one per lane
#define SG_TWSORT_MAX 512       // longest list one wave sorts: its 64 staging rows of 64 B hold 512 keys
static_assert(SG_TWSORT_MAX * 8 == SG_TW_BATCH * 64 && SG_RANKSORT_MAX * 2 * 8 <= SG_TW_BATCH * 64, "sort buffers alias the wave's rows");
static_assert(SG_FB % SG_TW_BATCH == 0, "boxes and checkpoints are refreshed between batches");

// One (entry, quadrant) pass: SG_FWD_PASS on the state of quadrant Q -- straight-line, predicated.  The quadrant's `done` flags are a
// wave-wide mask in scalar registers (dn4[Q]): the validity logic is scalar arithmetic on the compares' lane masks and costs no vector
// instruction or register.  (As four per-lane bools hipcc kept a byte register each and paid a compare, a select and an OR per pass.)
#define SG_FWD_TW_QUAD(Q)                                                                                  \
    do {                                                                                                   \
        const float dx = ga.x - (((Q) & 1) ? pxf1 : pxf0), dy = ga.y - (((Q) >> 1) ? pyf1 : pyf0);         \
        const float power = sg_power2(ga.z, ga.w, gb.x, dx, dy);                                           \
        const float alpha = fminf(0.99f, gb.y * __builtin_amdgcn_exp2f(power));                            \
        const float test_T = Tr4[Q] * (1.0f - alpha);                                                      \
        const unsigned long long valid = __ballot(!(power > 0.0f)) & __ballot(!(alpha < 1.0f / 255.0f)) & ~dn4[Q]; \
        const unsigned long long term = valid & __ballot(test_T < 0.0001f);                                \
        const bool blend = __builtin_amdgcn_inverse_ballot_w64(valid & ~term);                             \
        const float w = blend ? alpha * Tr4[Q] : 0.0f;                                                     \
        C04[Q] = fmaf(gb.z, w, C04[Q]); C14[Q] = fmaf(gb.w, w, C14[Q]); C24[Q] = fmaf(gm.x, w, C24[Q]);    \
        if (AUX) Dz4[Q] = fmaf(gm.y, w, Dz4[Q]);                                                           \
        Tr4[Q] = blend ? test_T : Tr4[Q];                                                                  \
        last4[Q] = blend ? pos1 : last4[Q];                                                                \
        dn4[Q] |= term;                                                                                    \
    } while (0)

// A wave-uniform float in a scalar register.  (gfx950 converts integers to floats on the vector unit only, and hipcc leaves the result
// there: the sixteen box coordinates and the tile origin then occupied eighteen vector registers through the walk.)
__device__ __forceinline__ float sg_uniform(float x) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(x))); }

// An id of a sorted list, past the CU's vector cache.  Lists sorted in this kernel are written by one wave, or by the workgroup, and read
// back here; a neighbouring tile's read-back on the same CU may have cached the 128-byte line that holds the head of this list before
// it was written (a list's tail and the next list's head share a line).
__device__ __forceinline__ uint32_t sg_list_id(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <bool AUX>
__device__ __forceinline__ void sg_render_fwd_tile_wave(SG_FWD_PARAMS, SgAuxFwd ax = SgAuxFwd{})
{
    // per wave: its staged batch, a 64-byte row per entry -- (mean x, mean y, A', B') (C', opacity, colour 0, 1) (colour 2, z [AUX],
    // quadrant mask, -) -- and, before the first batch, the tile's sort keys
    __shared__ float4 sR[4][SG_TW_BATCH][4];
    (void)nblocks; (void)long_items; (void)mask_plane; (void)plan; (void)item_w; (void)w_plane;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // (see sg_render_fwd_body: the next forward's counters are consumed by now)
    if (tid == 0 && blockIdx.x == 0) header[2] = 0u;
    const int tile0 = 4 * sg_tile_of_block((int)blockIdx.x);
    if (tile0 >= T) return;
    const bool overflow = header[1] != 0u;              // part of the sorted list was never written: render the background
    // Lists of SG_TWSORT_MAX + 1 .. SG_WSORT_MAX entries are longer than a wave's rows: the workgroup sorts them together first, in
    // the four waves' rows, and every wave then walks its own tile like a list that arrived sorted.  Every wave reads the four
    // ranges, so the decision is workgroup-uniform without a barrier.  (cfg3's longest list has 135 entries.)
    {
        bool coop = false;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const uint2 r = ranges[tile0 + w < T ? tile0 + w : T - 1];
            const int nw = overflow ? 0 : (int)(r.y - r.x);
            coop |= nw > SG_TWSORT_MAX && nw <= SG_WSORT_MAX;
        }
        if (coop) {
            static_assert((SG_WSORT_MAX + SG_RANKSORT_MAX) * 8 <= 4 * SG_TW_BATCH * 64, "the workgroup's sort buffers alias the four waves' rows");
            uint64_t *sKey = (uint64_t *)sR;
            for (int w = 0; w < 4; w++) {
                if (tile0 + w >= T) break;
                const uint2 r = ranges[tile0 + w];
                const int nw = (int)(r.y - r.x);
                if (!(nw > SG_TWSORT_MAX && nw <= SG_WSORT_MAX)) continue;
                sg_sort_short_list(key_pitch ? pair_keys + (size_t)(tile0 + w) * key_pitch : pair_keys + r.x, nw, sKey, sKey + SG_WSORT_MAX, tid);
                for (int i = tid; i < nw; i += 256) {
                    const uint64_t key = sKey[i];
                    point_list[r.x + i] = (uint32_t)key;
                    if (point_keys) point_keys[r.x + i] = ((uint64_t)(tile0 + w) << 32) | (key >> 32);
                }
                __syncthreads();                                 // the keys are consumed: the next tile's sort, the waves' rows
            }
            __threadfence_block();                               // the waves read these ids back from point_list
        }
    }
    const int tile = tile0 + wave;
    if (tile >= T) return;
    if (lane == 0) tile_count[sg_ctr_of_tile((uint32_t)tile, (uint32_t)gx)] = 0u;
    const int X0 = (tile % gx) * 16, Y0 = (tile / gx) * 16;
    const uint2 range = ranges[tile];
    const int n = overflow ? 0 : (int)(range.y - range.x);
    const uint32_t cks = n > SG_SEG ? ck_start[tile] : 0xffffffffu;   // segmented list: checkpoint slots cks + segment
    // quadrant 0's pixel of this lane; the others' are + 8, exactly
    const int px0 = X0 + (lane & 7), py0 = Y0 + (lane >> 3);
    const float pxf0 = (float)px0, pyf0 = (float)py0, pxf1 = pxf0 + 8.0f, pyf1 = pyf0 + 8.0f;
    float Tr4[4], C04[4], C14[4], C24[4], Dz4[4];
    uint32_t last4[4];
    unsigned long long dn4[4];                               // the quadrants' finished pixels: terminated, or outside the image
#pragma unroll
    for (int q = 0; q < 4; q++) {
        Tr4[q] = 1.0f; C04[q] = 0.0f; C14[q] = 0.0f; C24[q] = 0.0f; Dz4[q] = 0.0f; last4[q] = 0u;
        dn4[q] = __ballot(!(px0 + 8 * (q & 1) < W && py0 + 8 * (q >> 1) < H));
    }
    float4 (*row)[4] = sR[wave];
    // software pipeline over batches: the gathers of batch k + 1 are in flight while batch k is walked
    float4 pa = make_float4(0, 0, 0, 0), pb = pa;
    float pc = 0.0f, pz = 0.0f;
    if (n > 0 && n <= SG_TWSORT_MAX) {
        // the wave sorts the tile's keys itself, in its rows, and hands the order to the backward pass through point_list
        // (direct binning, key_pitch != 0: `pair_keys` is SgBin::tile_keys, the tile's unsorted keys are its row)
        uint64_t *sKey = (uint64_t *)row;
        sg_sort_short_list_wave(key_pitch ? pair_keys + (size_t)tile * key_pitch : pair_keys + range.x, n, sKey, lane);
        for (int i = lane; i < n; i += SG_TW_BATCH) {
            const uint64_t key = sKey[i];
            const uint32_t gid = (uint32_t)key;
            point_list[range.x + i] = gid;
            if (point_keys) point_keys[range.x + i] = ((uint64_t)tile << 32) | (key >> 32);
            if (i == lane) {
                pa = recA[SG_REC_STRIDE * (size_t)gid]; pb = recB[SG_REC_STRIDE * (size_t)gid]; pc = recC[SG_REC_STRIDE * (size_t)gid].x;
                if (AUX) pz = ax.depth[gid];
            }
        }
        if (n > SG_TW_BATCH) __threadfence_block();          // later batches read their ids back from point_list
    } else if (lane < n) {                                   // sorted by the workgroup above, or by sg_tile_sort_kernel / sg_tile_rank_kernel
        const uint32_t gid = sg_list_id(point_list + range.x + lane);
        pa = recA[SG_REC_STRIDE * (size_t)gid]; pb = recB[SG_REC_STRIDE * (size_t)gid]; pc = recC[SG_REC_STRIDE * (size_t)gid].x;
        if (AUX) pz = ax.depth[gid];
    }
    float4 box[4];                                           // the quadrants' live boxes (wave-uniform)
    const float X0f = sg_uniform((float)X0), Y0f = sg_uniform((float)Y0);
    for (int base = 0; base < n; base += SG_TW_BATCH) {
        if ((base & (SG_FB - 1)) == 0) {
            // every SG_FB entries, as the cooperative body does per batch of its own: the boxes of the pixels still being composited,
            // the exit once no pixel is, and the state in front of entry `base` for the backward pass of the segments behind it
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float4 b = sg_live_box(~dn4[q], q);
                box[q] = make_float4(sg_uniform(b.x), sg_uniform(b.y), sg_uniform(b.z), sg_uniform(b.w));
            }
            if ((dn4[0] & dn4[1] & dn4[2] & dn4[3]) == ~0ull) break;
            if (base > 0 && cks != 0xffffffffu && cks + (uint32_t)(base / SG_SEG) < ck_cap) {
                // (the lane taken afresh: from `lane` hipcc forms this address in front of the loop and keeps it in two vector registers,
                //  through the walk, for a store that lists of up to SG_SEG entries never reach)
                int ln = lane;
                asm volatile("" : "+v"(ln));
                const size_t slot = (size_t)(cks + (uint32_t)(base / SG_SEG)) * 256 + (uint32_t)ln;
#pragma unroll
                for (int q = 0; q < 4; q++)
                    if (dn4[q] != ~0ull) {                    // (a finished quadrant leaves its slot alone)
                        ckpt[slot + q * 64] = make_float4(Tr4[q], C04[q], C14[q], C24[q]);
                        if (AUX) ax.ckD[slot + q * 64] = Dz4[q];
                    }
            }
        }
        const int e = base + lane;
        uint32_t mk = 0u;
        if (e < n) {
            mk = sg_quad_mask(pa, pb, X0f, Y0f, box);
            row[lane][0] = make_float4(pa.x, pa.y, SG_KA * pa.z, SG_KB * pa.w);
            row[lane][1] = make_float4(SG_KA * pb.x, pb.y, pb.z, pb.w);
            row[lane][2] = make_float4(pc, pz, __uint_as_float(mk), 0.0f);
            pair_mask[range.x + e] = (uint8_t)mk;            // the backward composites exactly these (entry, quadrant) pairs
        }
        if (e + SG_TW_BATCH < n) {
            const uint32_t gid = sg_list_id(point_list + range.x + e + SG_TW_BATCH);
            pa = recA[SG_REC_STRIDE * (size_t)gid]; pb = recB[SG_REC_STRIDE * (size_t)gid]; pc = recC[SG_REC_STRIDE * (size_t)gid].x;
            if (AUX) pz = ax.depth[gid];
        }
        unsigned long long todo = __ballot(mk != 0u);        // entries still to walk, front to back
        __builtin_amdgcn_wave_barrier();
        while (todo) {
            const int k = __builtin_ctzll(todo);
            todo &= todo - 1ull;
            const float4 ga = row[k][0], gb = row[k][1], gm = row[k][2];
            const uint32_t mke = __builtin_amdgcn_readfirstlane(__float_as_uint(gm.z));
            uint32_t pos1;                                   // n_contrib of a pixel whose last contributor this entry is
            asm volatile("v_mov_b32 %0, %1" : "=v"(pos1) : "s"(base + k + 1));   // (one copy per entry: a select takes no second scalar operand)
            if (mke & 1u) SG_FWD_TW_QUAD(0);
            if (mke & 2u) SG_FWD_TW_QUAD(1);
            if (mke & 4u) SG_FWD_TW_QUAD(2);
            if (mke & 8u) SG_FWD_TW_QUAD(3);
        }
        __builtin_amdgcn_wave_barrier();
    }
    const size_t hw = (size_t)H * W;
    const float bg0 = bg[0], bg1 = bg[1], bg2 = bg[2];
    int ln = lane;                                           // (afresh, as above: the pixel's integer coordinates are not carried through the walk)
    asm volatile("" : "+v"(ln));
#pragma unroll
    for (int q = 0; q < 4; q++) {
        if (cks < ck_cap) {
            ckpt[(size_t)cks * 256 + q * 64 + ln] = make_float4(Tr4[q], C04[q], C14[q], C24[q]);   // slot 0: final state
            if (AUX) ax.ckD[(size_t)cks * 256 + q * 64 + ln] = Dz4[q];
        }
        const int px = X0 + (ln & 7) + 8 * (q & 1), py = Y0 + (ln >> 3) + 8 * (q >> 1);
        if (px < W && py < H) {
            const size_t pid = (size_t)py * W + px;
            final_T[pid] = Tr4[q];
            n_contrib[pid] = last4[q];
            out_color[pid] = fmaf(Tr4[q], bg0, C04[q]);
            out_color[hw + pid] = fmaf(Tr4[q], bg1, C14[q]);
            out_color[2 * hw + pid] = fmaf(Tr4[q], bg2, C24[q]);
            if (AUX) { ax.out_depth[pid] = Dz4[q]; ax.out_alpha[pid] = 1.0f - Tr4[q]; }
        }
    }
}

#undef SG_FWD_TW_QUAD
