// What the two frame encoders share (sg_jpeg.hip, sg_png.hip): the scan that places a frame's segments in its file, and the refusals
// of a call's output capacity and workspace.
#pragma once
#include "sg_host.h"

// A workgroup of 256 threads, all of them here: frame k's segment s (of nseg) starts at header_bytes + the sum over the segments
// before it of (seg_bytes + overhead), overhead being what the file carries around a segment beyond its bytes; that goes to
// seg_off, as 32 bits.  Returns the end of the last segment, carried in 64 bits (a caller's forced worst case may pass 2^31).
// 256 segments per round.  `sm`: 256 words of LDS.
__device__ __forceinline__ unsigned long long sg_codec_segment_offsets(int k, int nseg, uint32_t overhead, int header_bytes,
                                                                       const uint32_t *__restrict__ seg_bytes, uint32_t *__restrict__ seg_off,
                                                                       uint32_t *sm)
{
    const int tid = threadIdx.x;
    // (the total as two words with the carry by hand: a caller that narrows the result then carries the low word alone)
    uint32_t running = (uint32_t)header_bytes, high = 0u;
    for (int s0 = 0; s0 < nseg; s0 += 256) {
        const int s = s0 + tid;
        const uint32_t v = s < nseg ? seg_bytes[(size_t)k * (size_t)nseg + (size_t)s] + overhead : 0u;
        sm[tid] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const uint32_t t = tid >= d ? sm[tid - d] : 0u;
            __syncthreads();
            sm[tid] += t;
            __syncthreads();
        }
        if (s < nseg) seg_off[(size_t)k * (size_t)nseg + (size_t)s] = running + sm[tid] - v;
        running += sm[255];
        high += running < sm[255] ? 1u : 0u;
        __syncthreads();
    }
    return (unsigned long long)high << 32 | running;
}

// The refusals of an encoder's entry point `who` behind its plan: the capacity of an output row, the workspace against what
// `layout` (the name of the layout function) asks for, and its alignment.
static inline int sg_codec_check_buffers(const char *who, const char *layout, size_t capacity, const void *ws, size_t ws_bytes, size_t needed)
{
    if (capacity < 1 || capacity >= ((size_t)1 << 31)) return sg_failf("%s: capacity = %llu bytes per frame", who, (unsigned long long)capacity);
    if (ws_bytes < needed)
        return sg_failf("%s: a workspace of %llu bytes, %s asks for %llu", who, (unsigned long long)ws_bytes, layout, (unsigned long long)needed);
    if ((uintptr_t)ws & 15) return sg_failf("%s: the workspace must be 16-byte aligned", who);
    return 0;
}
