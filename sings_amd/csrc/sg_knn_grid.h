// Sizing of the k-NN search grids: bounding box + cell budget -> cell edge and dims.  Plain C / C++, shared by the device
// (thread 0 of sg_grid_setup2_kernel, sg_knn.hip) and by the host tests (oracle/knn_grid_host.c), so that what is tested on the CPU is
// the arithmetic the kernel runs.
#ifndef SG_KNN_GRID_H
#define SG_KNN_GRID_H
#include <math.h>
#if defined(__HIPCC__)
#define SG_KNN_HD __host__ __device__
#else
#define SG_KNN_HD
#endif

typedef struct SgGrid {
    float lo[3], inv_h, h;
    int dim[3], ncells;
} SgGrid;

// cell budgets of the coarse (~4N) and the fine (~32N) grid: the workspace holds exactly this many counters per level
static inline int sg_knn_max_cells(int N) { long long c = 4LL * N; if (c < 4096) c = 4096; if (c > (1 << 23)) c = 1 << 23; return (int)c; }
static inline int sg_knn_max_cells_fine(int N) { long long c = 32LL * N; if (c < 4096) c = 4096; if (c > (1 << 25)) c = 1 << 25; return (int)c; }

// dims of cell edge h over the (clamped) extents; returns whether their product fits in max_cells.  A quotient that no int
// holds counts as max_cells + 1 cells and the product saturates there: no overflow, no conversion of a float out of range.
SG_KNN_HD static inline int sg_knn_grid_dims(const float ext[3], float h, int max_cells, int dim[3])
{
    long long n = 1;
    for (int c = 0; c < 3; c++) {
        const float q = ext[c] / h;
        dim[c] = q < (float)max_cells ? (int)q + 1 : max_cells + 1;
        n *= dim[c];
        if (n > (long long)max_cells) n = (long long)max_cells + 1;
    }
    return n <= (long long)max_cells;
}

// Bounding box -> cell edge h with ~max_cells cells in the box, and the dims of THAT h.  For every finite box and every
// max_cells >= 8:  1 <= ncells <= max_cells, every dim >= 1, h and 1 / h finite and positive, dim[c] = (int)(ext[c] / h) + 1
// for the h stored.  The bound is checked on the integers that are stored, whatever cbrtf returned.
//   Each extent counts as at least 1e-3 of the largest, so a thin axis enters the volume estimate as a fraction of a cell
// but the grid as one whole cell: a flat cloud's first h gives up to (10 max_cells^(1/3))^2 cells (6 889 for 4 096).  h
// therefore grows by 1.1 until the dims fit -- a flat sheet needs 10 steps at 4 096 cells, the most of any box in the sweep
// of tests/test_knn_grid_host.py -- and the first eight steps are the ones the earlier, unchecked loop took: a cloud that
// fitted then has the grid it had, bit for bit.
SG_KNN_HD static inline void sg_knn_grid_size(const float mn[3], const float mx[3], int max_cells, SgGrid *grid)
{
    float ext[3], vol = 1.0f, emax = 0.0f;
    for (int c = 0; c < 3; c++) { ext[c] = mx[c] - mn[c]; emax = fmaxf(emax, ext[c]); }
    if (!(emax > 0.0f)) emax = 1.0f;                       // all points coincide
    // (extents beyond 1e-30 .. 3.4e38 -- no cloud in metres -- are sized as if they were inside: memory stays safe)
    emax = fminf(fmaxf(emax, 1e-30f), 3.4e38f);
    for (int c = 0; c < 3; c++) { ext[c] = fminf(fmaxf(ext[c], 1e-3f * emax), emax); vol *= ext[c]; }
    float h = cbrtf(vol / (float)max_cells);
    if (!(h > 0.0f && h <= 3.4e38f)) {                     // the volume left the fp32 range: the same in units of emax
        float v = 1.0f;
        for (int c = 0; c < 3; c++) v *= ext[c] / emax;
        h = emax * cbrtf(v / (float)max_cells);
    }
    int dim[3], fits = 0;
    for (int it = 0; it < 72 && !fits; it++) {             // grow h until the cell count fits
        fits = sg_knn_grid_dims(ext, h, max_cells, dim);
        if (!fits) h *= 1.1f;
    }
    if (!(fits && h <= 3.4e38f)) {                         // (not reached for 1e-30 < emax < 1e36)  one or two cells per axis
        h = emax;
        sg_knn_grid_dims(ext, h, max_cells, dim);
    }
    grid->h = h; grid->inv_h = 1.0f / h;
    for (int c = 0; c < 3; c++) { grid->lo[c] = mn[c]; grid->dim[c] = dim[c]; }
    grid->ncells = dim[0] * dim[1] * dim[2];
}
#endif
