/* TEST INFRASTRUCTURE: the product's k-NN grid sizing (sings_amd/csrc/sg_knn_grid.h, the function thread 0 of
 * sg_grid_setup2_kernel runs) compiled for the CPU, and -- for comparison only -- the loop it replaced. */
#include "../sings_amd/csrc/sg_knn_grid.h"

int sgk_max_cells(int N, int fine) { return fine ? sg_knn_max_cells_fine(N) : sg_knn_max_cells(N); }

/* the loop before the fit was guaranteed, kept word for word: the host tests compare bits with it wherever IT stayed within
 * max_cells, and tools/knn_grid_census.py counts where it did not */
static void sgk_previous(const float mn[3], const float mx[3], int max_cells, SgGrid *grid)
{
    float ext[3], vol = 1.0f, emax = 0.0f;
    for (int c = 0; c < 3; c++) { ext[c] = mx[c] - mn[c]; emax = fmaxf(emax, ext[c]); }
    if (!(emax > 0.0f)) emax = 1.0f;
    for (int c = 0; c < 3; c++) { ext[c] = fmaxf(ext[c], 1e-3f * emax); vol *= ext[c]; }
    float h = cbrtf(vol / (float)max_cells);
    int dim[3];
    for (int it = 0; it < 8; it++) {                       // grow h until the cell count fits
        long long n = 1;
        for (int c = 0; c < 3; c++) { dim[c] = (int)(ext[c] / h) + 1; n *= dim[c]; }
        if (n <= (long long)max_cells) break;
        h *= 1.1f;
    }
    grid->h = h; grid->inv_h = 1.0f / h;
    for (int c = 0; c < 3; c++) { grid->lo[c] = mn[c]; grid->dim[c] = dim[c]; }
    grid->ncells = dim[0] * dim[1] * dim[2];
}

/* n boxes: mn, mx [n][3], max_cells [n] -> grids [n] (which = 0: the product's function, 1: the previous loop) */
void sgk_size_batch(int which, int n, const float *mn, const float *mx, const int *max_cells, SgGrid *out)
{
    for (int i = 0; i < n; i++) {
        if (which) sgk_previous(mn + 3 * i, mx + 3 * i, max_cells[i], out + i);
        else sg_knn_grid_size(mn + 3 * i, mx + 3 * i, max_cells[i], out + i);
    }
}

#ifdef SGK_MAIN
/* Stand-alone check (make -C oracle knn_grid_check: built with the host sanitizers, float-to-int conversions included): the
 * guarantee of sg_knn_grid_size over extents from denormal to the whole fp32 range, flat, thin and cubic, at every budget. */
#include <stdio.h>
int main(void)
{
    static const float thin[] = { 0.0f, 1e-6f, 1e-3f, 0.01f, 0.3f, 1.0f };
    static const int ns[] = { 1, 2, 9, 362, 1000, 1024, 1025, 4000, 4600, 150000, 500000, 1 << 21, 1 << 23, 2147483647 };
    long checked = 0, bad = 0;
    for (int e = -45; e <= 38; e++)
        for (int m = 0; m < 3; m++)
            for (unsigned a = 0; a < 6; a++)
                for (unsigned b = 0; b < 6; b++)
                    for (unsigned k = 0; k < sizeof ns / sizeof *ns; k++)
                        for (int fine = 0; fine < 2; fine++)
                            for (int off = 0; off < 2; off++) {
                                const float s = (m == 0 ? 1.0f : m == 1 ? 3.4f : 7.7f) * powf(10.0f, (float)e);
                                const float o = off ? -0.5f * s : 0.0f;
                                const float mn[3] = { o, o, o }, mx[3] = { o + s, o + s * thin[a], o + s * thin[b] };
                                const int mc = sgk_max_cells(ns[k], fine);
                                SgGrid g;
                                sg_knn_grid_size(mn, mx, mc, &g);
                                const long long n = (long long)g.dim[0] * g.dim[1] * g.dim[2];
                                const int ok = g.dim[0] >= 1 && g.dim[1] >= 1 && g.dim[2] >= 1 && n >= 1 && n <= mc && g.ncells == n &&
                                               g.h > 0.0f && g.h <= 3.4028235e38f && g.inv_h > 0.0f && g.inv_h <= 3.4028235e38f;
                                checked++;
                                if (!ok && bad++ < 10)
                                    printf("BAD: edge %g thin %g %g max_cells %d: dims %d %d %d ncells %d h %g\n", (double)s, (double)thin[a],
                                           (double)thin[b], mc, g.dim[0], g.dim[1], g.dim[2], g.ncells, (double)g.h);
                            }
    printf("%ld boxes checked, %ld break the guarantee\n", checked, bad);
    return bad != 0;
}
#endif
