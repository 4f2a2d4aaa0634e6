#!/usr/bin/env python3
"""Census of the k-NN grid sizing on the host (no GPU): over the random sweep of tests/test_knn_grid_host.py, how often the sizing
loop that sg_knn_grid.h replaced stored more cells than the workspace holds (oracle/knn_grid_host.c keeps that loop for this
purpose), the worst ratio per level and decade of N, how many growth steps the present function takes, and the flat clouds on
which the defect was found as the present function sizes them.  Prints markdown (LAB.md, "k-NN grids on degenerate clouds")."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from oracle import knn_grid                      # noqa: E402
import test_knn_grid_host as T                  # noqa: E402


def main():
    lo, hi, N = T._sweep()
    print(f"sweep: {len(N)} boxes\n")
    print("| level | overflowed before | now | largest N that overflowed | growth steps now (max) |\n|---|---|---|---|---|")
    rows = {}
    for fine in (0, 1):
        mc = T._max_cells(N, fine)
        p = knn_grid.size_batch(lo, hi, mc, previous=True)
        g = knn_grid.size_batch(lo, hi, mc)
        bad_p, bad_g = ~T._valid(p, mc), ~T._valid(g, mc)
        ext = np.maximum(hi - lo, np.float32(1e-3) * (hi - lo).max(1, keepdims=True)).astype(np.float64)
        h0 = np.cbrt(ext.prod(1) / mc)
        steps = np.rint(np.log(g["h"].astype(np.float64) / h0) / np.log(1.1)).astype(int)
        print(f"| {'fine' if fine else 'coarse'} | {bad_p.sum()} | {bad_g.sum()} | {N[bad_p].max()} | {steps.max()} |")
        rows[fine] = (mc, p, bad_p)
    print("\nworst ncells / max_cells of the previous loop, by decade of N (overflowing boxes / boxes):\n")
    print("| N | coarse | fine |\n|---|---|---|")
    for d in range(7):
        sel = (N >= 10 ** d) & (N < 10 ** (d + 1))
        cells = []
        for fine in (0, 1):
            mc, p, bad = rows[fine]
            r = p["ncells"][sel].astype(np.float64) / mc[sel]
            cells.append(f"{r.max():.3f} ({(bad & sel).sum()} / {sel.sum()})")
        print(f"| 1e{d} .. 1e{d + 1} | {cells[0]} | {cells[1]} |")
    print("\nthe flat clouds on which the defect was found, before -> now:\n")
    print("| cloud | N | level | dims before | ncells before | dims now | ncells now | max_cells |\n|---|---|---|---|---|---|---|---|")
    for ext, n, fine, _, mc in T.TABLE:
        a = knn_grid.size_batch([[0, 0, 0]], [ext], [mc], previous=True)[0]
        b = knn_grid.size_batch([[0, 0, 0]], [ext], [mc])[0]
        f = lambda g: " x ".join(str(int(v)) for v in g["dim"])
        print(f"| {ext[0]:g} x {ext[1]:g} sheet, z constant | {n} | {'fine' if fine else 'coarse'} | {f(a)} | {int(a['ncells'])} | {f(b)} | "
              f"{int(b['ncells'])} | {mc} |")


if __name__ == "__main__":
    main()
