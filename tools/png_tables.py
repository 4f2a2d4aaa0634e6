"""Regenerates the code lengths of the pre-built dynamic Huffman tables of the device PNG encoder (``sings_amd/png.py`` CODE_LENGTHS;
INTEGRATION.md §24).  Integer arithmetic only, so every machine prints the same literals:

    python tools/png_tables.py            # the four tuples, ready to paste
    python tools/png_tables.py --check    # exit status 1 when sings_amd/png.py holds other numbers

The model.  A filtered residual byte v costs by its distance from zero, d = min(v, 256 - v); table i spreads the literals as
weight(v) = floor(2^48 r_i^d) + 1 with r = 1/2, 3/4, 22/25, 19/20.  End-of-block and the 29 length symbols share a small part of the
literals' mass S: S / 2048 for symbol 256, S / 128 for symbol 285 (a 258-byte match: what a flat region is made of), S / (256 (j + 1))
for length symbol 257 + j.  The lengths are those of a Huffman code over these weights, limited to 15 bits: longer codes are cut to
15, the least likely shorter codes are lengthened until the code fits, and the most likely codes are shortened again while room is
left, so the Kraft sum is exactly 1 and every one of the 286 symbols has a code.
"""
import heapq
import os
import sys
from fractions import Fraction

SPREADS = (Fraction(1, 2), Fraction(3, 4), Fraction(22, 25), Fraction(19, 20))
SYMBOLS = 286
MAX_BITS = 15


def weights(r):
    lit = [(r.numerator ** min(v, 256 - v) << 48) // r.denominator ** min(v, 256 - v) + 1 for v in range(256)]
    S = sum(lit)
    lengths = [S // (256 * (j + 1)) + 1 for j in range(29)]
    lengths[28] = S // 128 + 1
    return lit + [S // 2048 + 1] + lengths


def limited_lengths(w, limit):
    """Code lengths of a complete prefix code over every symbol of ``w`` (all weights > 0), none longer than ``limit``."""
    n = len(w)
    if n == 1:
        return [1]
    heap = [(w[i], i, (i,)) for i in range(n)]                    # (weight, tie-break, leaves)
    heapq.heapify(heap)
    depth = [0] * n
    serial = n
    while len(heap) > 1:
        a = heapq.heappop(heap)
        b = heapq.heappop(heap)
        for i in a[2] + b[2]:
            depth[i] += 1
        heapq.heappush(heap, (a[0] + b[0], serial, a[2] + b[2]))
        serial += 1
    depth = [min(d, limit) for d in depth]
    unit = lambda d: 1 << (limit - d)
    kraft, full = sum(unit(d) for d in depth), 1 << limit
    by_rarity = sorted(range(n), key=lambda i: (w[i], i))
    while kraft > full:                                           # lengthen the least likely code that is still short
        for i in by_rarity:
            if depth[i] < limit:
                kraft -= unit(depth[i]) - unit(depth[i] + 1)
                depth[i] += 1
                break
    changed = True
    while kraft < full and changed:                               # shorten the most likely code that still fits
        changed = False
        for i in reversed(by_rarity):
            if depth[i] > 1 and kraft + unit(depth[i]) <= full:
                kraft += unit(depth[i])
                depth[i] -= 1
                changed = True
                break
    assert kraft == full and all(1 <= d <= limit for d in depth)
    return depth


def code_lengths():
    return tuple(tuple(limited_lengths(weights(r), MAX_BITS)) for r in SPREADS)


def render(tables):
    lines = ["CODE_LENGTHS = ("]
    for t in tables:
        lines.append("    (")
        for i in range(0, len(t), 32):
            lines.append("        " + " ".join(f"{v}," for v in t[i:i + 32]))
        lines.append("    ),")
    lines.append(")")
    return "\n".join(lines)


if __name__ == "__main__":
    tables = code_lengths()
    if "--check" in sys.argv[1:]:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
        from sings_amd import png
        sys.exit(0 if tuple(map(tuple, png.CODE_LENGTHS)) == tables else 1)
    print(render(tables))
