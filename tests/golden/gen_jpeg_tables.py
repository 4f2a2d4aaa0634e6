"""Writes tests/golden/jpeg_tables.npz: the Annex K quantisation and Huffman tables, read out of a file written by a decoder-side
library we did not write.

A non-optimised JPEG that PIL (libjpeg) writes at ``quality=50, subsampling=0`` carries the base tables unscaled (libjpeg's scale at
quality 50 is 100 %) in its DQT segments, in zig-zag order, and the four standard Huffman tables in its DHT segments.  This script
parses those segments and stores

    quant_luma, quant_chroma          [64] uint8, zig-zag order
    dc0_bits, ac0_bits, dc1_bits, ac1_bits   [16] uint8: codes per length 1..16
    dc0_vals, ac0_vals, dc1_vals, ac1_vals   the symbols in code order

``sings_amd/video.py`` keeps the same numbers as literals; tests/test_video_host.py holds the two to each other.

    python tests/golden/gen_jpeg_tables.py
"""
import io
import os
import struct

import numpy as np


def segments(data):
    """(marker, payload) of every segment in front of the entropy-coded data."""
    assert data[:2] == b"\xff\xd8"
    pos = 2
    while True:
        assert data[pos] == 0xFF
        marker = data[pos + 1]
        n = struct.unpack(">H", data[pos + 2:pos + 4])[0]
        yield marker, data[pos + 4:pos + 2 + n]
        if marker == 0xDA:
            return
        pos += 2 + n


def tables_of(data):
    out = {}
    for marker, p in segments(data):
        if marker == 0xDB:                                        # DQT: (precision << 4 | id), 64 bytes; several per segment
            while p:
                assert p[0] >> 4 == 0, "8-bit tables expected"
                out["quant_luma" if (p[0] & 15) == 0 else "quant_chroma"] = np.frombuffer(p[1:65], dtype=np.uint8).copy()
                p = p[65:]
        elif marker == 0xC4:                                      # DHT: (class << 4 | id), 16 counts, the symbols
            while p:
                name = ("dc" if p[0] >> 4 == 0 else "ac") + str(p[0] & 15)
                bits = np.frombuffer(p[1:17], dtype=np.uint8).copy()
                n = int(bits.sum())
                out[name + "_bits"], out[name + "_vals"] = bits, np.frombuffer(p[17:17 + n], dtype=np.uint8).copy()
                p = p[17 + n:]
    return out


def main():
    from PIL import Image
    rng = np.random.default_rng(0)
    img = Image.fromarray(rng.integers(0, 256, (16, 16, 3), dtype=np.uint8), "RGB")
    f = io.BytesIO()
    img.save(f, "JPEG", quality=50, subsampling=0, optimize=False)
    t = tables_of(f.getvalue())
    assert sorted(t) == sorted(["quant_luma", "quant_chroma"] + [f"{c}{i}_{w}" for c in ("dc", "ac") for i in (0, 1)
                                                                 for w in ("bits", "vals")]), sorted(t)
    assert t["quant_luma"][:8].tolist() == [16, 11, 12, 14, 12, 10, 16, 14] and len(t["ac0_vals"]) == 162
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_tables.npz")
    np.savez(path, **t)
    print(path, {k: v.shape for k, v in t.items()})


if __name__ == "__main__":
    main()
