"""Test-side restatement of the reference's scene-complexity colour (gVals[5]; src/scene_trace.cpp:62-76, :513-517) in numpy float32.

    heat_rgb(stats4)       -> float32[3]  (r, g, b) = (float(intersects) * (0.002f / 64), float(iterations) * (0.02f / 64), float(skips * 0.25f))
    heat_bgr_bytes(stats4) -> uint8[3]    ConvColor of it: Trunc(Clamp(c * 255, 0, 255)) per channel, stored B, G, R (src/render.cpp:11-17)
    heat_aa_bgr_bytes(stats4) -> uint8[3] the 2x2 reduction of FOUR equal colours first: ((c + c) * 0.25) + ((c + c) * 0.25) (src/render.cpp:71-110)

stats4 = {intersects, iterations, rays, skips} (the order of d_stats); rays does not enter.  Every operation is one float32 operation, separately
rounded.  tests/test_heatmap_host.py pins these functions on literal bit patterns that were derived ONCE with this stand-alone program (built with
`g++ -O0 -ffp-contract=off`; it is not part of any build):

    #include <cstdio>
    #include <cstring>
    int main() { unsigned t[][4] = {{0,0,256,0},{1,1,256,1},{12345,678,300,2},{40000,4000,512,3},{32000,3200,256,4},{4000000000u,4000000000u,256,7},{31999,3199,256,0}}; int size = 64;
      for(auto &s : t) { float c[3] = {float(s[0]) * (0.002f / size), float(s[1]) * (0.02f / size), float(s[3] * 0.25f)}; unsigned b[3]; memcpy(b, c, 12);
        printf("(%uu,%u,%u,%u): 0x%08x 0x%08x 0x%08x |", s[0], s[1], s[2], s[3], b[0], b[1], b[2]);
        for(int k = 2; k >= 0; k--) { float v = c[k] * 255.0f; v = v > 0.0f ? v : 0.0f; v = v < 255.0f ? v : 255.0f; printf(" %d", (int)v); } printf("\\n"); } }
"""
from __future__ import annotations

import numpy as np

F = np.float32
_KR = F(0.002) / F(64)
_KG = F(0.02) / F(64)


def heat_rgb(stats4) -> np.ndarray:
    s = [int(x) & 0xFFFFFFFF for x in np.asarray(stats4).reshape(4).tolist()]
    return np.array([F(np.uint32(s[0])) * _KR, F(np.uint32(s[1])) * _KG, F(np.uint32(s[3])) * F(0.25)], dtype=np.float32)


def conv_color(rgb) -> np.ndarray:
    """ConvColor: (r, g, b) floats -> B, G, R bytes"""
    out = np.zeros(3, dtype=np.uint8)
    for k, c in enumerate(np.asarray(rgb, dtype=np.float32)[::-1]):
        v = F(c) * F(255.0)
        v = v if v > F(0.0) else F(0.0)
        v = v if v < F(255.0) else F(255.0)
        out[k] = int(v)
    return out


def heat_bgr_bytes(stats4) -> np.ndarray:
    return conv_color(heat_rgb(stats4))


def heat_aa_bgr_bytes(stats4) -> np.ndarray:
    c = heat_rgb(stats4)
    return conv_color((c + c) * F(0.25) + (c + c) * F(0.25))


def heat_packets(pstats) -> np.ndarray:
    """[n, 4] counters -> packet-major bytes [n, 256, 3]: every ray of a packet carries the packet's colour"""
    ps = np.asarray(pstats).reshape(-1, 4)
    return np.stack([np.tile(heat_bgr_bytes(p), (256, 1)) for p in ps])


def heat_frame(pstats, xy, resx, resy) -> np.ndarray:
    """[n, 4] counters of the packets at xy -> the frame [resy, resx, 3] (pixels outside the image dropped)"""
    f = np.zeros((resy, resx, 3), dtype=np.uint8)
    for p, (x, y) in zip(np.asarray(pstats).reshape(-1, 4), np.asarray(xy).reshape(-1, 2).tolist()):
        f[y:y + 16, x:x + 16] = heat_bgr_bytes(p)
    return f


def heat_aa_packets(pstats4) -> np.ndarray:
    """[n, 4, 4] counters of the four double-resolution packets of every packet -> packet-major bytes [n, 256, 3]: the 8x8 quadrant
    (k & 1, k >> 1) of a packet carries the reduced colour of sub-packet k"""
    ps = np.asarray(pstats4).reshape(-1, 4, 4)
    out = np.zeros((len(ps), 16, 16, 3), dtype=np.uint8)
    for i, four in enumerate(ps):
        for k in range(4):
            out[i, 8 * (k >> 1):8 * (k >> 1) + 8, 8 * (k & 1):8 * (k & 1) + 8] = heat_aa_bgr_bytes(four[k])
    return out.reshape(len(ps), 256, 3)


def packets_to_frame(bgr_packets, xy, resx, resy) -> np.ndarray:
    f = np.zeros((resy, resx, 3), dtype=np.uint8)
    for blk, (x, y) in zip(np.asarray(bgr_packets).reshape(-1, 16, 16, 3), np.asarray(xy).reshape(-1, 2).tolist()):
        h, w = min(16, resy - y), min(16, resx - x)
        if h > 0 and w > 0:
            f[y:y + h, x:x + w] = blk[:h, :w]
    return f
