"""What tests/test_materials_tiles_host.py and tests/test_gpu_materials_tiles.py share: the tile list, its offsets, the frames, and ONE
restatement object per case (tests/materials_tiles_ref.py; its memo holds every reference colour once, for both files).  The cases are those
of tests/materials_bounce_cases.py.  Nothing here touches the product library."""
from __future__ import annotations

import functools

import numpy as np

from tests import dbvh_shade_ref as S
from tests import materials_bounce_cases as BK
from tests import materials_tiles_ref as MT

REFL, DEPTH, AA = MT.REFLECTIONS, MT.DEPTH, MT.AA4
RES = (44, 70)
# the reference's tile size; a tile over the right edge; one over the bottom edge; an unaligned origin with a size that is no multiple of 16 or 4;
# a tile narrower than a quad.  21 packets, 84 under AA.
TILES = np.array([(0, 0, 16, 64), (16, 0, 16, 64), (32, 0, 16, 64), (0, 64, 16, 64), (8, 8, 20, 24), (40, 3, 3, 5)], dtype=np.int32)
OTHER_TILES = np.array([(16, 32, 28, 38), (0, 0, 9, 70), (3, 40, 16, 16)], dtype=np.int32)      # a second list, for the cache rebuild
PACKET_RES = (48, 32)            # 6 packets
IMAGE_RES = (35, 25)


def tile_sizes(tiles):
    t = np.asarray(tiles).reshape(-1, 4)
    return 3 * t[:, 2].astype(np.int64) * t[:, 3]


def scattered_offsets(tiles, order=None, gaps=(4, 3, 8, 5, 2, 7), start=2):
    """offsets out of order with gaps between the tiles (some offsets odd: the store's byte path) -> (offsets int64 [n], total bytes, inside bool [total])"""
    size = tile_sizes(tiles)
    n = len(size)
    order = list(order) if order is not None else [(3 * k + n // 2) % n if n % 3 else (n - 1 - k) for k in range(n)]
    assert sorted(order) == list(range(n))
    off = np.zeros(n, dtype=np.int64)
    pos = start
    for j, k in enumerate(order):
        off[k] = pos
        pos += int(size[k]) + gaps[j % len(gaps)]
    inside = np.zeros(pos, dtype=bool)
    for o, s in zip(off.tolist(), size.tolist()):
        assert not inside[o:o + s].any()
        inside[o:o + s] = True
    return off, pos, inside


OFFSETS, TOTAL, INSIDE = scattered_offsets(TILES, order=[3, 0, 5, 1, 4, 2])


def camera(name, res):
    """the case's camera for a frame of this module: `small` at 35 x 25 takes cam70 (closer), everything else the case's first camera"""
    c = BK.case(name)
    return c["cam70"] if (name == "small" and tuple(res) == IMAGE_RES) else c["cam"]


@functools.lru_cache(maxsize=None)
def tref(name):
    return MT.MaterialTilesRef(BK.materials_ref(name))


def diag_of(name, res, packet_xy, flags, mode, lights_key="case"):
    """the restatement's diagnostics of the frames the GPU tests use (a run of its own: colours with a Diag are not memoised)"""
    d = MT.new_diag(flags)
    tref(name).colors(camera(name, res).as_array13(), res[0], res[1], packet_xy, BK.lights_of(name, lights_key), flags, mode=mode, diag=d)
    return d


def frame_xy(res):
    return S.frame_packets(res[0], res[1])
