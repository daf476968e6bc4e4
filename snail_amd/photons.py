"""Photons: the record of include/snail_wide.h (`struct Photon`, src/photons.h:7-24) and a NumPy stand-in for the emission loop of
TracePhotons (src/photons.cpp:217-237).

The device side (Scene.trace_photons) takes rays as an INPUT.  The reference draws them from std::tr1::mt19937 streams seeded per light
and per 8192-ray step, through libm's sin / cos and a rejection loop; `emit` restates the same stratified sampling of the sphere and the
same offset rule with NumPy's generator, and is NOT claimed equal to the reference's random stream -- only its distribution."""
from __future__ import annotations

import numpy as np

PHOTON = np.dtype([("position", "<f4", 3), ("direction", "<f4", 3), ("color", "u1", 4), ("temp", "<u4")])
assert PHOTON.itemsize == 32

LIGHT_SIZE = 4.0   # `lightSize` of TracePhotons: offsets with LengthSq(offset) > 4 are drawn again


def emit(light_pos, count: int, seed: int = 1):
    """`count` photon rays of one light -> (origin float32 [count, 3], dir float32 [count, 3]).

    Directions: tcount = int(sqrt(count)) strata per axis, u1 = (n % tcount + 0.75 (r - 0.5)) / tcount, u2 = (n // tcount + 0.75 (r - 0.5)) /
    tcount, UniformSampleSphere(u1, u2) = (r cos phi, r sin phi, z) with z = 1 - 2 u1, r = sqrt(max(0, 1 - z^2)), phi = 2 pi u2.
    Origins: light_pos + offset, offset = (r - 0.5) * 4 per component, drawn again while its squared length exceeds 4.  Deterministic in
    `seed`."""
    count = int(count)
    rng = np.random.RandomState(seed)
    f32 = np.float32
    n = np.arange(count, dtype=np.int64)
    tcount = max(int(np.sqrt(count)), 1)
    itc = f32(1.0) / f32(tcount)
    r1 = rng.random_sample(count).astype(f32)
    r2 = rng.random_sample(count).astype(f32)
    u1 = ((n % tcount).astype(f32) + f32(0.75) * (r1 - f32(0.5))) * itc
    u2 = ((n // tcount).astype(f32) + f32(0.75) * (r2 - f32(0.5))) * itc
    z = f32(1.0) - f32(2.0) * u1
    r = np.sqrt(np.maximum(f32(0.0), f32(1.0) - z * z)).astype(f32)
    phi = (f32(2.0 * np.pi) * u2).astype(f32)
    dirs = np.stack([r * np.cos(phi).astype(f32), r * np.sin(phi).astype(f32), z], axis=1).astype(f32)
    off = np.full((count, 3), np.inf, dtype=f32)
    todo = np.arange(count)
    while len(todo):
        off[todo] = ((rng.random_sample((len(todo), 3)).astype(f32) - f32(0.5)) * f32(LIGHT_SIZE)).astype(f32)
        todo = todo[(off[todo] * off[todo]).sum(axis=1) > LIGHT_SIZE]
    origin = (np.asarray(light_pos, dtype=f32).reshape(1, 3) + off).astype(f32)
    return np.ascontiguousarray(origin), np.ascontiguousarray(dirs)
