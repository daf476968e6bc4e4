"""A numpy restatement of what the device pack of include/snail_materials_dynamic.h computes besides snail_shtris_pack: the face normal of
BaseScene::Object::GetTriangle for a triangle without vn (src/base_scene.cpp:313-314) with veclib's scalar definitions
(veclib/vec3.h:92-106, veclib/vecbase.h:56), every fp32 operation rounded separately, and the header's one deviation (a triangle with a
non-finite normal component gets three zero normals).  Nothing here touches the product library."""
from __future__ import annotations

import numpy as np

F = np.float32


def face_normals(tri_verts) -> np.ndarray:
    """tri_verts [n, 3, 3] -> fnrm [n, 3] float32: fnrm = (p1 - p0) ^ (p2 - p0); fnrm *= 1.0f / Sqrt(fnrm | fnrm), the dot product summed
    left to right.  A zero-area triangle gives 0 * inf = NaN, as the reference does."""
    p = np.ascontiguousarray(tri_verts, dtype=F).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        b = (p[:, 1] - p[:, 0]).astype(F)
        c = (p[:, 2] - p[:, 0]).astype(F)
        mul = lambda x, y: (x * y).astype(F)      # noqa: E731
        fx = (mul(b[:, 1], c[:, 2]) - mul(b[:, 2], c[:, 1])).astype(F)
        fy = (mul(b[:, 2], c[:, 0]) - mul(b[:, 0], c[:, 2])).astype(F)
        fz = (mul(b[:, 0], c[:, 1]) - mul(b[:, 1], c[:, 0])).astype(F)
        d = ((mul(fx, fx) + mul(fy, fy)).astype(F) + mul(fz, fz)).astype(F)
        r = (F(1) / np.sqrt(d).astype(F)).astype(F)
        return np.stack([mul(fx, r), mul(fy, r), mul(fz, r)], axis=1)


def vertex_normals_from_faces(tri_verts) -> np.ndarray:
    """[n, 3, 3]: the face normal at all three vertices (out.nrm[k] = out.fnrm)"""
    return np.repeat(face_normals(tri_verts)[:, None, :], 3, axis=1).copy()


def zero_nonfinite(nrm):
    """the deviation: -> (nrm [n, 3, 3] with the triangles that hold a non-finite component set to zero, how many there were)"""
    nr = np.array(nrm, dtype=F).reshape(-1, 3, 3)
    bad = ~np.isfinite(nr).all(axis=(1, 2))
    nr[bad] = 0.0
    return nr, int(bad.sum())
