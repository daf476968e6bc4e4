/*
 * snail_materials.h -- full shading of the primary packets of a plain scene (Scene<BVH>) on the device: the gVals[6] && HasShadingData()
 * branch of Scene::RayTrace (src/scene_trace.cpp:145-358) with per-vertex normals, texture coordinates, a material per triangle and
 * mip-mapped rgb8 textures, then the lights of the simple-shading pipeline of snail_hip.h on those samples.  A header of its own: snail_hip.h
 * and its symbol list stay as they are.  Plain C.
 *
 * NOT here: the mirrored bounce is snail_materials_bounce.h's; 4x antialiasing, depth shading, the tint and tile lists are
 * snail_materials_tiles.h's; the material kinds that can select a transparent lane, their sample stages and the continuation's packets are
 * snail_materials_transparency.h's and the frames of the continuation too (a set that holds such a kind is refused by every function here that takes a set).  The host renderer keeps
 * multi-device frames, the ordered launches (the heat-map, gVals[5], of full shading is snail_materials_heatmap.h's), OBJ vt / vn / usemtl and
 * MTL ingest, the DXT and SAT samplers and rgba8 textures.
 */
#ifndef SNAIL_MATERIALS_H
#define SNAIL_MATERIALS_H
#include "snail_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- data ------------------------------------------------------------------------------------------------------------------------------
 * ShTriangle (src/triangle.h:181-230), 64 bytes = 16 words per triangle: uv[3] (6 floats), nrm[3] (9 floats), matId | flat << 31 (int32).
 * uv[1], uv[2], nrm[1], nrm[2] are stored as DIFFERENCES from element 0 (the constructor subtracts in fp32).  One record per triangle in
 * triId order, i.e. permuted by the builder's perm (BVH slot -> input triangle), as BVH::FindSplitSweep permutes shTris with tris
 * (src/bvh/tree.cpp:123,250).  snail_shtris_pack makes them: uv6 [n][3][2], nrm9 [n][3][3], matIdx [n] (an index into the material MAP
 * below, 0 .. 2^31 - 1), flat [n] (bytes, non-zero = flat) of the INPUT triangles; perm [n] or NULL (identity); out64 [n] records.
 * uv and normals must be finite and |uv| < 2^20 (validated here: non-zero return and a snail_last_error() text otherwise). */
int snail_shtris_pack(const float *uv6, const float *nrm9, const int32_t *matIdx, const uint8_t *flat, int n, const int32_t *perm, void *out64);

/* Textures: rgb8, width and height powers of two, each at most 8192 (so that the level count stays inside the sampler's mipPitch[16]).  A
 * texture is ONE buffer: min(32, log2(max(w, h)) + 1) levels back to back in MipmapTexture order, level m of max(w >> m, 1) x max(h >> m, 1)
 * pixels with the TIGHT pitch 3 * max(w >> m, 1) (the reference takes its pitch from imageRowSize of the absent libfwk; the tight pitch is this
 * project's stated assumption).  snail_texture_size = the bytes of that buffer (0 for a refused shape) and the level count;
 * snail_texture_build copies level0 (w * h * 3 bytes, tight) and restates MipmapTexture::GenMips for rgb8 LITERALLY
 * (src/mipmap_texture.cpp:256-285) -- including the src[4 + i] stride of the height-1 row case, whose read one byte past a pixel pair is
 * defined because the next level follows in the same buffer.  cap = bytes available at out. */
int64_t snail_texture_size(int w, int h, int *nLevels);
int snail_texture_build(const uint8_t *level0, int w, int h, uint8_t *out, int64_t cap, int *nLevels);

enum { SNAIL_MAT_SIMPLE = 0, SNAIL_MAT_TEX = 1, SNAIL_MAT_UBER = 2, SNAIL_MAT_TRANSPARENT = 3 };
/* One material (the headers under src/shading), 40 bytes:
 *   SNAIL_MAT_SIMPLE  SimpleMaterial<nDotR>: diffuse = `diffuse` [* Abs(d.n)], specular = diffuse
 *   SNAIL_MAT_TEX     TexMaterial<nDotR> over PointSampler(`texture`): diffuse = sample [* (d.n), no Abs], specular = diffuse; the only kind
 *                     with Material::fTexCoords
 *   SNAIL_MAT_UBER    UberMaterial: `diffuse` / `specular` / `dissolve` are the MaterialDesc's; the constructor's Swap(diffuse.x, diffuse.z) is
 *                     applied by snail_materials_create.  diffuse * Abs(d.n); specular = the sample's diffuse on the unmasked path, `specular`
 *                     on the masked one
 *   SNAIL_MAT_TRANSPARENT  refused here (below); accepted by snail_materials_create_transparent (snail_materials_transparency.h) */
typedef struct SnailMaterial {
	int32_t kind, nDotR;
	float diffuse[3], specular[3];
	float dissolve;
	int32_t texture;
} SnailMaterial;
typedef struct SnailTexture {
	const uint8_t *levels;   /* HOST pointer: the buffer of snail_texture_build */
	int32_t width, height;
} SnailTexture;

/* ---- the material set of a scene ----------------------------------------------------------------------------------------------------------
 * shtris64: nTris records (= the scene's triangle count), triId order.  matMap [nMap]: BVH::GetMaterialId(idx) = materials[idx].id
 * (src/bvh/tree.h:74-84) as int32, -1 = the scene's defaultMat = SimpleMaterial<true>(1, 1, 1) (src/scene.cpp:6), otherwise an index into
 * mats [nMats].  Everything is copied (textures with 4 bytes of padding: the sampler reads 4 bytes per tap and uses 3).  The scene must
 * outlive the set.  REFUSED (NULL, snail_last_error() says why), before anything touches a device: a record whose matId is outside the map, a
 * map entry outside -1 .. nMats - 1, a texture index outside the textures, a texture that is no power of two or larger than 8192, and every
 * material that could select a transparent lane: SNAIL_MAT_TRANSPARENT, or SNAIL_MAT_UBER with 0 < dissolve < 1 or a NaN dissolve (UBER with
 * dissolve <= 0 or >= 1 carries fTransparency at most, and opacity < 1 never holds for it). */
typedef struct SnailMaterials SnailMaterials;
SnailMaterials *snail_materials_create(SnailScene *scene, const void *shtris64, int nTris, const int32_t *matMap, int nMap, const SnailMaterial *mats,
                                       int nMats, const SnailTexture *textures, int nTex);
void snail_materials_destroy(SnailMaterials *);

/* ---- the sample stage ---------------------------------------------------------------------------------------------------------------------
 * The samples of a packet list from its hit records -- packet-major t, u, v, triId as snail_trace_packets_dev writes them (bar.x = u,
 * bar.y = v) -- with the rays generated again: per ray 9 floats (normal, diffuse, specular), component-major
 * d_samples [nPackets][9][64 quads][4 lanes].  The three branches of src/scene_trace.cpp:171-356 as written:
 *   (a) a block of 4 quads, all 16 rays on ONE triangle: Shade unmasked; without texture coordinates the normal is nrm0 (flat flag) or
 *       nrm0 + (nrm1 bx + nrm2 by); with them (nrm0 + nrm1 bx) + nrm2 by (the flat flag is not looked at), texCoord = (uv0 + uv1 bx) + uv2 by and
 *       texDiff = Maximize - Minimize of the quad's texCoord: the only place where the sampler picks a mip above 0
 *   (b) otherwise per quad: lane 0's triangle supplies texCoord, normal ((a + b bx) + c by) and material for the quad if lane 0 hit; lanes 1..3
 *       take their own triangle's when it differs from lane 0's (triId 0 stands for a lane 0 that missed: a lane that hit triangle 0 beside it
 *       keeps the default material and zero normal / texCoord); texDiff = 0; all 16 rays hit and ONE material: Shade unmasked
 *   (c) several materials: every hit lane by its own material on the MASKED path (UBER: specular = `specular`)
 * PointSampler::Sample (src/sampling/point_sampler.cpp:126-210) op for op.  Values the reference reads before it writes them are zeros, and
 * so is everything of a lane that missed.  triIds outside the scene are clamped.  Preconditions: uv and normals finite, |uv| < 2^20. */
int snail_materials_shade_packets_dev(SnailMaterials *, const float cam[13], int resx, int resy, const int32_t *d_packet_xy, int nPackets, const float *d_t,
                                      const float *d_u, const float *d_v, const int32_t *d_triId, float *d_samples, void *stream);

/* ---- lit frames ---------------------------------------------------------------------------------------------------------------------------
 * Primary packets -> samples -> per light the packet-level cull and Scene::TraceLight on the samples' normals (N.L uses the interpolated
 * normal) -> outColor = diffuse * lDiffuse + specular * lSpecular -> ConvColor -> B,G,R.  Conventions of snail_render_whitted_dev /
 * _packets_dev / snail_render_image (lights7 a HOST pointer to 0..SNAIL_MAX_LIGHTS x {pos[3], color[3], radius}; the store rule; d_stats /
 * stats += {intersects, iterations, traced rays, skips}, rays = primary rays + shadow lanes with N.L > 0; the scene's arithmetic), without
 * their `color` (the default material's colour is the scene's (1, 1, 1)).  flags: must be 0.  Intermediates live in the set, 8 per set in flight,
 * each guarded by an event; launches are booked under the scene's lock. */
int snail_render_materials_dev(SnailMaterials *, const float cam[13], int resx, int resy, const float *lights7, int nLights, const float ambient[3],
                               int flags, uint8_t *d_frame_bgr, int pitch, uint64_t *d_stats, void *stream);
int snail_render_materials_packets_dev(SnailMaterials *, const float cam[13], int resx, int resy, const int32_t *d_packet_xy, int nPackets,
                                       const float *lights7, int nLights, const float ambient[3], int flags, uint8_t *d_bgr_packets, uint64_t *d_stats,
                                       void *stream);
int snail_render_materials_image(SnailMaterials *, const float cam[13], int resx, int resy, const float *lights7, int nLights, const float ambient[3],
                                 int flags, uint8_t *image_bgr, int pitch, uint64_t stats[4]);

#ifdef __cplusplus
}
#endif
#endif
