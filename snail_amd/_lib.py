"""ctypes binding of libsnailhip.so (the C-ABI of include/snail_hip.h).

There is NO fallback: if the HIP library is missing or a call fails, SnailError is raised.  Nothing in
this package imports or calls the CPU oracle under oracle/ (that is test infrastructure)."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# SNAIL_LIB_PATH: load another build of the same C-ABI (an experiment of tools/variant.sh, or the workbench build libsnailhip_debug.so
# when a whole process should run under its SNAIL_DEBUG_* environment switches) without touching the product library
LIB_PATH = os.environ.get("SNAIL_LIB_PATH") or os.path.join(HERE, "libsnailhip.so")


class SnailError(RuntimeError):
    pass


_lib = None

# name -> (restype, argtypes); kept in one table so tests can check every symbol of include/snail_hip.h
_VP, _I, _F13 = C.c_void_p, C.c_int, C.c_void_p
SIGNATURES = {
    "snail_last_error": (C.c_char_p, []),
    "snail_device_count": (_I, []),
    "snail_tris_from_verts": (_I, [_VP, _I, _VP]),
    "snail_bvh_build": (_I, [_VP, _I, _VP, _VP, _VP, _VP]),
    "snail_scene_create": (_VP, [_VP, _I, _VP, _I, _I, _I]),
    "snail_scene_destroy": (None, [_VP]),
    "snail_scene_info": (_I, [_VP, _VP, _VP, _VP, _VP]),
    "snail_scene_flags": (_I, [_VP, _VP, _VP]),
    "snail_scene_set_arith": (_I, [_VP, _I]),
    "snail_scene_arith": (_I, [_VP, _VP]),
    "snail_host_sse_tables": (_I, [_VP]),
    "snail_arith_set_tables": (_I, [_VP]),
    "snail_arith_prepare_device": (_I, []),
    "snail_host_sse_check": (_I, [_I, C.c_uint64, C.c_uint64, _I, _VP, _VP]),
    "snail_scene_create_lbvh": (_VP, [_VP, _I, _I, _I, _VP, _VP]),
    "snail_scene_download": (_I, [_VP, _VP, _VP]),
    "snail_trace_primary": (_I, [_VP, _F13, _I, _I, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _VP]),
    "snail_trace_frame_packets": (_I, [_VP, _F13, _I, _I, _VP, _VP, _VP, _VP, _VP]),
    "snail_trace_primary_dev": (_I, [_VP, _F13, _I, _I, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_trace_packets_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_trace_packets_shaded_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _VP, _VP]),
    "snail_trace_primary_batch_dev": (_I, [_VP, _I, _VP, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_trace_packets_shaded_batch_dev": (_I, [_VP, _I, _VP, _I, _I, _VP, _I, _VP, _VP, _VP]),
    "snail_trace_primary_batch_reorder_dev": (_I, [_VP, _I, _VP, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I, _VP]),
    "snail_render_whitted_reorder_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _VP, _I, _VP, _I, _VP, _VP, _VP, _VP, _I, _VP]),
    "snail_primary_slots": (_I, [_I, _I]),
    "snail_trace_primary_ordered_dev": (_I, [_VP, _F13, _I, _I, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_trace_packets_ordered_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_order_from_cost_dev": (_I, [_VP, _I, _VP, _VP]),
    "snail_order_from_cost_hint_dev": (_I, [_VP, _I, _VP, _I, _VP]),
    "snail_packets_to_frame_dev": (_I, [_VP, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_trace_rays": (_I, [_VP, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_trace_rays_dev": (_I, [_VP, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_trace_shadow": (_I, [_VP, _I, _I, _VP, _VP, _VP, _VP, _VP]),
    "snail_trace_shadow_dev": (_I, [_VP, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_shade_depth_dev": (_I, [_VP, _I, _VP, _VP]),
    "snail_shade_depth_arith_dev": (_I, [_VP, _I, _VP, _I, _VP]),
    "snail_packets_bgr_to_frame_dev": (_I, [_VP, _I, _I, _I, _VP, _VP, _I, _VP]),
    "snail_packets_bgr_to_frame_chunked_dev": (_I, [_VP, _I, _I, C.c_int64, _I, _I, _VP, _VP, _I, _VP]),
    "snail_packets_bgr_to_planar_dev": (_I, [_VP, _VP, _VP, _I, _VP, _VP, _VP]),
    "snail_planar_to_frame_dev": (_I, [_VP, _VP, _I, _VP, _VP, _I, _I, _I, _VP]),
    "snail_render_whitted_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _VP, _I, _VP, _I, _VP, _VP]),
    "snail_render_whitted_ordered_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _VP, _I, _VP, _I, _VP, _VP, _VP, _VP]),
    "snail_render_whitted_packets_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _VP, _VP, _I, _VP, _VP, _VP]),
    "snail_trace_transparency_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _VP, _VP, _VP, _I, _VP, _VP, _VP, _VP, _VP]),
    "snail_render_tiles": (_I, [_VP, _F13, _I, _I, _VP, _VP, _I, _VP, _I, _VP, _VP, _I, _VP, _VP]),
    "snail_render_tiles_multi": (_I, [_VP, _I, _F13, _I, _I, _VP, _VP, _I, _VP, _I, _VP, _VP, _I, _VP, _VP]),
    "snail_render_image": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _VP, _I, _VP, _I, _VP]),
    "snail_account_primary": (_I, [_VP, _F13, _I, _I, _I, _I, _I, _I, _VP]),
    "snail_account_packets": (_I, [_VP, _F13, _I, _I, _VP]),
    "snail_last_launch": (_I, [_VP, _VP, _VP]),
}

# include/snail_instances.h (snail_amd/instances.py): a table of its own, because SIGNATURES is the list that
# tests/c/abi_c.c takes the address of, entry for entry
INSTANCES_SIGNATURES = {
    "snail_instances_build": (_I, [_VP, _VP, _I, _VP, _I, _VP, _VP, _VP, _VP]),
    "snail_instances_create": (_VP, [_VP, _I, _VP, _I, _VP, _VP, _I, _I]),
    "snail_instances_update": (_I, [_VP, _VP, _I, _VP, _VP, _I, _I, _VP]),
    "snail_instances_destroy": (None, [_VP]),
    "snail_instances_trace_primary_dev": (_I, [_VP, _F13, _I, _I, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_instances_trace_packets_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_instances_trace_rays_dev": (_I, [_VP, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_instances_trace_shadow_dev": (_I, [_VP, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_instances_trace_rays": (_I, [_VP, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_instances_trace_shadow": (_I, [_VP, _I, _I, _VP, _VP, _VP, _VP, _VP]),
    "snail_instances_trace_frame_packets": (_I, [_VP, _F13, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_instances_render_depth": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP]),
}

# include/snail_instances_shade.h (the lit frames of instanced scenes; part of snail_instances.h): a table of its own for the same reason --
# tests/c/instances_c.c enumerates INSTANCES_SIGNATURES entry for entry, tests/c/instances_shade_c.c this one
INSTANCES_SHADE_SIGNATURES = {
    "snail_instances_render_whitted_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _VP, _I, _VP, _I, _VP, _VP]),
    "snail_instances_render_whitted_packets_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _VP, _VP, _I, _VP, _VP, _VP]),
    "snail_instances_render_image": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _VP, _I, _VP, _I, _VP]),
}

# include/snail_instances_tiles.h (the tile renderer of instanced scenes; part of snail_instances.h): again a table of its own -- the tests of the
# two headers above count their entries; tests/c/instances_tiles_c.c enumerates this one
INSTANCES_TILES_SIGNATURES = {
    "snail_instances_shade_packets_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _VP, _VP, _I, _VP, _VP, _VP, _VP]),
    "snail_instances_render_tiles": (_I, [_VP, _F13, _I, _I, _VP, _VP, _I, _VP, _I, _VP, _VP, _I, _VP, _VP, _VP]),
    "snail_instances_render_frame": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _VP, _I, _VP, _I, _VP]),
}

# include/snail_instances_build.h (the top-level tree rebuilt on the device; part of snail_instances.h): a table of its own once more --
# tests/c/instances_build_c.c enumerates it
INSTANCES_BUILD_SIGNATURES = {
    "snail_instances_rebuild_dev": (_I, [_VP, _VP, _VP, _I, _VP, _VP, _VP]),
    "snail_instances_read_tree": (_I, [_VP, _VP, _I, _VP, _VP, _VP, _I, _VP]),
}

# include/snail_bvh_fast.h: the reference's fast (binned) builder, on the host and on the device
BVH_FAST_SIGNATURES = {
    "snail_bvh_build_fast": (_I, [_VP, _I, _VP, _VP, _VP, _VP]),
    "snail_scene_create_fast_dev": (_VP, [_VP, _I, _I, _VP, _VP, _VP]),
    "snail_scene_rebuild_fast_dev": (_I, [_VP, _VP, _I, _VP, _VP, _VP]),
}

# include/snail_bvh_fast_batch.h: the fast builder over several device handles in one batched pass (tests/c/bvh_fast_batch_c.c enumerates this
# table and the next)
BVH_FAST_BATCH_SIGNATURES = {
    "snail_scenes_rebuild_fast_dev": (_I, [_VP, _I, _VP]),
}

# include/snail_wide.h: BVH::WideTrace with one ray per lane and the photon pass (tests/c/wide_c.c enumerates this table)
WIDE_SIGNATURES = {
    "snail_wide_trace_dev": (_I, [_VP, _I, _VP, _VP, _VP, _VP, _I, _VP, _I, _VP, _VP, _VP]),
    "snail_wide_trace": (_I, [_VP, _I, _VP, _VP, _VP, _VP, _I, _VP, _I, _VP, _VP]),
    "snail_photons_trace_dev": (_I, [_VP, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_photons_trace": (_I, [_VP, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
}

# include/snail_instances_materials_rebuild_all.h: the per-frame step of a deforming instanced scene in one call
INSTANCES_MATERIALS_REBUILD_ALL_SIGNATURES = {
    "snail_instances_materials_rebuild_all_dev": (_I, [_VP, _VP, _I, _VP, _VP, _I, _VP, _VP, _VP]),
}

# include/snail_heatmap.h: per-packet TreeStats and the gVals[5] heat-map of plain and instanced scenes (tests/c/heatmap_c.c enumerates this table)
HEATMAP_SIGNATURES = {
    "snail_packet_stats_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _I, _VP, _VP, _VP]),
    "snail_render_heat_packets_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _I, _VP, _VP, _VP, _VP]),
    "snail_render_heat_tiles": (_I, [_VP, _F13, _I, _I, _VP, _VP, _I, _VP, _I, _I, _VP, _VP]),
    "snail_render_heat_image": (_I, [_VP, _F13, _I, _I, _VP, _I, _I, _VP, _I, _VP]),
    "snail_instances_packet_stats_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _I, _VP, _VP, _VP]),
    "snail_instances_heat_packets_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _I, _VP, _VP, _VP, _VP, _VP]),
    "snail_instances_render_heat_tiles": (_I, [_VP, _F13, _I, _I, _VP, _VP, _I, _VP, _I, _I, _VP, _VP, _VP]),
    "snail_instances_render_heat_frame": (_I, [_VP, _F13, _I, _I, _VP, _I, _I, _VP, _I, _VP]),
}

# include/snail_materials.h: full shading of plain scenes (snail_amd/materials.py; tests/c/materials_c.c enumerates this table)
MATERIALS_SIGNATURES = {
    "snail_shtris_pack": (_I, [_VP, _VP, _VP, _VP, _I, _VP, _VP]),
    "snail_texture_size": (C.c_int64, [_I, _I, _VP]),
    "snail_texture_build": (_I, [_VP, _I, _I, _VP, C.c_int64, _VP]),
    "snail_materials_create": (_VP, [_VP, _VP, _I, _VP, _I, _VP, _I, _VP, _I]),
    "snail_materials_destroy": (None, [_VP]),
    "snail_materials_shade_packets_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_render_materials_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _VP, _I, _VP, _VP]),
    "snail_render_materials_packets_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _VP, _I, _VP, _VP, _VP]),
    "snail_render_materials_image": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _VP, _I, _VP]),
}

# include/snail_materials_bounce.h: the one mirrored bounce under full shading (tests/c/materials_bounce_c.c enumerates this table)
MATERIALS_BOUNCE_SIGNATURES = {
    "snail_materials_mirror_packets_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_materials_shade_rays_dev": (_I, [_VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_materials_bounce_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _VP, _I, _VP, _VP]),
    "snail_materials_bounce_packets_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _VP, _I, _VP, _VP, _VP]),
    "snail_materials_bounce_image": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _VP, _I, _VP]),
}

# include/snail_materials_tiles.h: the tile renderer of full-shaded plain scenes (tests/c/materials_tiles_c.c enumerates this table)
MATERIALS_TILES_SIGNATURES = {
    "snail_materials_frame_packets_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _VP, _I, _VP, _VP, _VP, _VP]),
    "snail_materials_render_tiles": (_I, [_VP, _F13, _I, _I, _VP, _VP, _I, _VP, _I, _VP, _I, _VP, _VP, _VP]),
    "snail_materials_render_frame": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _VP, _I, _VP]),
}

# include/snail_materials_transparency.h: the kinds that can select a transparent lane, their sample stages and the continuation generator
# (tests/c/materials_transparency_c.c enumerates this table)
MATERIALS_TRANSPARENCY_SIGNATURES = {
    "snail_materials_create_transparent": (_VP, [_VP, _VP, _I, _VP, _I, _VP, _I, _VP, _VP, _I]),
    "snail_materials_can_select_transparent": (_I, [_VP]),
    "snail_materials_shade_packets_transp_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_materials_shade_rays_transp_dev": (_I, [_VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_materials_continue_packets_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_materials_transparent_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _VP, _I, _I, _VP, _VP, _VP]),
    "snail_materials_transparent_packets_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _VP, _I, _VP, _I, _VP, _VP, _VP]),
    "snail_materials_transparent_image": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _VP, _I, _I, _VP, _VP]),
}

# include/snail_materials_tree.h: the transparency continuation together with the bounce, tiles, 4x AA and the tint (tests/c/materials_tree_c.c
# enumerates this table)
MATERIALS_TREE_SIGNATURES = {
    "snail_materials_mirror_rays_dev": (_I, [_VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_materials_tree_frame_packets_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _VP, _I, _VP, _VP, _I, _VP, _VP, _VP]),
    "snail_materials_tree_render_tiles": (_I, [_VP, _F13, _I, _I, _VP, _VP, _I, _VP, _I, _VP, _I, _VP, _VP, _I, _VP, _VP]),
    "snail_materials_tree_render_frame": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _VP, _I, _I, _VP, _VP]),
    "snail_materials_set_level_budget": (_I, [_VP, C.c_uint64]),
    "snail_materials_level_bytes": (C.c_int64, [_I, _I, _I]),
}

# include/snail_materials_heatmap.h: per-packet TreeStats and the gVals[5] heat-map under full shading (tests/c/materials_heat_c.c enumerates
# this table)
MATERIALS_HEAT_SIGNATURES = {
    "snail_materials_packet_stats_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _I, _I, _VP, _VP, _VP, _VP]),
    "snail_materials_heat_packets_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _I, _VP, _VP, _VP, _I, _VP, _VP, _VP]),
    "snail_materials_render_heat_tiles": (_I, [_VP, _F13, _I, _I, _VP, _VP, _I, _VP, _I, _I, _VP, _VP, _I, _VP, _VP]),
    "snail_materials_render_heat_frame": (_I, [_VP, _F13, _I, _I, _VP, _I, _I, _VP, _I, _I, _VP, _VP]),
}

# include/snail_materials_dynamic.h: a material set whose records are packed on the device and follow the scene's device rebuilds
# (tests/c/materials_dynamic_c.c enumerates this table)
MATERIALS_DYNAMIC_SIGNATURES = {
    "snail_materials_create_dev": (_VP, [_VP, _VP, _VP, _VP, _I, _VP, _VP, _VP, _VP, _I, _VP, _I, _VP, _VP, _I, _VP]),
    "snail_materials_rebuild_dev": (_I, [_VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_materials_update_dev": (_I, [_VP, _VP, _VP, _VP, _VP, _VP]),
}

# include/snail_instances_materials.h: full shading of instanced scenes (snail_amd/instances_materials.py; tests/c/instances_materials_c.c
# enumerates this table)
INSTANCES_MATERIALS_SIGNATURES = {
    "snail_instances_materials_create": (_VP, [_VP, _VP, _I, _VP, _I, _VP, _I]),
    "snail_instances_materials_destroy": (None, [_VP]),
    "snail_instances_materials_shade_packets_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_instances_render_materials_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _VP, _I, _VP, _VP]),
    "snail_instances_render_materials_packets_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _VP, _I, _VP, _VP, _VP]),
    "snail_instances_render_materials_image": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _VP, _I, _VP]),
}

# include/snail_instances_materials_bounce.h: the one mirrored bounce under full shading of instanced scenes
# (tests/c/instances_materials_bounce_c.c enumerates this table)
INSTANCES_MATERIALS_BOUNCE_SIGNATURES = {
    "snail_instances_materials_mirror_packets_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_instances_materials_shade_rays_dev": (_I, [_VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_instances_materials_bounce_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _VP, _I, _VP, _VP]),
    "snail_instances_materials_bounce_packets_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _VP, _I, _VP, _VP, _VP]),
    "snail_instances_materials_bounce_image": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _VP, _I, _VP]),
}

# include/snail_instances_materials_transparency.h: the transparency continuation under full shading of instanced scenes
# (tests/c/instances_materials_transparency_c.c enumerates this table)
INSTANCES_MATERIALS_TRANSPARENCY_SIGNATURES = {
    "snail_instances_materials_create_transparent": (_VP, [_VP, _VP, _I, _VP, _I, _VP, _VP, _I]),
    "snail_instances_materials_can_select_transparent": (_I, [_VP]),
    "snail_instances_materials_shade_packets_transp_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_instances_materials_shade_rays_transp_dev": (_I, [_VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_instances_materials_continue_packets_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_instances_materials_transparent_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _VP, _I, _I, _VP, _VP, _VP]),
    "snail_instances_materials_transparent_packets_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _VP, _I, _VP, _I, _VP, _VP, _VP]),
    "snail_instances_materials_transparent_image": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _VP, _I, _I, _VP, _VP]),
}

# include/snail_instances_materials_tree.h: the continuation together with the bounce, tiles, 4x AA and the tint under full shading of instanced
# scenes (tests/c/instances_materials_tree_c.c enumerates this table)
INSTANCES_MATERIALS_TREE_SIGNATURES = {
    "snail_instances_materials_mirror_rays_dev": (_I, [_VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "snail_instances_materials_tree_frame_packets_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _VP, _I, _VP, _VP, _I, _VP, _VP, _VP]),
    "snail_instances_materials_tree_render_tiles": (_I, [_VP, _F13, _I, _I, _VP, _VP, _I, _VP, _I, _VP, _I, _VP, _VP, _I, _VP, _VP]),
    "snail_instances_materials_tree_render_frame": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _VP, _I, _I, _VP, _VP]),
    "snail_instances_materials_set_level_budget": (_I, [_VP, C.c_uint64]),
    "snail_instances_materials_level_bytes": (C.c_int64, [_I, _I, _I]),
}

# include/snail_instances_materials_heatmap.h: per-packet TreeStats and the gVals[5] heat-map under full shading of instanced scenes
# (tests/c/instances_materials_heat_c.c enumerates this table)
INSTANCES_MATERIALS_HEAT_SIGNATURES = {
    "snail_instances_materials_packet_stats_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _I, _I, _VP, _VP, _VP, _VP]),
    "snail_instances_materials_heat_packets_dev": (_I, [_VP, _F13, _I, _I, _VP, _I, _VP, _I, _I, _VP, _VP, _VP, _I, _VP, _VP, _VP]),
    "snail_instances_materials_render_heat_tiles": (_I, [_VP, _F13, _I, _I, _VP, _VP, _I, _VP, _I, _I, _VP, _VP, _I, _VP, _VP]),
    "snail_instances_materials_render_heat_frame": (_I, [_VP, _F13, _I, _I, _VP, _I, _I, _VP, _I, _I, _VP, _VP]),
}

# include/snail_instances_materials_dynamic.h: an instanced set whose BLASes deform on the device -- per-BLAS records packed on the device and packed
# again behind every rebuild of a BLAS (tests/c/instances_materials_dynamic_c.c enumerates this table)
INSTANCES_MATERIALS_DYNAMIC_SIGNATURES = {
    "snail_instances_materials_create_dev": (_VP, [_VP, _VP, _I, _VP, _I, _VP, _VP, _I, _VP]),
    "snail_instances_materials_rebuild_dev": (_I, [_VP, _VP, _I, _VP]),
    "snail_instances_materials_update_dev": (_I, [_VP, _VP, _I, _VP]),
}

# include/snail_hip_debug.h: the workbench build only (libsnailhip_debug.so, -DSNAIL_DEBUG_API)
DEBUG_SIGNATURES = {
    "snail_debug_delay_dev": (_I, [C.c_float, _VP]),
    "snail_debug_clock_dev": (_I, [C.c_float, _VP, _VP]),
    "snail_debug_recip_check": (_I, [_VP]),
    "snail_debug_dispatch_rate": (_I, [_I, _I, _I, _VP]),
    "snail_debug_hostsse_device_check": (_I, [_I, _I, _VP, _VP]),
    "snail_debug_occupancy": (_I, [_VP]),
    "snail_debug_anyorder": (_I, [_VP, _F13, _I, _I, _I, _I, _VP]),
    "snail_debug_rel_flag_count": (_I, [_VP, _VP, _VP]),
    "snail_debug_rel_axis_flag_count": (_I, [_VP, _VP, _VP]),
}
DEBUG_LIB_PATH = os.path.join(HERE, "libsnailhip_debug.so")
_dbg = None


def debug_lib():
    """The workbench build of the same sources: the product C-ABI + include/snail_hip_debug.h + the SNAIL_DEBUG_* environment switches.
    For tests and tools only; nothing on a product path loads it."""
    global _dbg
    if _dbg is None:
        if not os.path.exists(DEBUG_LIB_PATH):
            raise SnailError("workbench library %s is missing: `make -C snail_amd/csrc debug`" % DEBUG_LIB_PATH)
        L = C.CDLL(DEBUG_LIB_PATH)
        for table in (SIGNATURES, INSTANCES_SIGNATURES, INSTANCES_SHADE_SIGNATURES, INSTANCES_TILES_SIGNATURES, INSTANCES_BUILD_SIGNATURES, BVH_FAST_SIGNATURES, HEATMAP_SIGNATURES, MATERIALS_SIGNATURES, MATERIALS_BOUNCE_SIGNATURES, MATERIALS_TILES_SIGNATURES, MATERIALS_TRANSPARENCY_SIGNATURES, MATERIALS_TREE_SIGNATURES, MATERIALS_HEAT_SIGNATURES, MATERIALS_DYNAMIC_SIGNATURES, INSTANCES_MATERIALS_SIGNATURES, INSTANCES_MATERIALS_BOUNCE_SIGNATURES, INSTANCES_MATERIALS_TRANSPARENCY_SIGNATURES, INSTANCES_MATERIALS_TREE_SIGNATURES, INSTANCES_MATERIALS_HEAT_SIGNATURES, INSTANCES_MATERIALS_DYNAMIC_SIGNATURES, BVH_FAST_BATCH_SIGNATURES, INSTANCES_MATERIALS_REBUILD_ALL_SIGNATURES, WIDE_SIGNATURES, DEBUG_SIGNATURES):
            for name, (res, args) in table.items():
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
        _dbg = L
    return _dbg


def lib():
    """Load libsnailhip.so or fail loudly."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SnailError(
                "HIP extension %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C snail_amd/csrc`). There is no CPU fallback." % LIB_PATH)
        try:
            L = C.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover - depends on the box
            raise SnailError("cannot load %s: %s" % (LIB_PATH, e)) from e
        for table in (SIGNATURES, INSTANCES_SIGNATURES, INSTANCES_SHADE_SIGNATURES, INSTANCES_TILES_SIGNATURES, INSTANCES_BUILD_SIGNATURES, BVH_FAST_SIGNATURES, HEATMAP_SIGNATURES, MATERIALS_SIGNATURES, MATERIALS_BOUNCE_SIGNATURES, MATERIALS_TILES_SIGNATURES, MATERIALS_TRANSPARENCY_SIGNATURES, MATERIALS_TREE_SIGNATURES, MATERIALS_HEAT_SIGNATURES, MATERIALS_DYNAMIC_SIGNATURES, INSTANCES_MATERIALS_SIGNATURES, INSTANCES_MATERIALS_BOUNCE_SIGNATURES, INSTANCES_MATERIALS_TRANSPARENCY_SIGNATURES, INSTANCES_MATERIALS_TREE_SIGNATURES, INSTANCES_MATERIALS_HEAT_SIGNATURES, INSTANCES_MATERIALS_DYNAMIC_SIGNATURES, BVH_FAST_BATCH_SIGNATURES, INSTANCES_MATERIALS_REBUILD_ALL_SIGNATURES, WIDE_SIGNATURES):
            for name, (res, args) in table.items():
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
        for name, (res, args) in DEBUG_SIGNATURES.items():     # present only when SNAIL_LIB_PATH names the workbench build
            fn = getattr(L, name, None)
            if fn is not None:
                fn.restype = res
                fn.argtypes = args
        _lib = L
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().snail_last_error()
        raise SnailError("%s failed (status %d): %s" % (what, rc, msg.decode() if msg else "?"))


def ptr(a):
    """Device/host address of a numpy array, torch tensor, or None."""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    return a.ctypes.data_as(C.c_void_p)
