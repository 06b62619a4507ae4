"""kanter_core_amd -- MI355X (gfx950) per-pixel evaluation backend for kanter_core / vismut_core
graphs.  The product is libkanter_core_amd.so (C ABI: include/kanter_core_amd.h, hand-written HIP
kernels in csrc/*.hip); this package mirrors the reference's host API on top of it.
Build the library with `python -m kanter_core_amd.build`; importing `api` symbols that touch the
device fails loudly when it is missing -- there is no CPU fallback.
"""
from .api import (Edge, EmbeddedSlotDataId, LiveGraph, MixType, Node, NodeGraph, NodeId, NodeState, NodeType,  # noqa: F401
                  ResizeFilter, ResizePolicy, Side, Size, SlotData, SlotId, SlotImage, TexProError,
                  TextureProcessor, calculate_size, combine_rgba_process, get_stream, height_to_normal_process,
                  init, is_initialized, mix_process, resize_image, separate_rgba_process, set_fusion, set_stream,
                  shutdown, stats, sync, value_process, set_specialize, get_specialize, specialize_wait,
                  specialize_stats, specialize_compile_check, Partition, PartitionPolicy, NodeKind, set_resize_mode,
                  get_resize_mode, resize_upsample_plan, resize_down2_plan, stats_counter, specialize_compile_check_upsample, specialize_compile_check_mask, set_chain_quads, get_chain_quads, set_pack_sources, get_pack_sources, set_pack_budget_mb, get_pack_budget_mb, set_cache_policy, get_cache_policy, set_option, get_option, comm_unique_id, comm_init,
                  comm_destroy, comm_info, comm_stats, comm_transport, comm_gather_bands, PlanKind, pool_trim, kernel_cache_set_dir, kernel_cache_stats,
                  kernel_cache_precompile, specialize_reset, U8Pipe, device_image_desc, DEVICE_SRGB, DEVICE_GRAY,
                  ChannelStats, STATS_HISTOGRAM, STATS_SRGB, BC_SRGB, BC6H, BC7, BC_BLOCK_BYTES, BC_PUNCH_THROUGH, bc_punch_through_ref, bc1_punch_through_block,
                  MIP_PER_LEVEL, MIP_NORMALS, MIP_COVERAGE, MIP_ALPHA_WEIGHT, mip_alpha_weight, mip_alpha_texel, mip_coverage_ref, MipCoverageLevel, alpha_ref_threshold, mip_coverage_target, mip_coverage_scale, mip_normal_texel, mip_unit_normal, mip_roughness_texel, levels_to_bc_mips, write_dds_levels, mip_level_count, bc_mip_layout, dds_header, BC_GRAY, BC_ALL_MODES, BcError, DdsInfo, dds_parse, preview_level,
                  PREVIEW_SRGB, PreviewPlan, preview_plan, previews, previews_torch, SDF_WRAP, SDF_MAX_SPREAD, sdf_cap, sdf_texel,
                  BLUR_WRAP, BLUR_MAX_RADIUS, blur_weights, blur_texel)

__all__ = [n for n in dir() if not n.startswith("_")]
