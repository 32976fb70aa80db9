"""ctypes binding of libmydet_hip.so (C ABI declared in include/mydet.h).

The library is the product: there is no CPU or PyTorch fallback.  If it is missing
the import of any op fails loudly with instructions to build it.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# MYDET_LIB_PATH: a differently built copy of the library (kernel experiments: tools/ablate_sepconv.sh); default = the in-tree build
LIB_PATH = os.environ.get('MYDET_LIB_PATH') or os.path.join(_HERE, 'lib', 'libmydet_hip.so')

c_int, c_i64, c_f32, c_f64, c_ptr = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_void_p

# name -> argtypes, exactly the prototypes of include/mydet.h
SIGNATURES = {
    'mydet_abi_version': [],
    'mydet_conv2d_igemm_f32': [c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_ptr, c_i64, c_ptr, c_i64]
    + [c_int] * 13 + [c_ptr],
    'mydet_wino_weights_floats': [c_int, c_int],
    'mydet_wino_weights_f32': [c_ptr, c_int, c_int, c_ptr, c_ptr],
    'mydet_conv2d_wino_f32': [c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64] + [c_int] * 6
    + [c_ptr],
    'mydet_wino_plan': [c_int] * 5 + [c_i64, c_int, c_ptr],
    'mydet_wino4_weights_floats': [c_int, c_int],
    'mydet_wino4_weights_f32': [c_ptr, c_int, c_int, c_ptr, c_ptr],
    'mydet_wino4_workspace_bytes': [c_int, c_int, c_int, c_int, c_int],
    'mydet_wino4_reload_tuning': [],
    'mydet_conv_b3_reload_tuning': [],
    'mydet_conv_igemm_occupancy': [c_int, c_ptr],
    'mydet_conv_igemm_plan': [c_int] * 7 + [c_i64, c_int, c_ptr],
    'mydet_conv_b3_plan': [c_int] * 7 + [c_i64, c_int, c_ptr],
    'mydet_split_bf16_elems': [c_int, c_int],
    'mydet_split_bf16_f32': [c_ptr, c_int, c_int, c_ptr, c_ptr],
    'mydet_conv2d_igemm_b3_f32': [c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_ptr, c_i64, c_ptr, c_i64] + [c_int] * 13 + [c_ptr],
    'mydet_conv3x3_p3_f32': [c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_i64] + [c_int] * 7 + [c_ptr],
    'mydet_conv3x3_p3_plan': [c_int, c_int, c_int, c_int, c_ptr],
    'mydet_conv_stem_p3_f32': [c_ptr, c_i64, c_i64, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_int, c_ptr, c_ptr, c_ptr, c_int, c_ptr, c_i64]
    + [c_int] * 11 + [c_ptr],
    'mydet_conv_stem_p3_lds_bytes': [],
    'mydet_wino4_tail_plan': [c_int, c_int, c_int, c_int, c_int, c_int, c_ptr],
    'mydet_conv2d_wino4_f32': [c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64] + [c_int] * 6 + [c_ptr],
    'mydet_dwconv_slices': [c_int, c_int, c_int, c_int, c_int],
    'mydet_dwconv_se_groups': [c_int, c_int, c_int, c_int, c_int],
    'mydet_dwconv_f32': [c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_i64] + [c_int] * 11 + [c_ptr, c_int, c_ptr, c_ptr],
    'mydet_channel_sums_f32': [c_ptr, c_i64, c_int, c_int, c_int, c_int, c_ptr, c_int, c_ptr],
    'mydet_se_gate_f32': [c_ptr, c_int, c_int, c_int, c_int, c_ptr, c_ptr, c_int, c_ptr, c_ptr, c_ptr, c_ptr],
    'mydet_maxpool3s2_f32': [c_ptr, c_i64, c_ptr, c_i64] + [c_int] * 6 + [c_ptr],
    'mydet_bifpn_fuse_f32': [c_int, c_ptr, c_i64, c_int, c_ptr, c_i64, c_int, c_ptr, c_i64, c_int, c_ptr, c_ptr, c_i64,
                             c_int, c_int, c_int, c_int, c_ptr],
    'mydet_conv2d_stem_f32': [c_ptr, c_i64, c_i64, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_i64] + [c_int] * 10 + [c_ptr],
    'mydet_upsample_concat_f32': [c_ptr, c_i64, c_int, c_int, c_int, c_ptr, c_i64, c_int, c_ptr, c_i64, c_int, c_int,
                                  c_int, c_ptr],
    'mydet_conv1x1_upcat_f32': [c_ptr, c_i64, c_int, c_ptr, c_i64, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_i64]
    + [c_int] * 5 + [c_ptr],
    'mydet_space_to_depth_f32': [c_ptr, c_i64, c_i64, c_i64, c_i64, c_ptr, c_i64, c_int, c_int, c_int, c_int, c_ptr],
    'mydet_spp_concat_f32': [c_ptr, c_i64, c_ptr, c_i64] + [c_int] * 7 + [c_ptr],
    'mydet_decode_levels_f32': [c_int, c_int, c_ptr, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                c_ptr, c_ptr, c_ptr, c_i64, c_ptr],
    'mydet_decode_uv5_levels_f32': [c_int, c_ptr, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                    c_ptr, c_ptr, c_ptr, c_i64, c_ptr],
    'mydet_decode_f32': [c_int, c_ptr, c_i64, c_int, c_int, c_ptr, c_i64, c_int, c_int, c_int, c_ptr, c_int, c_int,
                         c_int, c_int, c_int, c_f32, c_int, c_int, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_ptr],
    'mydet_postprocess_f32': [c_ptr, c_ptr, c_ptr, c_int, c_i64, c_f32, c_f64, c_int, c_ptr, c_ptr, c_ptr, c_ptr,
                              c_ptr, c_ptr, c_ptr],
    'mydet_postprocess_records_f32': [c_ptr, c_ptr, c_ptr, c_int, c_i64, c_f32, c_f64, c_ptr, c_ptr, c_ptr],
    'mydet_postprocess_rot_f32': [c_ptr, c_ptr, c_ptr, c_int, c_i64, c_f32, c_f64, c_int, c_ptr, c_ptr, c_ptr, c_ptr,
                                  c_ptr, c_ptr, c_ptr],
    'mydet_postprocess_records_rot_f32': [c_ptr, c_ptr, c_ptr, c_int, c_i64, c_f32, c_f64, c_ptr, c_ptr, c_ptr],
    'mydet_postprocess_rotnms_f32': [c_ptr, c_ptr, c_ptr, c_int, c_i64, c_f32, c_f64, c_int, c_ptr, c_ptr, c_ptr, c_ptr,
                                     c_ptr, c_ptr, c_ptr],
    'mydet_postprocess_records_rotnms_f32': [c_ptr, c_ptr, c_ptr, c_int, c_i64, c_f32, c_f64, c_ptr, c_ptr, c_ptr],
    'mydet_postprocess_nms_f32': [c_ptr, c_ptr, c_ptr, c_int, c_i64, c_f32, c_f64, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr,
                                  c_ptr, c_ptr, c_ptr],
    'mydet_postprocess_records_nms_f32': [c_ptr, c_ptr, c_ptr, c_int, c_i64, c_f32, c_f64, c_ptr, c_ptr, c_ptr, c_ptr],
    'mydet_postprocess_rot_nms_f32': [c_ptr, c_ptr, c_ptr, c_int, c_i64, c_f32, c_f64, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr,
                                      c_ptr, c_ptr, c_ptr],
    'mydet_postprocess_records_rot_nms_f32': [c_ptr, c_ptr, c_ptr, c_int, c_i64, c_f32, c_f64, c_ptr, c_ptr, c_ptr, c_ptr],
    'mydet_rotated_iou_f32': [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_ptr],
    'mydet_merge_tile_records_scratch_bytes': [c_int, c_int, c_int],
    'mydet_merge_tile_records_f32': [c_ptr, c_i64, c_i64, c_int, c_int, c_int, c_ptr, c_f64, c_int, c_int, c_ptr, c_ptr, c_i64, c_ptr],
    'mydet_merge_tile_records_nms_f32': [c_ptr, c_i64, c_i64, c_int, c_int, c_int, c_ptr, c_f64, c_int, c_int, c_int, c_ptr, c_ptr, c_i64,
                                         c_ptr],
    'mydet_fuse_view_records_scratch_bytes': [c_int, c_int, c_int, c_int],
    'mydet_fuse_view_records_f32': [c_ptr, c_i64, c_i64, c_int, c_int, c_int, c_ptr, c_int, c_int, c_f64, c_ptr, c_ptr, c_ptr, c_i64, c_ptr],
    'mydet_track_state_words': [c_int],
    'mydet_track_reset': [c_ptr, c_int, c_int, c_ptr],
    'mydet_track_frames_f32': [c_ptr, c_i64, c_i64, c_int, c_int, c_int, c_ptr, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr],
    'mydet_track_frames_assoc_f32': [c_ptr, c_i64, c_i64, c_int, c_int, c_int, c_ptr, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr,
                                     c_ptr, c_ptr],
    'mydet_track_frames_motion_f32': [c_ptr, c_i64, c_i64, c_int, c_int, c_int, c_ptr, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr,
                                      c_ptr, c_ptr, c_ptr],
    'mydet_track_frames_warp_f32': [c_ptr, c_i64, c_i64, c_int, c_int, c_int, c_ptr, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr,
                                    c_ptr, c_ptr, c_ptr],
    'mydet_track_appear_state_words': [c_int],
    'mydet_track_frames_appear_f32': [c_ptr, c_i64, c_i64, c_int, c_int, c_int, c_ptr, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr,
                                      c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr],
    'mydet_track_frames_appear_warp_f32': [c_ptr, c_i64, c_i64, c_int, c_int, c_int, c_ptr, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr,
                                           c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr],
    'mydet_track_appear_ws_words': [c_int],
    'mydet_track_frames_appear_optimal_f32': [c_ptr, c_i64, c_i64, c_int, c_int, c_int, c_ptr, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr,
                                              c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_ptr, c_ptr],
    'mydet_track_frames_appear_optimal_warp_f32': [c_ptr, c_i64, c_i64, c_int, c_int, c_int, c_ptr, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr,
                                                   c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_ptr, c_ptr],
    'mydet_appear_boxes_rgb_u8': [c_ptr, c_int, c_int, c_int, c_i64, c_i64, c_ptr, c_ptr, c_i64, c_ptr],
    'mydet_appear_boxes_yuv420': [c_ptr, c_int, c_int, c_int, c_ptr, c_ptr, c_i64, c_ptr],
    'mydet_motion_default_reduce': [c_int, c_int],
    'mydet_motion_state_words': [c_int, c_int, c_int, c_int],
    'mydet_motion_workspace_bytes': [c_int, c_int, c_int, c_int, c_int],
    'mydet_motion_reset': [c_ptr, c_int, c_int, c_int, c_int, c_int, c_ptr],
    'mydet_motion_frames_rgb_u8': [c_ptr, c_int, c_int, c_int, c_i64, c_i64, c_int, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_ptr, c_ptr],
    'mydet_motion_frames_yuv420': [c_ptr, c_int, c_int, c_int, c_int, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_ptr, c_ptr],
    'mydet_motion_warp_frames_rgb_u8': [c_ptr, c_int, c_int, c_int, c_i64, c_i64, c_int, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr,
                                        c_ptr],
    'mydet_motion_warp_frames_yuv420': [c_ptr, c_int, c_int, c_int, c_int, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr],
    'mydet_carry_state_words': [],
    'mydet_carry_reset': [c_ptr, c_int, c_ptr],
    'mydet_carry_records_rgb_u8': [c_ptr, c_int, c_int, c_int, c_i64, c_i64, c_int, c_ptr, c_int, c_ptr, c_i64, c_int, c_ptr, c_ptr, c_ptr, c_ptr,
                                   c_ptr, c_ptr, c_ptr, c_ptr],
    'mydet_carry_records_yuv420': [c_ptr, c_int, c_int, c_int, c_int, c_ptr, c_int, c_ptr, c_i64, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr,
                                   c_ptr, c_ptr],
    'mydet_zones_state_words': [c_int],
    'mydet_zones_reset': [c_ptr, c_int, c_int, c_ptr],
    'mydet_zones_frames': [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_int, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr,
                           c_ptr],
    'mydet_trails_state_words': [c_int, c_int],
    'mydet_trails_reset': [c_ptr, c_int, c_int, c_int, c_ptr],
    'mydet_trails_frames': [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_int, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr],
    'mydet_draw_overlay_rgb_u8': [c_ptr, c_int, c_int, c_int, c_i64, c_i64, c_ptr, c_ptr, c_ptr],
    'mydet_draw_overlay_yuv420_u8': [c_ptr, c_int, c_int, c_int, c_ptr, c_ptr, c_ptr],
    'mydet_mbconv_tiles': [c_int, c_int, c_int],
    'mydet_mbconv_expand_dw_f32': [c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64] + [c_int] * 11 + [c_ptr, c_int, c_ptr, c_ptr],
    'mydet_sepconv_nodes_f32': [c_int, c_ptr, c_int, c_int, c_ptr],
    'mydet_stem_dw_f32': [c_ptr, c_i64, c_i64, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_int,
                          c_int, c_int, c_int, c_int, c_ptr, c_int, c_ptr, c_ptr],
    'mydet_lr_tb_levels_f32': [c_int, c_ptr, c_int, c_int, c_ptr],
    'mydet_sepconv_decode_retina_f32': [c_int, c_ptr, c_int, c_int, c_int, c_int, c_int, c_int, c_ptr, c_ptr, c_ptr, c_i64, c_ptr],
    'mydet_bboxes_iou_f32': [c_ptr, c_int, c_ptr, c_int, c_int, c_ptr, c_ptr],
    'mydet_bboxes_to_original_batched_f32': [c_ptr, c_i64, c_ptr, c_i64, c_int, c_int, c_ptr, c_ptr],
    'mydet_detections_to_json_f64': [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_int, c_int, c_ptr, c_int, c_ptr, c_ptr, c_ptr],
    'mydet_resize_bilinear_u8': [c_ptr, c_int, c_int, c_i64, c_ptr, c_int, c_int, c_i64, c_ptr, c_ptr, c_int, c_ptr, c_ptr, c_int, c_ptr],
    'mydet_preprocess_u8_f32': [c_ptr, c_int, c_int, c_int, c_ptr, c_int, c_int, c_int, c_ptr, c_ptr, c_ptr],
    'mydet_frames_to_input_f32': [c_ptr, c_int, c_int, c_int, c_i64, c_i64, c_ptr, c_int, c_int, c_int, c_int, c_int, c_int,
                                  c_ptr, c_ptr, c_int, c_ptr, c_ptr, c_int, c_int, c_ptr, c_ptr, c_ptr],
    'mydet_frames_to_input_flip_f32': [c_ptr, c_int, c_int, c_int, c_i64, c_i64, c_ptr, c_int, c_int, c_int, c_int, c_int, c_int,
                                       c_ptr, c_ptr, c_int, c_ptr, c_ptr, c_int, c_int, c_ptr, c_ptr, c_int, c_ptr],
    'mydet_nv12_to_rgb_u8': [c_ptr, c_i64, c_i64, c_ptr, c_i64, c_i64, c_int, c_int, c_int, c_ptr, c_i64, c_i64, c_int, c_int, c_ptr],
    'mydet_nv12_to_input_f32': [c_ptr, c_i64, c_i64, c_ptr, c_i64, c_i64, c_int, c_int, c_int, c_int, c_int,
                                c_ptr, c_int, c_int, c_int, c_int, c_int, c_int,
                                c_ptr, c_ptr, c_int, c_ptr, c_ptr, c_int, c_int, c_ptr, c_ptr, c_ptr],
    'mydet_yuv420_to_rgb_u8': [c_ptr, c_int, c_int, c_int, c_ptr, c_i64, c_i64, c_ptr],
    'mydet_yuv420_to_input_f32': [c_ptr, c_int, c_int, c_int,
                                  c_ptr, c_int, c_int, c_int, c_int, c_int, c_int,
                                  c_ptr, c_ptr, c_int, c_ptr, c_ptr, c_int, c_int, c_ptr, c_ptr, c_ptr],
    'mydet_yuv420_to_input_flip_f32': [c_ptr, c_int, c_int, c_int,
                                       c_ptr, c_int, c_int, c_int, c_int, c_int, c_int,
                                       c_ptr, c_ptr, c_int, c_ptr, c_ptr, c_int, c_int, c_ptr, c_ptr, c_int, c_ptr],
    'mydet_draw_boxes_rgb_u8': [c_ptr, c_int, c_int, c_int, c_i64, c_i64, c_ptr, c_ptr, c_ptr],
    'mydet_draw_boxes_yuv420_u8': [c_ptr, c_int, c_int, c_int, c_ptr, c_ptr, c_ptr],
    'mydet_redact_workspace_bytes': [c_int, c_int, c_int, c_int],
    'mydet_redact_boxes_rgb_u8': [c_ptr, c_int, c_int, c_int, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_ptr],
    'mydet_redact_boxes_yuv420_u8': [c_ptr, c_int, c_int, c_int, c_ptr, c_ptr, c_ptr, c_ptr],
    'mydet_crop_boxes_rgb': [c_ptr, c_int, c_int, c_int, c_i64, c_i64, c_ptr, c_ptr, c_ptr],
    'mydet_crop_boxes_yuv420': [c_ptr, c_int, c_int, c_int, c_ptr, c_ptr, c_ptr],
    'mydet_eval_ious_f64': [c_ptr, c_ptr, c_ptr],
    'mydet_eval_match_f64': [c_ptr, c_ptr, c_ptr, c_int, c_ptr, c_int, c_ptr, c_ptr, c_ptr, c_ptr],
    'mydet_eval_accumulate_f64': [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_ptr, c_int, c_ptr, c_int, c_ptr, c_int, c_ptr, c_ptr,
                                  c_ptr, c_ptr],
    'mydet_mot_clear_f64': [c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr],
    'mydet_mot_scratch_bytes': [c_ptr, c_int],
    'mydet_mot_id_overlap': [c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_ptr, c_i64, c_ptr],
    'mydet_mot_id_assign': [c_ptr, c_ptr, c_int, c_ptr, c_i64, c_ptr, c_ptr],
    'mydet_hota_align_f64': [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr],
    'mydet_hota_match': [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr],
    'mydet_hota_score_f64': [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr],
    'mydet_cxcywh_to_x1y1x2y2_f32': [c_ptr, c_ptr, c_i64, c_int, c_ptr],
    'mydet_bboxes_to_original_f32': [c_ptr, c_i64, c_f32, c_f32, c_f32, c_f32, c_f32, c_f32, c_ptr],
}



RETURNS_I64 = {'mydet_wino_weights_floats', 'mydet_wino4_weights_floats', 'mydet_wino4_workspace_bytes', 'mydet_split_bf16_elems',
               'mydet_merge_tile_records_scratch_bytes', 'mydet_fuse_view_records_scratch_bytes', 'mydet_track_state_words', 'mydet_mot_scratch_bytes', 'mydet_zones_state_words',
               'mydet_redact_workspace_bytes', 'mydet_trails_state_words', 'mydet_motion_state_words', 'mydet_motion_workspace_bytes',
               'mydet_track_appear_state_words', 'mydet_carry_state_words', 'mydet_track_appear_ws_words'}

# detection record layout (MYDET_REC_* of include/mydet.h), in int32 words
REC_TOPK = 512
REC_COUNT, REC_BBOX = 0, 4
REC_SCORE = REC_BBOX + 4 * REC_TOPK
REC_CLASS = REC_SCORE + REC_TOPK
REC_INDEX = REC_CLASS + 2 * REC_TOPK
REC_WORDS = REC_INDEX + REC_TOPK
# rotated record (bb_format 'cxcywhd'): the same fields at the same offsets + one angle plane behind them
REC_ANGLE = REC_WORDS
REC_ROT_WORDS = REC_WORDS + REC_TOPK
# merge of tile records (mydet_merge_tile_records_f32): MYDET_TILES_MAX windows per frame, MYDET_MERGE_* pair tests
TILES_MAX = 64
MERGE_IOU, MERGE_IOS = 0, 1
# mirrored views and their fusion (mydet_*_to_input_flip_f32, mydet_fuse_view_records_f32): MYDET_VIEW_*, MYDET_VIEWS_MAX, MYDET_FUSE_*
VIEW_HFLIP, VIEW_VFLIP = 1, 2
VIEWS_MAX = 8
FUSE_NMS, FUSE_WBF = 0, 1
# NMS modes (mydet_postprocess_*nms_f32): MYDET_NMS_* of include/mydet.h
NMS_HARD, NMS_SOFT_LINEAR, NMS_SOFT_GAUSSIAN, NMS_MERGE = range(4)
# tracking (mydet_track_frames_f32): MYDET_TRACK_* of include/mydet.h
TRACK_MAX_TRACKS = 512
TRACK_STATE_HEADER, TRACK_SLOT_WORDS = 8, 31
TRACK_MATCH_IOU, TRACK_MATCH_ROTATED = 0, 1
TRACK_ASSIGN_GREEDY, TRACK_ASSIGN_OPTIMAL = 0, 1
# appearance (mydet_appear_boxes_*, mydet_track_frames_appear_f32): MYDET_APPEAR_* of include/mydet.h
APPEAR_BINS, APPEAR_SAMPLES, APPEAR_SIM_MAX = 128, 512, 131072
# zones and lines (mydet_zones_frames): MYDET_ZONE* of include/mydet.h
ZONES_MAX, ZONE_MAX_VERTICES, ZONE_MAX_CLASSES, ZONE_MAX_HEAT, ZONE_MAX_FRAME, ZONE_COORD_MAX = 16, 16, 16, 1024, 32768, 1 << 20
ZONE_ANCHOR_CENTER, ZONE_ANCHOR_BOTTOM = 0, 1
ZONES_STATE_HEADER, ZONES_SLOT_WORDS = 148, 22
# camera motion (mydet_motion_frames_*): MYDET_MOTION_* of include/mydet.h
MOTION_MIN_SEARCH, MOTION_MAX_SEARCH, MOTION_MAX_BLOCKS, MOTION_STATE_HEADER = 4, 16, 1024, 4
MOTION_MODEL_SHIFT, MOTION_MODEL_SIMILARITY = 0, 1
# key frames (mydet_carry_records_*): MYDET_CARRY_* of include/mydet.h
CARRY_SLOTS, CARRY_SLOT_HEADER, CARRY_SLOT_WORDS, CARRY_MAX_EVERY = 512, 16, 336, 16
CARRY_HOW_NONE, CARRY_HOW_KEY, CARRY_HOW_CARRIED, CARRY_HOW_FLAT, CARRY_HOW_LOST, CARRY_HOW_LEFT, CARRY_HOW_NOT = range(7)
# overlay renderer (mydet_draw_boxes_*): MYDET_DRAW_* of include/mydet.h
DRAW_MAX_BOXES, DRAW_MAX_THICKNESS, DRAW_MAX_GLYPHS, DRAW_NAME_BYTES = 512, 64, 33, 16
DRAW_COLOR_CLASS, DRAW_COLOR_ID, DRAW_COLOR_FIXED = 0, 1, 2
DRAW_LABEL_CLASS, DRAW_LABEL_SCORE, DRAW_LABEL_ID = 1, 2, 4
# counting overlay and trails (mydet_draw_overlay_*, mydet_trails_frames): MYDET_OVERLAY_*, MYDET_TRAIL_MAX_POINTS of include/mydet.h
OVERLAY_MAX_GLYPHS, TRAIL_MAX_POINTS = 40, 32
OVERLAY_ZONES, OVERLAY_LINES, OVERLAY_TRAILS = 1, 2, 4
OVERLAY_COUNT_OCCUPANCY, OVERLAY_COUNT_ENTRIES, OVERLAY_COUNT_VISITS = 1, 2, 4
# redaction (mydet_redact_boxes_*): MYDET_REDACT_* of include/mydet.h
REDACT_MOSAIC, REDACT_SMOOTH, REDACT_SOLID = 0, 1, 2
REDACT_BOX, REDACT_ELLIPSE = 0, 1
REDACT_MIN_CELL, REDACT_MAX_CELL, REDACT_MAX_CLASSES = 4, 64, 16
# object chips (mydet_crop_boxes_*): MYDET_CROP_* of include/mydet.h
CROP_MAX_SIDE, CROP_MAX_SLOTS = 256, 512
CROP_U8, CROP_F32 = 0, 1
# scoring (mydet_eval_*): MYDET_EVAL_* of include/mydet.h
EVAL_MAX_GT, EVAL_MAX_DT, EVAL_MAX_THRS, EVAL_MAX_AREAS, EVAL_MAX_DETS, EVAL_MAX_RECS = 1024, 1024, 32, 8, 8, 128
EVAL_GT_IGNORE, EVAL_GT_CROWD = 1, 2
# track scoring (mydet_mot_*): MYDET_MOT_MAX_IDS of include/mydet.h
MOT_MAX_IDS = 1024
# HOTA (mydet_hota_*): the frame bound of include/mydet.h, and the fixed-point units of a potential and of a pair score
HOTA_MAX_FRAMES, HOTA_P_ONE, HOTA_Q_ONE = 1 << 22, 1 << 30, 1 << 20


class DecodeLevel(ctypes.Structure):
    """mydet_decode_level (include/mydet.h)."""
    _fields_ = [('box', c_ptr), ('ldbox', c_i64), ('cls', c_ptr), ('ldcls', c_i64), ('anchors_wh', c_ptr),
                ('H', c_int), ('W', c_int), ('stride', c_f32), ('n_off', c_i64)]


class NmsMode(ctypes.Structure):
    """mydet_nms_mode (include/mydet.h)."""
    _fields_ = [('kind', c_int), ('agnostic', c_int), ('sigma', c_f64), ('min_score', c_f32), ('reserved', c_int)]


class FuseMode(ctypes.Structure):
    """mydet_fuse_mode (include/mydet.h)."""
    _fields_ = [('kind', c_int), ('metric', c_int), ('rotated_nms', c_int), ('agnostic', c_int), ('min_score', c_f32), ('reserved', c_int)]


class SeTail(ctypes.Structure):
    """mydet_se_tail (include/mydet.h): the squeeze-excite tail finished inside the depthwise launch."""
    _fields_ = [('w1', c_ptr), ('b1', c_ptr), ('w2t', c_ptr), ('b2', c_ptr), ('gate', c_ptr), ('hpart', c_ptr), ('Cse', c_int),
                ('hpart_bytes', c_i64)]


SE_EPOCH_WORDS = 1024               # MYDET_SE_EPOCH_WORDS of include/mydet.h
ABI_VERSION = 2                     # MYDET_ABI_VERSION of include/mydet.h (2: mydet_se_tail.hpart_bytes, mydet_conv3x3_p3_f32)


class SepconvNode(ctypes.Structure):
    """mydet_sepconv_node (include/mydet.h)."""
    _fields_ = [('inp', c_ptr * 3), ('ld', c_i64 * 3), ('mode', c_int * 3), ('n_in', c_int), ('fuse_weights', c_ptr),
                ('w_dw', c_ptr), ('w_pw_packed', c_ptr), ('scale', c_ptr), ('shift', c_ptr), ('y', c_ptr), ('ldy', c_i64),
                ('H', c_int), ('W', c_int), ('Cout', c_int), ('act', c_int)]


class SepconvDecodeNode(ctypes.Structure):
    """mydet_sepconv_decode_node (include/mydet.h)."""
    _fields_ = [('node', SepconvNode), ('kind', c_int), ('stride', c_f32), ('anchors_wh', c_ptr), ('n_off', c_i64)]


SEPCONV_MAX_NODES = 10


class LrTbLevel(ctypes.Structure):
    """mydet_lr_tb_level (include/mydet.h)."""
    _fields_ = [('x', c_ptr), ('ldx', c_i64), ('w', c_ptr), ('y', c_ptr), ('ldy', c_i64), ('H', c_int), ('W', c_int)]


LR_TB_MAX_LEVELS = 8                # MYDET_LR_TB_MAX_LEVELS of include/mydet.h
LR_TB_MAX_C = 128                   # MYDET_LR_TB_MAX_C
FRAMES_MAX_TAPS = 17                # MYDET_FRAMES_MAX_TAPS: filter taps per axis mydet_frames_to_input_f32 takes



class Yuv420Src(ctypes.Structure):
    """mydet_yuv420_src (include/mydet.h)."""
    _fields_ = [('plane', c_ptr * 3), ('img_bytes', c_i64 * 3), ('row_bytes', c_i64 * 3), ('layout', c_int), ('matrix', c_int),
                ('full_range', c_int), ('reserved', c_int)]


class TrackParams(ctypes.Structure):
    """mydet_track_params (include/mydet.h): p0, q, r are variances."""
    _fields_ = [('p0', c_f32 * 10), ('q', c_f32 * 10), ('r', c_f32 * 5), ('momentum', c_f32), ('min_score', c_f32),
                ('new_thres', c_f32), ('match_thres', c_f32), ('img_h', c_f32), ('img_w', c_f32), ('max_missed', c_int),
                ('match', c_int)]


class TrackAssoc(ctypes.Structure):
    """mydet_track_assoc (include/mydet.h): the association mode of mydet_track_frames_assoc_f32."""
    _fields_ = [('assign', c_int), ('bands', c_int), ('high_thres', c_f32), ('low_thres', c_f32), ('low_match_thres', c_f32),
                ('reserved', c_int * 3)]


class TrackAppear(ctypes.Structure):
    """mydet_track_appear (include/mydet.h): the appearance settings of mydet_track_frames_appear_f32; gate and reid on the scale of S."""
    _fields_ = [('gate', c_int), ('reid', c_int), ('alpha', c_int), ('reach', c_f32), ('update_thres', c_f32), ('reserved', c_int * 3)]


class MotionSet(ctypes.Structure):
    """mydet_motion_set (include/mydet.h): the settings of the camera-motion estimator; 0 = the default of the frame size.
    reserved: the similarity model's words (the model, then tolerance, max_zoom, max_rotation in Q16), all 0 for the shift."""
    _fields_ = [('reduce', c_int), ('search', c_int), ('min_texture', c_int), ('min_blocks', c_int), ('reserved', c_int * 4)]


class CarrySet(ctypes.Structure):
    """mydet_carry_set (include/mydet.h): the settings of the key-frame carry."""
    _fields_ = [('every', c_int), ('search', c_int), ('min_texture', c_int), ('max_diff', c_int), ('reserved', c_int * 4)]


class ZoneSet(ctypes.Structure):
    """mydet_zone_set (include/mydet.h): quantised polygons and lines, the anchor, the class filter, the heat grid."""
    _fields_ = [('n_polygons', c_int), ('n_lines', c_int), ('n_classes', c_int), ('anchor', c_int), ('coasting', c_int),
                ('img_h', c_int), ('img_w', c_int), ('heat_h', c_int), ('heat_w', c_int), ('reserved', c_int * 3),
                ('n_vertices', c_int * 16), ('polygon', ((c_int * 2) * 16) * 16), ('line', (c_int * 4) * 16), ('classes', c_int * 16)]


class DrawList(ctypes.Structure):
    """mydet_draw_list (include/mydet.h): device pointers with element strides per frame and per row."""
    _fields_ = [('box', c_ptr), ('box_frame_stride', c_i64), ('box_row_stride', c_i64),
                ('angle', c_ptr), ('angle_frame_stride', c_i64), ('angle_row_stride', c_i64),
                ('score', c_ptr), ('score_frame_stride', c_i64), ('score_row_stride', c_i64),
                ('cls', c_ptr), ('cls_frame_stride', c_i64), ('cls_row_stride', c_i64),
                ('id', c_ptr), ('id_frame_stride', c_i64), ('id_row_stride', c_i64),
                ('count', c_ptr), ('count_stride', c_i64), ('K', c_int), ('reserved', c_int)]


class DrawStyle(ctypes.Structure):
    """mydet_draw_style (include/mydet.h)."""
    _fields_ = [('thickness', c_int), ('fill_alpha', c_int), ('color_mode', c_int), ('label_flags', c_int),
                ('color', ctypes.c_ubyte * 4), ('n_palette', c_int), ('ch', c_int), ('cw', c_int), ('n_names', c_int),
                ('palette', c_ptr), ('atlas', c_ptr), ('names', c_ptr)]


class TrailSet(ctypes.Structure):
    """mydet_trail_set (include/mydet.h): the ring length, the anchor and the class filter of mydet_trails_frames."""
    _fields_ = [('max_points', c_int), ('anchor', c_int), ('n_classes', c_int), ('reserved', c_int), ('classes', c_int * 16)]


class OverlayGeometry(ctypes.Structure):
    """mydet_overlay_geometry (include/mydet.h): what the overlay painter reads from a DEVICE buffer."""
    _fields_ = [('n_vertices', c_int * 16), ('polygon', ((c_int * 2) * 16) * 16), ('line', (c_int * 4) * 16), ('tick', (c_int * 4) * 16),
                ('anchor', (c_int * 2) * 32), ('name', (ctypes.c_ubyte * 16) * 32)]


class Overlay(ctypes.Structure):
    """mydet_overlay (include/mydet.h): device pointers and the settings of one overlay launch."""
    _fields_ = [('geometry', c_ptr), ('flags', c_int), ('counters', c_int), ('n_polygons', c_int), ('n_lines', c_int),
                ('zone_alpha', c_int), ('occupied_alpha', c_int), ('thickness', c_int), ('trail_thickness', c_int),
                ('S', c_int), ('F', c_int), ('max_tracks', c_int), ('max_points', c_int), ('coasting', c_int), ('reserved', c_int),
                ('occupancy', c_ptr), ('zone_counts', c_ptr), ('line_counts', c_ptr),
                ('trail_points', c_ptr), ('trail_len', c_ptr), ('trail_bbox', c_ptr), ('id', c_ptr), ('missed', c_ptr)]


class RedactStyle(ctypes.Structure):
    """mydet_redact_style (include/mydet.h)."""
    _fields_ = [('mode', c_int), ('shape', c_int), ('cell', c_int), ('pad', c_f32), ('color', ctypes.c_ubyte * 4), ('n_classes', c_int),
                ('classes', c_int * 16)]


class CropOut(ctypes.Structure):
    """mydet_crop_out (include/mydet.h): mean3 / std3 are host pointers, out a device pointer, strides in elements."""
    _fields_ = [('ch', c_int), ('cw', c_int), ('M', c_int), ('kind', c_int), ('pad', c_f32), ('fill', ctypes.c_ubyte * 4),
                ('norm', c_int), ('reserved', c_int), ('mean3', c_ptr), ('std3', c_ptr), ('out', c_ptr),
                ('slot_stride', c_i64), ('frame_stride', c_i64)]


class EvalSet(ctypes.Structure):
    """mydet_eval_set (include/mydet.h): the packed detections and ground truths, device pointers."""
    _fields_ = [('rotated', c_int), ('I', c_int), ('K', c_int), ('n_groups', c_int), ('max_dt', c_int), ('max_gt', c_int),
                ('D', c_i64), ('G', c_i64), ('n_pairs', c_i64), ('groups', c_ptr), ('dt_start', c_ptr), ('gt_start', c_ptr),
                ('pair_start', c_ptr), ('dt_box', c_ptr), ('gt_box', c_ptr), ('dt_score', c_ptr), ('dt_area', c_ptr), ('gt_area', c_ptr),
                ('gt_flags', c_ptr)]


class MotSet(ctypes.Structure):
    """mydet_mot_set (include/mydet.h): sequences and identities beside a mydet_eval_set, device pointers."""
    _fields_ = [('S', c_int), ('max_gt_ids', c_int), ('max_dt_ids', c_int), ('n_gt_ids', c_i64), ('n_dt_ids', c_i64), ('n_ov', c_i64),
                ('seq_start', c_ptr), ('gt_id', c_ptr), ('dt_id', c_ptr), ('gt_id_start', c_ptr), ('dt_id_start', c_ptr),
                ('ov_start', c_ptr)]


# MYDET_YUV420_* of include/mydet.h
YUV420_NV12, YUV420_NV21, YUV420_I420, YUV420_P010, YUV420_I010 = range(5)

_lib = None


class MissingHipLibrary(ImportError):
    pass


def lib():
    """Load (once) and return the bound library; raise MissingHipLibrary if it was not built."""
    global _lib
    if _lib is None:
        # PyTorch-ROCm ships its own libamdhip64; it must be in the process BEFORE this library is loaded so that
        # both resolve to ONE HIP runtime (otherwise launches here hit a runtime with no device: hipError 100).
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise MissingHipLibrary(
                f'{LIB_PATH} not found. mydetection_amd has no CPU/PyTorch fallback: build the gfx950 '
                'kernels first with  python -c "import __graft_entry__ as g; g.build()"  '
                '(or make -C mydetection_amd/csrc).')
        handle = ctypes.CDLL(LIB_PATH)
        for name, argtypes in SIGNATURES.items():
            fn = getattr(handle, name)          # AttributeError here = ABI mismatch, also loud
            fn.argtypes = argtypes
            fn.restype = c_i64 if name in RETURNS_I64 else c_int
        if handle.mydet_abi_version() != ABI_VERSION:
            raise MissingHipLibrary(f'libmydet_hip.so has ABI version {handle.mydet_abi_version()}, this package binds version {ABI_VERSION}; rebuild it '
                                    '(make -C mydetection_amd/csrc)')
        _lib = handle
    return _lib


class MydetError(RuntimeError):
    pass


def check(code, what):
    if code != 0:
        kind = {-1: 'bad argument', -2: 'unsupported configuration'}.get(code, f'hipError {code}')
        raise MydetError(f'{what} failed: {kind}')
