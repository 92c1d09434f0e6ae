"""ctypes binding of ``libopenglottal_hip.so`` (include/openglottal_hip.h, include/openglottal_hip_crops.h,
include/openglottal_hip_classic.h, include/openglottal_hip_gated.h, include/openglottal_hip_classic_tiled.h,
include/openglottal_hip_overlay.h, include/openglottal_hip_sweep.h, include/openglottal_hip_gate.h,
include/openglottal_hip_mjpeg.h, include/decode/openglottal_hip_mjpd.h, include/split/openglottal_hip_mjps.h,
include_ext/openglottal_hip_png.h, include_enc/openglottal_hip_pnge.h, include_enc/openglottal_hip_aug.h).

cffi is not installed in the build image, so the thin C-ABI layer
the north-star asks for is bound with ctypes; the declarations below are the
exact prototypes of the header.  There is NO fallback: if the shared library is
missing or a call fails, an ``OpenGlottalHipError`` is raised.
"""

from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# OPENGLOTTAL_HIP_LIB: load another build of the same C-ABI (A/B builds, an installed copy)
LIB_PATH = os.environ.get("OPENGLOTTAL_HIP_LIB") or os.path.join(_HERE, "libopenglottal_hip.so")

OG_DTYPE_F32, OG_DTYPE_I64 = 0, 1


class OpenGlottalHipError(RuntimeError):
    pass


_lib = None

# name -> (restype, argtypes); the complete export list of openglottal_hip.h
PROTOTYPES = {
    "og_last_error": (C.c_char_p, []),
    "og_version": (C.c_char_p, []),
    "og_device_count": (C.c_int, []),
    "og_init": (C.c_int, [C.c_int]),
    "og_malloc": (C.c_void_p, [C.c_size_t]),
    "og_free": (C.c_int, [C.c_void_p]),
    "og_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "og_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "og_unet_create": (C.c_void_p, [C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int]),
    "og_unet_destroy": (None, [C.c_void_p]),
    "og_unet_set_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_int]),
    "og_unet_finalize": (C.c_int, [C.c_void_p]),
    "og_unet_forward_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "og_unet_segment_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "og_unet_stream_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "og_unet_stream_frames_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "og_unet_stream_resized_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "og_unet_stream_frames_resized_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                   C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "og_unet_segment_resized_u8_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                 C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "og_linear_taps_host": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "og_unet_segment_u8_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "og_unet_segment_crops_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                           C.c_float, C.c_void_p]),
    "og_unet_segment_crops_u8_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                               C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "og_canvas_letterbox_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                         C.c_void_p]),
    "og_canvas_letterbox_u8_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                             C.c_int, C.c_void_p]),
    "og_mask_stats_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "og_mask_area_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "og_bgr2gray_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "og_bgr2gray_host": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p]),
    "og_unet_sync": (C.c_int, [C.c_void_p]),
    "og_unet_stream": (C.c_void_p, [C.c_void_p]),
    "og_unet_reserve": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "og_unet_set_chunk": (C.c_int, [C.c_void_p, C.c_int]),
    "og_unet_set_graphs": (C.c_int, [C.c_void_p, C.c_int]),
    "og_unet_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "og_timer_start": (C.c_int, [C.c_void_p]),
    "og_timer_stop": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "og_unet_get_activation": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]),
    "og_unet_profile": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p,
                                  C.c_char_p, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "og_unet_clock_probe": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double),
                                      C.POINTER(C.c_int)]),
    "og_unet_clock_probe_raw": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "og_unet_flops_per_frame": (C.c_double, [C.c_void_p, C.c_int, C.c_int]),
    "og_unet_plan_resized": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_longlong)]),
    "og_unet_plan": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_size_t,
                               C.POINTER(C.c_longlong)]),
    "og_workspace_limit": (C.c_longlong, [C.c_int]),
    "og_yolo_create": (C.c_void_p, [C.c_int]),
    "og_yolo_destroy": (None, [C.c_void_p]),
    "og_yolo_set_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_int]),
    "og_yolo_finalize": (C.c_int, [C.c_void_p]),
    "og_yolo_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "og_yolo_plan": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_longlong)]),
    "og_yolo_last_launches": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "og_yolo_num_anchors": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "og_yolo_detect_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "og_yolo_detect_u8_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float]),
    "og_yolo_detect_u8_end": (C.c_int, [C.c_void_p, C.c_void_p]),
    "og_yolo_detect_u8_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "og_yolo_sync": (C.c_int, [C.c_void_p]),
    "og_yolo_letterbox_geometry": (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 6 + [C.POINTER(C.c_double)]),
    "og_yolo_letterbox_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "og_yolo_letterbox_u8_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "og_yolo_detect_resized_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "og_yolo_detect_resized_u8_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                                C.c_void_p]),
    "og_yolo_detect_resized_u8_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float]),
    "og_yolo_launch_count": (C.c_longlong, [C.c_void_p, C.c_char_p]),
    "og_yolo_get_activation": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]),
}

# name -> (restype, argtypes); the complete export list of openglottal_hip_crops.h (the YOLO-Crop+UNet video pipeline)
CROP_PROTOTYPES = {
    "og_crop_geometry_host": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "og_crop_tile_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "og_crop_project_host": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "og_unet_stream_crops_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_float,
                                          C.c_void_p, C.c_void_p]),
    "og_unet_stream_frames_crops_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                 C.c_float, C.c_void_p, C.c_void_p]),
    "og_unet_segment_crops_area_u8_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                    C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "og_unet_plan_crops": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                     C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_longlong)]),
}

# name -> (restype, argtypes); the complete export list of openglottal_hip_classic.h (guided-VFT and YOLO+Otsu)
_VFT_STREAM = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
CLASSIC_PROTOTYPES = {
    "og_classic_limit": (C.c_longlong, [C.c_int]),
    "og_percentile_host": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p]),
    "og_otsu_threshold_host": (C.c_int, [C.c_void_p, C.c_void_p]),
    "og_box_hist_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "og_vft_step_host": (C.c_int, [C.c_double, C.c_double, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]),
    "og_blobs_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "og_classic_create": (C.c_void_p, []),
    "og_classic_destroy": (None, [C.c_void_p]),
    "og_classic_sync": (C.c_int, [C.c_void_p]),
    "og_classic_set_chunk": (C.c_int, [C.c_void_p, C.c_int]),
    "og_vft_guided_reset": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_int]),
    "og_vft_guided_init_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "og_vft_guided_get_state": (C.c_int, [C.c_void_p, C.c_void_p]),
    "og_vft_guided_set_state": (C.c_int, [C.c_void_p, C.c_double]),
    "og_vft_guided_stream_u8": (C.c_int, _VFT_STREAM),
    "og_vft_guided_stream_frames_u8": (C.c_int, _VFT_STREAM),
    "og_vft_guided_u8_dev": (C.c_int, _VFT_STREAM),
    "og_otsu_in_box_u8": (C.c_int, _VFT_STREAM),
    "og_otsu_in_box_u8_dev": (C.c_int, _VFT_STREAM),
    "og_classic_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_longlong)]),
}

# name -> (restype, argtypes); the complete export list of openglottal_hip_gated.h (device tracker, gated engine)
_GATED_STREAM = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
GATED_PROTOTYPES = {
    "og_track_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "og_gated_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_longlong)]),
    "og_gated_create": (C.c_void_p, [C.c_void_p, C.c_void_p]),
    "og_gated_destroy": (None, [C.c_void_p]),
    "og_gated_sync": (C.c_int, [C.c_void_p]),
    "og_gated_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "og_gated_reset": (C.c_int, [C.c_void_p]),
    "og_gated_set_params": (C.c_int, [C.c_void_p, C.c_void_p]),
    "og_gated_get_state": (C.c_int, [C.c_void_p, C.c_void_p]),
    "og_gated_set_state": (C.c_int, [C.c_void_p, C.c_void_p]),
    "og_track_boxes_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "og_gated_stream_u8": (C.c_int, _GATED_STREAM),
    "og_gated_stream_frames_u8": (C.c_int, _GATED_STREAM),
}

# name -> (restype, argtypes); the complete export list of openglottal_hip_classic_tiled.h (the tiled blob filter: frames of any size)
TILED_PROTOTYPES = {
    "og_classic_set_tiled": (C.c_int, [C.c_void_p, C.c_int]),
    "og_classic_tiled_limit": (C.c_longlong, [C.c_int]),
    "og_blobs_host_any": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "og_classic_plan_tiled": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_longlong)]),
}

# name -> (restype, argtypes); the complete export list of openglottal_hip_overlay.h (annotated frames)
_OVERLAY_STREAM = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
OVERLAY_PROTOTYPES = {
    "og_overlay_limit": (C.c_longlong, [C.c_int]),
    "og_outline_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "og_overlay_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "og_overlay_create": (C.c_void_p, []),
    "og_overlay_destroy": (None, [C.c_void_p]),
    "og_overlay_sync": (C.c_int, [C.c_void_p]),
    "og_overlay_set_chunk": (C.c_int, [C.c_void_p, C.c_int]),
    "og_overlay_u8_dev": (C.c_int, _OVERLAY_STREAM),
    "og_overlay_stream_u8": (C.c_int, _OVERLAY_STREAM),
    "og_overlay_stream_frames_u8": (C.c_int, _OVERLAY_STREAM),
    "og_overlay_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_longlong)]),
}

# name -> (restype, argtypes); the complete export list of openglottal_hip_sweep.h (detector ablation sweeps)
_SWEEP_ARGS = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
               C.c_float, C.c_int, C.c_int]
_SWEEP_OUT = [C.c_void_p, C.c_void_p, C.c_void_p]
SWEEP_PROTOTYPES = {
    "og_sweep_limit": (C.c_longlong, [C.c_int]),
    "og_sweep_host": (C.c_int, _SWEEP_ARGS + [C.c_void_p] + _SWEEP_OUT),
    "og_sweep_create": (C.c_void_p, []),
    "og_sweep_destroy": (None, [C.c_void_p]),
    "og_sweep_sync": (C.c_int, [C.c_void_p]),
    "og_sweep_set_chunk": (C.c_int, [C.c_void_p, C.c_int]),
    "og_sweep_reset": (C.c_int, [C.c_void_p]),
    "og_sweep_get_state": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "og_sweep_counts_u8_dev": (C.c_int, [C.c_void_p] + _SWEEP_ARGS + _SWEEP_OUT),
    "og_sweep_counts_u8": (C.c_int, [C.c_void_p] + _SWEEP_ARGS + _SWEEP_OUT),
    "og_sweep_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_longlong)]),
}

# name -> (restype, argtypes); the complete export list of openglottal_hip_gate.h (the U-Net on the kept frames only)
GATE_PROTOTYPES = {
    "og_gate_select_host": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "og_gate_select_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "og_gate_gather_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]),
    "og_gate_scatter_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "og_gated_segment_kept_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "og_gated_stream_kept_u8": (C.c_int, _GATED_STREAM + [C.c_void_p]),
    "og_gated_stream_kept_frames_u8": (C.c_int, _GATED_STREAM + [C.c_void_p]),
    "og_gate_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_longlong)]),
}

# name -> (restype, argtypes); the complete export list of openglottal_hip_mjpeg.h (baseline JPEG on the device)
_MJPEG_ENCODE = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
MJPEG_PROTOTYPES = {
    "og_mjpeg_limit": (C.c_longlong, [C.c_int]),
    "og_jpeg_bound": (C.c_longlong, [C.c_int, C.c_int]),
    "og_jpeg_tables_host": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "og_jpeg_coefficients_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "og_jpeg_encode_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "og_mjpeg_create": (C.c_void_p, []),
    "og_mjpeg_destroy": (None, [C.c_void_p]),
    "og_mjpeg_sync": (C.c_int, [C.c_void_p]),
    "og_mjpeg_set_chunk": (C.c_int, [C.c_void_p, C.c_int]),
    "og_mjpeg_set_quality": (C.c_int, [C.c_void_p, C.c_int]),
    "og_mjpeg_encode_u8_dev": (C.c_int, _MJPEG_ENCODE),
    "og_mjpeg_encode_stream_u8": (C.c_int, _MJPEG_ENCODE),
    "og_mjpeg_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_longlong)]),
}

# name -> (restype, argtypes); the complete export list of decode/openglottal_hip_mjpd.h (baseline JPEG decoded on the device)
MJPD_PROTOTYPES = {
    "og_mjpd_limit": (C.c_longlong, [C.c_int]),
    "og_jpegd_parse_host": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    "og_jpegd_decode_host": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "og_jpegd_idct_pass_host": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "og_jpegd_records_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5),
    "og_mjpd_create": (C.c_void_p, []),
    "og_mjpd_destroy": (None, [C.c_void_p]),
    "og_mjpd_sync": (C.c_int, [C.c_void_p]),
    "og_mjpd_set_chunk": (C.c_int, [C.c_void_p, C.c_int]),
    "og_mjpd_set_tables": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "og_mjpd_decode_u8_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                        C.c_void_p]),
    "og_mjpd_decode_stream": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "og_mjpd_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_longlong)]),
}

# name -> (restype, argtypes); the complete export list of split/openglottal_hip_mjps.h (Motion-JPEG without restart markers in parallel)
MJPS_PROTOTYPES = {
    "og_mjps_limit": (C.c_longlong, [C.c_int]),
    "og_mjps_set_split": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "og_mjps_plan": (C.c_int, [C.c_int] * 8 + [C.c_char_p, C.c_size_t, C.POINTER(C.c_longlong)]),
    "og_jpegs_decode_host": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
}

# name -> (restype, argtypes); the complete export list of include_ext/openglottal_hip_png.h (PNG files decoded on the device)
PNG_PROTOTYPES = {
    "og_png_limit": (C.c_longlong, [C.c_int]),
    "og_pngd_parse_host": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    "og_pngd_inflate_host": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "og_pngd_decode_host": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "og_pngd_records_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                       C.c_int, C.c_void_p, C.c_void_p]),
    "og_png_create": (C.c_void_p, []),
    "og_png_destroy": (None, [C.c_void_p]),
    "og_png_sync": (C.c_int, [C.c_void_p]),
    "og_png_set_chunk": (C.c_int, [C.c_void_p, C.c_int]),
    "og_png_set_palettes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "og_png_decode_u8_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p,
                                       C.c_size_t, C.c_void_p]),
    "og_png_decode_stream": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "og_png_plan": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_longlong)]),
}

# name -> (restype, argtypes); the complete export list of include_enc/openglottal_hip_pnge.h (PNG files encoded on the device)
_PNGE_ENCODE = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
PNGE_PROTOTYPES = {
    "og_pnge_limit": (C.c_longlong, [C.c_int]),
    "og_pnge_bound": (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "og_pnge_filter_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    "og_pnge_deflate_host": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "og_pnge_encode_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "og_pnge_create": (C.c_void_p, []),
    "og_pnge_destroy": (None, [C.c_void_p]),
    "og_pnge_sync": (C.c_int, [C.c_void_p]),
    "og_pnge_set_chunk": (C.c_int, [C.c_void_p, C.c_int]),
    "og_pnge_set_segment": (C.c_int, [C.c_void_p, C.c_int]),
    "og_pnge_encode_u8_dev": (C.c_int, _PNGE_ENCODE),
    "og_pnge_encode_stream_u8": (C.c_int, _PNGE_ENCODE),
    "og_pnge_label_bbox_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "og_pnge_label_bbox_u8_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "og_pnge_crop_tiles_u8_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "og_pnge_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_longlong)]),
}

# name -> (restype, argtypes); the complete export list of include_enc/openglottal_hip_aug.h (crop-training batches augmented on the device)
AUG_PROTOTYPES = {
    "og_aug_limit": (C.c_longlong, [C.c_int]),
    "og_aug_stage_host": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "og_aug_apply_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "og_aug_noise_host": (C.c_int, [C.c_uint64, C.c_size_t, C.c_void_p]),
    "og_aug_create": (C.c_void_p, []),
    "og_aug_destroy": (None, [C.c_void_p]),
    "og_aug_sync": (C.c_int, [C.c_void_p]),
    "og_aug_set_chunk": (C.c_int, [C.c_void_p, C.c_int]),
    "og_aug_batch_u8_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                      C.c_void_p]),
    "og_aug_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_longlong)]),
}


def lib() -> C.CDLL:
    """Load the HIP library once; fail loudly if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OpenGlottalHipError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or openglottal_amd/csrc/build.sh.  There is no CPU fallback."
            )
        # PyTorch-ROCm bundles its own HIP/HSA runtime.  If our library (linked against the system ROCm) initialises HIP
        # first, torch.cuda later reports "No HIP GPUs are available"; loaded in the other order, both share torch's copy.
        # So pull torch in first whenever it is installed (the reference depends on it anyway).
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        try:
            l = C.CDLL(LIB_PATH)
        except OSError as e:  # missing libamdhip64 etc.
            raise OpenGlottalHipError(f"cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in (list(PROTOTYPES.items()) + list(CROP_PROTOTYPES.items()) + list(CLASSIC_PROTOTYPES.items())
                                  + list(GATED_PROTOTYPES.items()) + list(TILED_PROTOTYPES.items()) + list(OVERLAY_PROTOTYPES.items())
                                  + list(SWEEP_PROTOTYPES.items()) + list(GATE_PROTOTYPES.items()) + list(MJPEG_PROTOTYPES.items())
                                  + list(MJPD_PROTOTYPES.items()) + list(MJPS_PROTOTYPES.items()) + list(PNG_PROTOTYPES.items())
                                  + list(PNGE_PROTOTYPES.items()) + list(AUG_PROTOTYPES.items())):
            fn = getattr(l, name)  # AttributeError if a symbol is missing: also loud
            fn.restype = res
            fn.argtypes = args
        ver = (l.og_version() or b"").decode()
        if "store_nop=1" not in ver and os.environ.get("OPENGLOTTAL_HIP_ALLOW_AUDIT_BUILD") != "1":
            # an audit build (-DOG_STORE_NOP=0, tools/epilogue_fence_audit.sh) reproduces a hardware store hazard and computes
            # wrong lanes: never let OPENGLOTTAL_HIP_LIB point the product at one
            raise OpenGlottalHipError(f"{LIB_PATH} reports {ver!r}: not a production build (store_nop=1 missing); refusing to load it")
        _lib = l
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().og_last_error()
        raise OpenGlottalHipError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")


def ptr(x) -> C.c_void_p | None:
    """Raw pointer of a numpy array, a torch tensor (host or device), an int, or None."""
    if x is None:
        return None
    if isinstance(x, int):
        return C.c_void_p(x)
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(x.ctypes.data)
