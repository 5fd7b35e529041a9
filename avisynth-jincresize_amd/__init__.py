"""Python host mirror of the AviSynth+ JincResize plugin surface, over libjincresize_hip.so.

The product is the C-ABI library (include/jincresize_hip.h: host C++ + gfx950 HIP kernels); this
module only binds it with ctypes and mirrors the script-level interface of the reference plugin
(/root/reference/src/JincResize.cpp:1042-1111): ``JincResize(clip, target_width, target_height,
src_left, src_top, src_width, src_height, quant_x, quant_y, tap, blur, cplace, threads, opt,
initial_capacity, initial_factor)`` and the ``Jinc36Resize/Jinc64Resize/Jinc144Resize/
Jinc256Resize`` aliases.  Errors surface as ``JincError`` carrying the reference's message text.

There is no CPU fallback here: if the library is missing the import fails, and frame calls fail
loudly when no HIP device is present.

The directory name contains a hyphen, so load it with ``importlib`` (see ``__graft_entry__.py``
``load_package()``), e.g. as module ``avisynth_jincresize_amd``.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import enum
import os
import subprocess
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("JINC_LIB") or os.path.join(_HERE, "lib", "libjincresize_hip.so")  # JINC_LIB: A/B runs against another build
SIMD_ORDER_ISA_PATH = os.path.join(_HERE, "lib", "kernel_simdorder-gfx950.s")  # the one unit with (explicit) fused multiply-adds
ISA_PATHS = [os.path.join(_HERE, "lib", f"{k}-gfx950.s") for k in ("kernel_gather", "kernel_interleave", "kernel_widen", "kernel_narrow", "kernel_matrix", "kernel_framelane", "kernel_framelane_sub", "kernel_framelane_pair", "kernel_periodic", "kernel_periodic_quad", "kernel_periodic_quad2_rg8", "kernel_periodic_quad2_rg4", "kernel_periodic_quad2x8", "kernel_periodic_rows", "kernel_rowpair", "kernel_strip", "kernel_colpair", "kernel_direct", *[f"kernel_direct_walk_{t}_sx{x}" for t in ("u8", "u16", "f16", "bf16", "f32") for x in (1, 2, 3, 4)], "kernel_colstrip", "kernel_quasi_fs7", "kernel_quasi_fs9", "kernel_quasi_exact_fs7",
                       "kernel_quasi_exact_fs9", "kernel_quasi_lane_fs7", "kernel_quasi_lane_fs9")]
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "jincresize_hip.h")
TEST_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "jincresize_hip_test.h")  # introspection, knobs, hooks


def build(jobs: int = 6) -> str:
    """Compile the HIP/C++ library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-C", _HERE, f"-j{jobs}"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("building libjincresize_hip.so failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    return LIB_PATH


class JincError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(message)
        self.code = code


# ---- ctypes mirror of include/jincresize_hip.h ---------------------------------------------------
class VideoInfo(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("width", "height", "bits_per_component", "component_size", "num_components",
                                       "is_planar", "is_rgb", "sub_w", "sub_h")]


class Args(C.Structure):
    _fields_ = [
        ("target_width", C.c_int), ("target_height", C.c_int),
        ("src_left", C.c_double), ("src_top", C.c_double), ("src_width", C.c_double), ("src_height", C.c_double),
        ("quant_x", C.c_int), ("quant_y", C.c_int), ("tap", C.c_int), ("blur", C.c_double),
        ("cplace", C.c_char_p), ("threads", C.c_int), ("opt", C.c_int), ("initial_capacity", C.c_int),
        ("initial_factor", C.c_double), ("defined", C.c_uint),
        ("frame0_chroma_location", C.c_int),
        ("cpu_has_sse41", C.c_int), ("cpu_has_avx2", C.c_int), ("cpu_has_avx512f", C.c_int),
    ]


class PlanInfo(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("src_width", "src_height", "dst_width", "dst_height", "filter_size", "num_sets",
                                       "periodic", "period_x", "period_y", "step_x", "step_y",
                                       "interior_x0", "interior_x1", "interior_y0", "interior_y1")] + \
               [("plan_bytes", C.c_int64)] + \
               [(n, C.c_int) for n in ("quasi", "quasi_period_x", "quasi_period_y", "quasi_step_x", "quasi_step_y")]


class GroupInfo(C.Structure):
    """jinc_group_info (test header): one pass of the last call with stand-ins (a channel group, a field or a block pass) as its
    launch got it."""
    _fields_ = [(n, C.c_int) for n in ("direction", "n", "members", "sample_bytes", "sample_type", "scaled", "unit", "vec_pixels",
                                       "width", "rows", "shifted")]


ARG_BITS = {"src_left": 1 << 0, "src_top": 1 << 1, "src_width": 1 << 2, "src_height": 1 << 3, "quant_x": 1 << 4,
            "quant_y": 1 << 5, "tap": 1 << 6, "blur": 1 << 7, "cplace": 1 << 8, "threads": 1 << 9, "opt": 1 << 10,
            "initial_capacity": 1 << 11, "initial_factor": 1 << 12}

EXPORTS = ["jinc_device_count", "jinc_pick_device", "jinc_last_error", "jinc_filter_create", "jinc_filter_create_ex", "jinc_batch_create_ex", "jinc_debug_convert_half", "jinc_debug_convert_bfloat16", "jinc_filter_free", "jinc_filter_output_info",
           "jinc_filter_chroma_location", "jinc_filter_set_chroma_location_mode", "jinc_filter_get_frame", "jinc_filter_process_device", "jinc_filter_sync",
           "jinc_alias_args", "jinc_filter_num_tables", "jinc_filter_plan_info", "jinc_filter_plan_pixel",
           "jinc_filter_plan_dump", "jinc_filter_plan_runs", "jinc_filter_plan_set", "jinc_filter_lut", "jinc_filter_set_kernel_mode", "jinc_filter_set_border_strips", "jinc_filter_interior_kernel", "jinc_filter_last_kernel",
           "jinc_filter_set_profiling", "jinc_filter_kernel_times", "jinc_filter_set_border_overlap", "jinc_debug_convert", "jinc_debug_buffer_range_check", "jinc_debug_set_direct_shape", "jinc_debug_last_direct_shape", "jinc_filter_set_simd_order", "jinc_debug_transport_counts", "jinc_debug_staged_frames", "jinc_debug_copy_rows", "jinc_debug_usable_cpus", "jinc_filter_periodic_support", "jinc_filter_periodic_taps", "jinc_filter_set_pipeline",
           "jinc_filter_set_pipeline_group", "jinc_filter_pipeline_group", "jinc_filter_flush", "jinc_filter_adopt_host_range", "jinc_filter_release_host_range", "jinc_batch_set_affinity", "jinc_batch_device_cpus", "jinc_debug_numa_cpus", "jinc_debug_batch_set_registrars", "jinc_debug_batch_refused", "jinc_debug_host_registrations", "jinc_debug_last_call", "jinc_filter_direct_premise", "jinc_debug_valu_pair_probe", "jinc_debug_clock_sampler_start", "jinc_debug_clock_sampler_stop",
           "jinc_filter_submit", "jinc_filter_wait", "jinc_shard_device", "jinc_batch_create", "jinc_batch_devices",
           "jinc_batch_device_of_frame", "jinc_batch_process", "jinc_batch_free", "jinc_batch_last_error",
           "jinc_filter_last_instance", "jinc_filter_last_finite_flags", "jinc_filter_last_border", "jinc_debug_last_instance", "jinc_debug_set_knob", "jinc_debug_clear_knob", "jinc_debug_get_knob", "jinc_debug_knob_name", "jinc_debug_chord_pattern", "jinc_debug_quad2_share", "jinc_debug_quad2_share_products",
           "jinc_filter_process_device_strided", "jinc_debug_strided_groups", "jinc_debug_last_strided", "jinc_debug_last_groups",
           "jinc_filter_process_device_shifted", "jinc_filter_process_device_packed10", "jinc_packed10_layout",
           "jinc_filter_process_device_v210", "jinc_v210_row_bytes", "jinc_filter_process_device_widened",
           "jinc_filter_process_device_widened_packed10", "jinc_filter_process_device_widened_v210",
           "jinc_filter_process_device_narrowed", "jinc_debug_narrow",
           "jinc_filter_process_device_widened_scaled", "jinc_filter_process_device_narrowed_scaled", "jinc_code_range",
           "jinc_debug_widen_scaled", "jinc_debug_narrow_scaled",
           "jinc_filter_process_device_narrowed_packed10", "jinc_filter_process_device_narrowed_v210",
           "jinc_debug_narrow_fields", "jinc_debug_narrow_v210",
           "jinc_filter_process_device_widened_packed10_scaled", "jinc_filter_process_device_widened_v210_scaled",
           "jinc_debug_widen_fields", "jinc_debug_widen_v210",
           "jinc_filter_create_out", "jinc_batch_create_out",
           "jinc_filter_process_device_shifted_packed10", "jinc_filter_process_device_v210_packed10", "jinc_debug_plane_extent_check",
           "jinc_filter_set_output_matrix", "jinc_colour_matrix", "jinc_debug_matrix_rows", "jinc_debug_last_matrix_launches"]

_lib = None
_P4 = C.c_void_p * 4
_I4 = C.c_int * 4
_S4 = C.c_size_t * 4
_F4 = C.c_float * 4


def lib():
    """Loads the C-ABI library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run __graft_entry__.build() (hipcc) first")
        L = C.CDLL(LIB_PATH)
        L.jinc_device_count.restype = C.c_int
        L.jinc_last_error.restype = C.c_char_p
        L.jinc_filter_create.restype = C.c_int
        L.jinc_filter_create.argtypes = [C.POINTER(VideoInfo), C.POINTER(Args), C.c_int, C.POINTER(C.c_void_p),
                                         C.c_char_p, C.c_size_t]
        L.jinc_filter_create_ex.restype = C.c_int
        L.jinc_filter_create_ex.argtypes = [C.POINTER(VideoInfo), C.POINTER(Args), C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                            C.c_char_p, C.c_size_t]
        L.jinc_filter_create_out.restype = C.c_int
        L.jinc_filter_create_out.argtypes = [C.POINTER(VideoInfo), C.POINTER(Args), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                             C.c_char_p, C.c_size_t]
        L.jinc_filter_free.restype = None
        L.jinc_filter_free.argtypes = [C.c_void_p]
        L.jinc_filter_output_info.argtypes = [C.c_void_p, C.POINTER(VideoInfo)]
        L.jinc_filter_chroma_location.argtypes = [C.c_void_p]
        L.jinc_filter_set_chroma_location_mode.argtypes = [C.c_void_p, C.c_int]
        L.jinc_filter_get_frame.argtypes = [C.c_void_p, _P4, _I4, _P4, _I4]
        L.jinc_filter_process_device.argtypes = [C.c_void_p, _P4, _I4, _S4, _P4, _I4, _S4, C.c_int, C.c_void_p]
        L.jinc_filter_process_device_strided.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                         C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.jinc_filter_process_device_shifted.argtypes = [C.c_void_p] + [C.c_void_p] * 10 + [C.c_int, C.c_void_p]
        L.jinc_filter_process_device_packed10.argtypes = [C.c_void_p] + [C.c_void_p] * 7 + [C.c_uint, C.c_void_p, C.c_int, C.c_void_p]
        L.jinc_packed10_layout.argtypes = [C.c_char_p, C.c_int * 3, C.POINTER(C.c_uint)]
        L.jinc_filter_process_device_v210.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                      C.c_void_p, C.c_int, C.c_void_p]
        L.jinc_filter_process_device_widened.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
        L.jinc_filter_process_device_widened_packed10.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p]
        L.jinc_filter_process_device_widened_v210.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p]
        L.jinc_filter_process_device_narrowed.argtypes = [C.c_void_p] + [C.c_void_p] * 8 + [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.jinc_filter_process_device_widened_scaled.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 7 + [C.c_int, C.c_void_p]
        L.jinc_filter_process_device_narrowed_scaled.argtypes = [C.c_void_p] + [C.c_void_p] * 8 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p]
        L.jinc_code_range.argtypes = [C.c_int, C.c_int, C.c_int] + [C.POINTER(C.c_float)] * 4
        L.jinc_v210_row_bytes.argtypes = [C.c_int]
        L.jinc_v210_row_bytes.restype = C.c_size_t
        L.jinc_debug_strided_groups.argtypes = [_P4, _I4, C.c_void_p, C.c_void_p, _I4, _I4, C.c_int, C.c_int, _I4, _I4]
        L.jinc_debug_last_strided.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
        L.jinc_debug_last_groups.argtypes = [C.POINTER(GroupInfo), C.c_int]
        if hasattr(L, "jinc_debug_plane_extent_check"):   # (JINC_LIB may name an older build: A/B runs)
            L.jinc_debug_plane_extent_check.argtypes = [C.c_void_p, _I4, _I4]
        L.jinc_filter_sync.argtypes = [C.c_void_p]
        L.jinc_filter_set_pipeline.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.jinc_filter_set_pipeline_group.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.jinc_filter_pipeline_group.argtypes = [C.c_void_p]
        L.jinc_filter_flush.argtypes = [C.c_void_p]
        L.jinc_filter_direct_premise.argtypes = [C.c_void_p]
        L.jinc_filter_adopt_host_range.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.jinc_filter_release_host_range.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.jinc_batch_set_affinity.argtypes = [C.c_void_p, C.c_int]
        L.jinc_batch_device_cpus.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int]
        L.jinc_debug_batch_set_registrars.argtypes = [C.c_void_p, C.c_int]
        L.jinc_debug_host_registrations.restype = C.c_longlong
        L.jinc_debug_batch_refused.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        L.jinc_debug_numa_cpus.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_int), C.c_int]
        L.jinc_debug_clock_sampler_start.argtypes = [C.c_int, C.c_double, C.POINTER(C.c_void_p)]
        L.jinc_debug_clock_sampler_stop.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.jinc_debug_valu_pair_probe.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.jinc_debug_last_call.argtypes = [C.POINTER(C.c_int)]
        L.jinc_debug_last_call.restype = C.c_char_p
        L.jinc_filter_submit.argtypes = [C.c_void_p, _P4, _I4, _P4, _I4, C.POINTER(C.c_longlong)]
        L.jinc_filter_wait.argtypes = [C.c_void_p, C.c_longlong]
        L.jinc_alias_args.argtypes = [C.c_int, C.POINTER(Args), C.POINTER(Args)]
        L.jinc_filter_num_tables.argtypes = [C.c_void_p]
        L.jinc_filter_plan_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(PlanInfo)]
        L.jinc_filter_plan_pixel.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                             C.POINTER(C.c_int), C.c_void_p]
        L.jinc_filter_plan_dump.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.jinc_filter_plan_runs.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_int]
        L.jinc_filter_plan_set.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.jinc_filter_lut.argtypes = [C.c_void_p, C.c_void_p]
        L.jinc_filter_set_kernel_mode.argtypes = [C.c_void_p, C.c_int]
        L.jinc_filter_set_border_overlap.argtypes = [C.c_void_p, C.c_int]
        L.jinc_filter_set_border_strips.argtypes = [C.c_void_p, C.c_int]
        L.jinc_filter_interior_kernel.argtypes = [C.c_void_p, C.c_int]
        L.jinc_filter_interior_kernel.restype = C.c_char_p
        L.jinc_filter_last_kernel.argtypes = [C.c_void_p, C.c_int]
        L.jinc_filter_last_kernel.restype = C.c_char_p
        L.jinc_debug_convert.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int]
        L.jinc_debug_convert_half.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.jinc_debug_convert_bfloat16.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.jinc_debug_narrow.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.jinc_debug_narrow_scaled.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int]
        L.jinc_filter_process_device_narrowed_packed10.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_void_p, C.c_int, C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        L.jinc_filter_process_device_narrowed_v210.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        L.jinc_debug_narrow_fields.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_int]
        L.jinc_debug_narrow_v210.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.jinc_debug_widen_scaled.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_int]
        L.jinc_filter_process_device_widened_packed10_scaled.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p]
        L.jinc_filter_process_device_widened_v210_scaled.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p]
        L.jinc_debug_widen_fields.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.jinc_debug_widen_v210.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.jinc_filter_set_profiling.argtypes = [C.c_void_p, C.c_int]
        L.jinc_filter_kernel_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int),
                                               C.POINTER(C.c_double), C.POINTER(C.c_int)]
        L.jinc_debug_buffer_range_check.argtypes = [C.c_int]
        L.jinc_debug_set_direct_shape.argtypes = [C.c_int]
        L.jinc_filter_set_simd_order.argtypes = [C.c_void_p, C.c_int]
        L.jinc_filter_periodic_support.argtypes = [C.c_void_p, C.c_int]
        L.jinc_filter_periodic_taps.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.jinc_filter_periodic_taps.restype = C.c_double
        L.jinc_debug_transport_counts.argtypes = [C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.c_int]
        L.jinc_debug_staged_frames.restype = C.c_longlong
        L.jinc_debug_copy_rows.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int]
        L.jinc_debug_staged_frames.argtypes = []
        L.jinc_shard_device.argtypes = [C.c_int, C.c_int]
        L.jinc_batch_create.argtypes = [C.POINTER(VideoInfo), C.POINTER(Args), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                        C.c_char_p, C.c_size_t]
        L.jinc_batch_create_ex.argtypes = [C.POINTER(VideoInfo), C.POINTER(Args), C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
        L.jinc_batch_create_out.argtypes = [C.POINTER(VideoInfo), C.POINTER(Args), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
        L.jinc_batch_devices.argtypes = [C.c_void_p]
        L.jinc_batch_device_of_frame.argtypes = [C.c_void_p, C.c_int]
        L.jinc_batch_process.argtypes = [C.c_void_p, C.c_int, C.c_void_p, _I4, C.c_void_p, _I4]
        L.jinc_batch_free.restype = None
        L.jinc_batch_free.argtypes = [C.c_void_p]
        L.jinc_batch_last_error.restype = C.c_char_p
        L.jinc_filter_last_instance.argtypes = [C.c_void_p, C.c_int]
        L.jinc_filter_last_instance.restype = C.c_char_p
        L.jinc_filter_last_border.argtypes = [C.c_void_p, C.c_int]
        L.jinc_filter_last_finite_flags.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.jinc_debug_last_instance.restype = C.c_char_p
        L.jinc_debug_set_knob.argtypes = [C.c_int, C.c_double]
        L.jinc_debug_clear_knob.argtypes = [C.c_int]
        L.jinc_debug_get_knob.argtypes = [C.c_int, C.POINTER(C.c_double)]
        L.jinc_debug_chord_pattern.argtypes = [C.c_int, C.c_uint64]
        L.jinc_debug_chord_pattern.restype = C.c_int
        L.jinc_debug_quad2_share.argtypes = [C.c_void_p, C.c_void_p]
        L.jinc_debug_quad2_share.restype = C.c_int
        if hasattr(L, "jinc_debug_quad2_share_products"):   # (JINC_LIB may name an older build: A/B runs)
            L.jinc_debug_quad2_share_products.argtypes = [C.c_int]
            L.jinc_debug_quad2_share_products.restype = C.c_int
        L.jinc_debug_knob_name.argtypes = [C.c_int]
        L.jinc_debug_knob_name.restype = C.c_char_p
        if hasattr(L, "jinc_filter_set_output_matrix"):   # (JINC_LIB may name an older build: A/B runs)
            L.jinc_filter_set_output_matrix.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
            L.jinc_colour_matrix.argtypes = [C.c_int, C.c_int, C.c_void_p]
            L.jinc_debug_matrix_rows.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
            L.jinc_debug_last_matrix_launches.argtypes = []
        _lib = L
    return _lib


def device_count() -> int:
    return int(lib().jinc_device_count())


class ClockSampler:
    """Shader clock while other kernels run (jinc_debug_clock_sampler_*): `with ClockSampler(0) as c: ...; c.ghz` = (min, median, max)."""

    def __init__(self, device: int = 0, max_seconds: float = 60.0):
        self._h = C.c_void_p()
        rc = lib().jinc_debug_clock_sampler_start(int(device), float(max_seconds), C.byref(self._h))
        if rc != 0:
            raise JincError(rc, lib().jinc_last_error().decode())
        self.ghz = None

    def stop(self):
        if self._h.value:
            a, b, c = C.c_double(), C.c_double(), C.c_double()
            rc = lib().jinc_debug_clock_sampler_stop(self._h, C.byref(a), C.byref(b), C.byref(c))
            self._h = C.c_void_p()
            if rc != 0:
                raise JincError(rc, lib().jinc_last_error().decode())
            self.ghz = (a.value, b.value, c.value)
        return self.ghz

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.stop()
        return False


def transport_counts(reset: bool = False) -> Tuple[int, int, int]:
    """(frames whose results the shader wrote into pinned host planes, frames that left by DMA copies, host ranges pinned by the
    process-wide registry) over all filter instances of this process since the last reset."""
    a, b, c = C.c_longlong(), C.c_longlong(), C.c_longlong()
    lib().jinc_debug_transport_counts(C.byref(a), C.byref(b), C.byref(c), int(reset))
    return a.value, b.value, c.value


def copy_rows(dst: np.ndarray, src: np.ndarray, row_bytes: int, rows: int, helpers: bool = True) -> None:
    """host_copy.cpp's plane copy between two 2-D arrays (test header; no device needed)."""
    rc = lib().jinc_debug_copy_rows(dst.ctypes.data, dst.strides[0], src.ctypes.data, src.strides[0], int(row_bytes), int(rows), int(helpers))
    if rc != 0:
        raise JincError(rc, lib().jinc_last_error().decode())


def usable_cpus() -> int:
    """CPUs the process may keep busy as the library counts them (test header)."""
    return int(lib().jinc_debug_usable_cpus())


def staged_frames() -> int:
    """Frames whose planes went through the library's own pinned buffers (register_host_buffers = 0) since the last reset of
    transport_counts."""
    return int(lib().jinc_debug_staged_frames())


def host_registrations() -> int:
    """Host ranges the library holds registered with hipHostRegister right now (registry and batch registrars; test header)."""
    return int(lib().jinc_debug_host_registrations())


def valu_pair_probe(device: int = 0, waves_per_simd: int = 8) -> Tuple[float, float]:
    """(Tops, shader clock GHz) that plain v_mul_f32 + v_add_f32 sustain on this part at the given occupancy (measurement hook)."""
    t, g = C.c_double(), C.c_double()
    rc = lib().jinc_debug_valu_pair_probe(int(device), int(waves_per_simd), C.byref(t), C.byref(g))
    if rc != 0:
        raise JincError(rc, lib().jinc_last_error().decode())
    return t.value, g.value


def last_call() -> Tuple[str, int]:
    """(interior kernel of table 0, frames) of the most recent kernel call of any filter instance in this process (test hook)."""
    n = C.c_int()
    name = lib().jinc_debug_last_call(C.byref(n))
    return (name or b"").decode(), n.value


def strided_groups(bases, pitches, steps, frame_strides, widths, heights, component_size: int) -> Tuple[int, List[int], List[int]]:
    """Channel groups of one side's planes for Filter.process_device_strided (test header, no device needed): planes with the same
    step N > 1, pitch, frame stride and dimensions whose bases lie in one N-sample pixel on distinct channels move in one pass.
    `steps` / `frame_strides` may be None (all ones / all zero).  Returns (groups, group of each plane, channel of each plane); dense
    planes have group and channel -1."""
    n = len(bases)
    b, p, w, h, g, c = _P4(), _I4(), _I4(), _I4(), _I4(), _I4()
    st, fs = (_I4() if steps is not None else None), (_S4() if frame_strides is not None else None)
    for i in range(n):
        b[i], p[i], w[i], h[i] = bases[i], pitches[i], widths[i], heights[i]
        if st is not None:
            st[i] = steps[i]
        if fs is not None:
            fs[i] = frame_strides[i]
    rc = int(lib().jinc_debug_strided_groups(b, p, st, fs, w, h, int(component_size), n, g, c))
    if rc < 0:
        raise JincError(rc, lib().jinc_last_error().decode())
    return rc, [int(g[i]) for i in range(n)], [int(c[i]) for i in range(n)]


def last_strided() -> Tuple[int, int, int, int]:
    """(split launches, merge launches, slices, bytes of dense planes held) of the calling thread's most recent
    process_device_strided call (test header); launches and slices are 0 when every step was 1."""
    a, b, c, d = C.c_int(), C.c_int(), C.c_int(), C.c_longlong()
    lib().jinc_debug_last_strided(C.byref(a), C.byref(b), C.byref(c), C.byref(d))
    return a.value, b.value, c.value, d.value


def last_groups() -> List[Dict[str, int]]:
    """The passes of the first slice of the calling thread's most recent strided / shifted / packed10 / v210 / widened / narrowed call
    (scaled or not) as their launches got them (jinc_debug_last_groups, test header): one dict per channel group of the widening,
    narrowing, split and merge launches and one per field or block pass, the source side's first, then the destination side's, each
    side in the order of its groups' first planes.  Keys: direction (0 widened, 1 narrowed, 2 split, 3 merge, 4 / 5 / 6 unpack_fields /
    pack_fields / widen_fields, 7 / 8 / 9 unpack_v210 / pack_v210 / widen_v210, 10 / 11 narrow_fields / narrow_v210), n (samples per pixel), members, sample_bytes,
    sample_type (SAMPLE_*), scaled, unit (16, 4 or 0), vec_pixels (0: the whole row moved sample by sample; v210: 6 x the blocks
    that moved in pairs), width, rows and shifted (split / merge: the launch took the shifted form).  At most 8; empty after a call
    on dense planes alone."""
    g = (GroupInfo * 8)()
    count = int(lib().jinc_debug_last_groups(g, 8))
    return [{name: int(getattr(g[i], name)) for name, _ in GroupInfo._fields_} for i in range(count)]


def packed10_layout(name: str) -> Tuple[List[int], int]:
    """(field offsets in the library's plane order, the fill with every spare bit set) of a named 10:10:10:2 word for
    Filter.process_device_packed10 (jinc_packed10_layout; no device needed): Y410, R10G10B10A2, ABGR2101010, XBGR2101010, ARGB2101010,
    XRGB2101010, RGBA1010102, RGBX1010102, BGRA1010102, BGRX1010102, in either letter case."""
    o, fill = (C.c_int * 3)(), C.c_uint()
    rc = int(lib().jinc_packed10_layout(name.encode(), o, C.byref(fill)))
    if rc != 0:
        raise JincError(rc, lib().jinc_last_error().decode())
    return [int(o[i]) for i in range(3)], int(fill.value)


def v210_row_bytes(width: int) -> int:
    """Bytes of the blocks of one v210 row of `width` luma samples, 16 * ceil(width / 6); 0 for width < 1 (jinc_v210_row_bytes; no
    device needed).  Writers conventionally pad the pitch to a multiple of 128 bytes."""
    return int(lib().jinc_v210_row_bytes(int(width)))


class KernelMode(enum.IntEnum):
    """enum jinc_kernel_mode of include/jincresize_hip_test.h."""
    AUTO = 0
    GATHER = 1
    PERIODIC = 2
    ROWS = 3
    WINDOW_HALF_TILES = 4
    PACKED_RG4 = 5
    PACKED_RG8 = 6
    QUASI = 7
    QUASI_WATERFALL = 8
    DIRECT = 9
    QUASI_LANE = 10
    FRAMELANE = 11
    FRAMELANE_PAIR = 12
    QUAD = 13
    RUNS = 14
    FULL_WINDOW = 15
    FRAMELANE_SUB = 16


def knob_ids() -> dict:
    """{lower-case knob name: id} as the loaded library lists them (enum jinc_knob of the test header)."""
    out, k = {}, 0
    while True:
        name = lib().jinc_debug_knob_name(k)
        if not name:
            return out
        out[name.decode()] = k
        k += 1


def set_knob(name: str, value: float) -> None:
    """Process-wide A/B / tuning knob (test header): `name` as in knob_ids(), e.g. "quad_rg"."""
    ids = knob_ids()
    if name.lower() not in ids:
        raise KeyError(f"no such knob: {name}")
    rc = lib().jinc_debug_set_knob(ids[name.lower()], float(value))
    if rc != 0:
        raise JincError(rc, lib().jinc_last_error().decode())


def clear_knob(name: Optional[str] = None) -> None:
    """One knob (or, without a name, every knob) back to unset."""
    rc = lib().jinc_debug_clear_knob(-1 if name is None else knob_ids()[name.lower()])
    if rc != 0:
        raise JincError(rc, lib().jinc_last_error().decode())


def get_knob(name: str) -> Optional[float]:
    v = C.c_double()
    return v.value if lib().jinc_debug_get_knob(knob_ids()[name.lower()], C.byref(v)) == 1 else None


class knobs:
    """`with knobs(quad_rg=8): ...` sets knobs for a block and restores what was there before."""

    def __init__(self, **kv):
        self._kv = kv
        self._old = {}

    def __enter__(self):
        for k, v in self._kv.items():
            self._old[k] = get_knob(k)
            set_knob(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self._old.items():
            clear_knob(k) if v is None else set_knob(k, v)
        return False


# JINC_<NAME> environment variables the profiles/ scripts and recheck_rules.py pass: translated into knobs by bench.py (the
# library itself never reads the environment for them).
def apply_env_knobs(environ=None) -> dict:
    """Sets the knobs the environment names; JINC_* variables that name no knob are reported on stderr and returned under
    "unknown_variables" (a script that still sets a variable whose knob is gone measures A against A without a word).
    JINC_LIB, JINC_BENCH_* and the profiles/ scripts' own variables are not knobs by design."""
    environ = os.environ if environ is None else environ
    applied = {}
    known = {"JINC_" + n.upper() for n in knob_ids()}
    # (not knobs by design: the loader's JINC_LIB, bench.py's JINC_BENCH_*, the variables of the profiles/ scripts and of the tests)
    own = ("JINC_LIB", "JINC_FRAMES_PER_LAUNCH")
    own_prefixes = ("JINC_BENCH_", "JINC_PROFILE_", "JINC_LINE_", "JINC_TEST_")
    unknown = sorted(k for k in environ if k.startswith("JINC_") and k not in known and k not in own and not k.startswith(own_prefixes))
    if unknown:
        import sys
        print("avisynth_jincresize_amd: environment variables that name no knob (ignored): " + ", ".join(unknown), file=sys.stderr, flush=True)
        applied["unknown_variables"] = unknown
    for name in knob_ids():
        e = environ.get("JINC_" + name.upper())
        if e is None or e == "":
            continue
        if name == "pipeline_skip":
            e = {"h2d": "1", "kernels": "2"}.get(e, e)
        set_knob(name, float(e))
        applied[name] = float(e)
    return applied


def last_instance() -> str:
    """Full instantiation of the interior kernel (table 0) of the most recent kernel call of any filter instance in this process."""
    return (lib().jinc_debug_last_instance() or b"").decode()


def set_direct_shape(shape: int) -> None:
    """Process-wide A/B knob of ewa_direct_kernel's interior form (test hook): 0 per-chain fetches, 2 row walk, 3 row walk
    with 8 columns per lane (where it applies), -1 automatic."""
    rc = lib().jinc_debug_set_direct_shape(int(shape))
    if rc != 0:
        raise JincError(rc, lib().jinc_last_error().decode())


def last_direct_shape() -> int:
    """Interior form of the most recent ewa_direct_kernel interior launch in this process (test hook)."""
    return int(lib().jinc_debug_last_direct_shape())


def debug_convert(sums: np.ndarray, dtype, peak: float, device: int = 0) -> np.ndarray:
    """The kernels' sum -> sample conversion applied to `sums` on the device (test hook)."""
    sums = np.ascontiguousarray(sums, dtype=np.float32)
    out = np.zeros(sums.shape, dtype=dtype)
    rc = lib().jinc_debug_convert(sums.ctypes.data, out.ctypes.data, sums.size, out.dtype.itemsize, float(peak), device)
    if rc != 0:
        raise JincError(rc, lib().jinc_last_error().decode())
    return out


def debug_convert_half(sums: np.ndarray, device: int = 0) -> np.ndarray:
    """The half planes' fp32 -> binary16 store path applied to `sums` on the device (test hook); returns float16."""
    sums = np.ascontiguousarray(sums, dtype=np.float32)
    out = np.zeros(sums.shape, dtype=np.uint16)
    rc = lib().jinc_debug_convert_half(sums.ctypes.data, out.ctypes.data, sums.size, device)
    if rc != 0:
        raise JincError(rc, lib().jinc_last_error().decode())
    return out.view(np.float16)


def debug_convert_bfloat16(sums: np.ndarray, device: int = 0) -> np.ndarray:
    """The bfloat16 planes' fp32 -> bfloat16 store path applied to `sums` on the device (test hook); returns the bit patterns as
    uint16 (numpy has no bfloat16 dtype)."""
    sums = np.ascontiguousarray(sums, dtype=np.float32)
    out = np.zeros(sums.shape, dtype=np.uint16)
    rc = lib().jinc_debug_convert_bfloat16(sums.ctypes.data, out.ctypes.data, sums.size, device)
    if rc != 0:
        raise JincError(rc, lib().jinc_last_error().decode())
    return out


def debug_narrow(values: np.ndarray, dst_bits: int, shift: int = 0, bfloat16: bool = False, device: int = 0) -> np.ndarray:
    """The narrowing pass of process_device_narrowed applied to one dense row of `values` on the device (test hook): float32 or
    float16 values, or with bfloat16=True uint16 bit patterns of bfloat16 values; returns rint(clip(value, 0, 2^dst_bits - 1)) << shift
    as uint8 (dst_bits 8) or uint16 (9 .. 16)."""
    values = np.ascontiguousarray(values)
    if bfloat16:
        if values.dtype != np.uint16:
            raise TypeError("bfloat16 values are given as uint16 bit patterns")
        kind = SAMPLE_BFLOAT16
    elif values.dtype == np.float16:
        kind = SAMPLE_FLOAT16
    else:
        values, kind = np.ascontiguousarray(values, dtype=np.float32), SAMPLE_DEFAULT
    out = np.zeros(values.shape, dtype=np.uint8 if dst_bits == 8 else np.uint16)
    rc = lib().jinc_debug_narrow(values.ctypes.data, kind, out.ctypes.data, values.size, int(dst_bits), int(shift), device)
    if rc != 0:
        raise JincError(rc, lib().jinc_last_error().decode())
    return out


def debug_narrow_scaled(values: np.ndarray, dst_bits: int, shift: int, scale: float, offset: float, bfloat16: bool = False,
                        device: int = 0) -> np.ndarray:
    """The scaled narrowing pass of process_device_narrowed_scaled applied to one dense row of `values` on the device (test hook;
    values as for debug_narrow); returns rint(clip(fl32(fl32(value * scale) + offset), 0, 2^dst_bits - 1)) << shift as uint8
    (dst_bits 8) or uint16 (9 .. 16)."""
    values = np.ascontiguousarray(values)
    if bfloat16:
        if values.dtype != np.uint16:
            raise TypeError("bfloat16 values are given as uint16 bit patterns")
        kind = SAMPLE_BFLOAT16
    elif values.dtype == np.float16:
        kind = SAMPLE_FLOAT16
    else:
        values, kind = np.ascontiguousarray(values, dtype=np.float32), SAMPLE_DEFAULT
    out = np.zeros(values.shape, dtype=np.uint8 if dst_bits == 8 else np.uint16)
    rc = lib().jinc_debug_narrow_scaled(values.ctypes.data, kind, out.ctypes.data, values.size, int(dst_bits), int(shift), float(scale),
                                        float(offset), device)
    if rc != 0:
        raise JincError(rc, lib().jinc_last_error().decode())
    return out


def _hook_planes(planes, bfloat16):
    """The three rows of debug_narrow_fields / debug_narrow_v210 as contiguous arrays of one kind, and that kind."""
    planes = [np.ascontiguousarray(p) for p in planes]
    if len(planes) != 3:
        raise ValueError("three planes are needed")
    if bfloat16:
        if any(p.dtype != np.uint16 for p in planes):
            raise TypeError("bfloat16 values are given as uint16 bit patterns")
        return planes, SAMPLE_BFLOAT16
    if all(p.dtype == np.float16 for p in planes):
        return planes, SAMPLE_FLOAT16
    return [np.ascontiguousarray(p, dtype=np.float32) for p in planes], SAMPLE_DEFAULT


def _three_floats(values):
    return None if values is None else (C.c_float * 3)(*[float(v) for v in values])


def debug_narrow_fields(planes, offsets, fill: int = 0, scale=None, offset=None, bfloat16: bool = False, device: int = 0) -> np.ndarray:
    """The pass of process_device_narrowed_packed10 applied to one dense row per plane on the device (test hook): `planes` are three
    rows of one length, float32 or float16 values, or with bfloat16=True uint16 bit patterns; scale / offset are three floats each or
    None.  Returns the words (v0 << offsets[0]) | (v1 << offsets[1]) | (v2 << offsets[2]) | (fill & ~fields) as uint32."""
    planes, kind = _hook_planes(planes, bfloat16)
    n = planes[0].size
    if planes[1].size != n or planes[2].size != n:
        raise ValueError("the three planes must have one length")
    out = np.zeros(n, dtype=np.uint32)
    rc = lib().jinc_debug_narrow_fields((C.c_void_p * 3)(*[p.ctypes.data for p in planes]), kind, out.ctypes.data, n,
                                        (C.c_int * 3)(*[int(o) for o in offsets]), int(fill) & 0xFFFFFFFF, _three_floats(scale),
                                        _three_floats(offset), device)
    if rc != 0:
        raise JincError(rc, lib().jinc_last_error().decode())
    return out


def debug_narrow_v210(planes, scale=None, offset=None, bfloat16: bool = False, device: int = 0) -> np.ndarray:
    """The pass of process_device_narrowed_v210 applied to one dense row on the device (test hook): planes[0] holds `width` (even) luma
    values, planes[1] and planes[2] width / 2 chroma values each, kinds as for debug_narrow_fields.  Returns the row's blocks as
    uint32 words, four per block."""
    planes, kind = _hook_planes(planes, bfloat16)
    width = planes[0].size
    if width % 2 or planes[1].size != width // 2 or planes[2].size != width // 2:
        raise ValueError("an even number of luma values and half as many of each chroma plane are needed")
    out = np.zeros(4 * ((width + 5) // 6), dtype=np.uint32)
    rc = lib().jinc_debug_narrow_v210((C.c_void_p * 3)(*[p.ctypes.data for p in planes]), kind, out.ctypes.data, width, _three_floats(scale),
                                      _three_floats(offset), device)
    if rc != 0:
        raise JincError(rc, lib().jinc_last_error().decode())
    return out


def debug_widen_scaled(raw: np.ndarray, src_bits: int, shift: int, scale: float, offset: float, out_kind: int = 0,
                       device: int = 0) -> np.ndarray:
    """The scaled widening pass of process_device_widened_scaled applied to one dense row of integer samples on the device (test
    hook): uint8 samples for src_bits 8, uint16 words for 9 .. 16.  Returns fl32(fl32(float((raw >> shift) & mask) * scale) + offset)
    as float32 (out_kind SAMPLE_DEFAULT), float16 (SAMPLE_FLOAT16) or uint16 bfloat16 bit patterns (SAMPLE_BFLOAT16), the 16-bit
    types rounded to nearest even."""
    raw = np.ascontiguousarray(raw, dtype=np.uint8 if src_bits == 8 else np.uint16)
    out = np.zeros(raw.shape, dtype=np.float32 if out_kind == SAMPLE_DEFAULT else np.uint16)
    rc = lib().jinc_debug_widen_scaled(raw.ctypes.data, int(src_bits), int(shift), float(scale), float(offset), int(out_kind),
                                       out.ctypes.data, raw.size, device)
    if rc != 0:
        raise JincError(rc, lib().jinc_last_error().decode())
    return out.view(np.float16) if out_kind == SAMPLE_FLOAT16 else out


def _widen_hook_out(n_luma: int, n_chroma: int, out_kind: int):
    dtype = np.float32 if out_kind == SAMPLE_DEFAULT else np.uint16
    return [np.zeros(n_luma, dtype=dtype), np.zeros(n_chroma, dtype=dtype), np.zeros(n_chroma, dtype=dtype)]


def debug_widen_fields(words: np.ndarray, offsets, scale=None, offset=None, out_kind: int = 0, device: int = 0):
    """The pass of process_device_widened_packed10(_scaled) applied to one row of 32-bit words on the device (test hook): returns the
    three planes fl32(fl32(float((word >> offsets[c]) & 1023) * scale[c]) + offset[c]) as float32 (out_kind SAMPLE_DEFAULT), float16
    (SAMPLE_FLOAT16) or uint16 bfloat16 bit patterns (SAMPLE_BFLOAT16), the 16-bit types rounded to nearest even.  scale / offset
    are three floats each or None; both None runs the unscaled form (no bfloat16 there)."""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    out = _widen_hook_out(words.size, words.size, out_kind)
    rc = lib().jinc_debug_widen_fields(words.ctypes.data, words.size, (C.c_int * 3)(*[int(o) for o in offsets]), _three_floats(scale),
                                       _three_floats(offset), int(out_kind), (C.c_void_p * 3)(*[p.ctypes.data for p in out]), device)
    if rc != 0:
        raise JincError(rc, lib().jinc_last_error().decode())
    return [p.view(np.float16) if out_kind == SAMPLE_FLOAT16 else p for p in out]


def debug_widen_v210(blocks: np.ndarray, width: int, scale=None, offset=None, out_kind: int = 0, device: int = 0):
    """The pass of process_device_widened_v210(_scaled) applied to one row of blocks (uint32 words, four per block,
    4 * ceil(width / 6) of them; width even) on the device (test hook): returns `width` luma samples and width / 2 samples of Cb and
    of Cr, kinds and pairs as for debug_widen_fields."""
    blocks = np.ascontiguousarray(blocks, dtype=np.uint32)
    if width % 2 or blocks.size != 4 * ((width + 5) // 6):
        raise ValueError("an even width and 4 * ceil(width / 6) words are needed")
    out = _widen_hook_out(width, width // 2, out_kind)
    rc = lib().jinc_debug_widen_v210(blocks.ctypes.data, int(width), _three_floats(scale), _three_floats(offset), int(out_kind),
                                     (C.c_void_p * 3)(*[p.ctypes.data for p in out]), device)
    if rc != 0:
        raise JincError(rc, lib().jinc_last_error().decode())
    return [p.view(np.float16) if out_kind == SAMPLE_FLOAT16 else p for p in out]


RANGE_FULL, RANGE_LIMITED = 0, 1          # jinc_code_range: range
PLANE_LUMA_OR_RGB, PLANE_CHROMA = 0, 1    # jinc_code_range: plane_kind


def code_range(bits: int, range: int, plane_kind: int) -> Tuple[float, float, float, float]:
    """jinc_code_range: (to_float_scale, to_float_offset, to_code_scale, to_code_offset) between the code values of a `bits`-bit
    plane and the float range 0 .. 1 (luma, RGB) or -0.5 .. 0.5 (chroma), as float32 values; needs no device."""
    v = [C.c_float() for _ in (0, 1, 2, 3)]
    rc = lib().jinc_code_range(int(bits), int(range), int(plane_kind), *[C.byref(x) for x in v])
    if rc != 0:
        raise JincError(rc, lib().jinc_last_error().decode())
    return tuple(np.float32(x.value) for x in v)


MATRIX_BT601, MATRIX_BT709, MATRIX_BT2020_NCL = 0, 1, 2   # jinc_colour_matrix: standard
YCBCR_TO_RGB, RGB_TO_YCBCR = 0, 1                         # ... and direction


def colour_matrix(standard: int, direction: int) -> np.ndarray:
    """jinc_colour_matrix: the 3 x 3 float32 matrix between normalised Y' (0 .. 1), Cb / Cr (-0.5 .. 0.5) and R'G'B' (0 .. 1), rows
    in R, G, B (to RGB) or Y', Cb, Cr (from RGB) order; needs no device."""
    m = (C.c_float * 9)()
    rc = lib().jinc_colour_matrix(int(standard), int(direction), m)
    if rc != 0:
        raise JincError(rc, lib().jinc_last_error().decode())
    return np.array(list(m), dtype=np.float32).reshape(3, 3)


def last_matrix_launches() -> int:
    """jinc_debug_last_matrix_launches: the output matrix launches of this thread's most recent process_device* call."""
    return int(lib().jinc_debug_last_matrix_launches())


def debug_matrix_rows(rows, m, offset=None, bfloat16: bool = False, device: int = 0):
    """The output matrix pass applied to three dense rows on the device (test hook): float32 or float16 values, or with bfloat16=True
    uint16 bit patterns; returns the three rows after o = M r + offset in the rows' own type."""
    rows, kind = _hook_planes(rows, bfloat16)
    if len({r.size for r in rows}) != 1:
        raise ValueError("three rows of one length are needed")
    rows = [r.copy() for r in rows]
    ptrs = (C.c_void_p * 3)(*[r.ctypes.data for r in rows])
    mm = (C.c_float * 9)(*[float(v) for v in np.asarray(m, dtype=np.float32).reshape(9)])
    rc = lib().jinc_debug_matrix_rows(ptrs, kind, rows[0].size, mm, _three_floats(offset), device)
    if rc != 0:
        raise JincError(rc, lib().jinc_last_error().decode())
    return rows


# Sample types of jinc_filter_create_ex / jinc_batch_create_ex
SAMPLE_DEFAULT = 0
SAMPLE_FLOAT16 = 1
SAMPLE_BFLOAT16 = 3  # (2 is not a sample type: jinc_filter_create_ex keeps refusing it)


# ---- clip / format model (what an AviSynth+ host would provide) -----------------------------------
@dataclass(frozen=True)
class Format:
    name: str
    bits: int
    planes: int
    sub_w: int = 0
    sub_h: int = 0
    rgb: bool = False
    half: bool = False  # IEEE binary16 samples (bits 16, 2 bytes): created with SAMPLE_FLOAT16; bits == 32 stays fp32
    bfloat16: bool = False  # bfloat16 samples (bits 16, 2 bytes): created with SAMPLE_BFLOAT16; planes are uint16 bit patterns

    @property
    def sample_bytes(self) -> int:
        return 1 if self.bits == 8 else (2 if self.bits <= 16 else 4)

    @property
    def sample_type(self) -> int:
        return SAMPLE_FLOAT16 if self.half else (SAMPLE_BFLOAT16 if self.bfloat16 else SAMPLE_DEFAULT)

    @property
    def dtype(self):
        if self.half:
            return np.float16
        return {1: np.uint8, 2: np.uint16, 4: np.float32}[self.sample_bytes]

    def plane_dims(self, w: int, h: int) -> List[Tuple[int, int]]:
        dims = [(w, h)]
        if self.planes >= 3:
            dims += [(w >> self.sub_w, h >> self.sub_h)] * 2
        if self.planes == 4:
            dims.append((w, h))
        return dims

    def video_info(self, w: int, h: int) -> VideoInfo:
        return VideoInfo(w, h, self.bits, self.sample_bytes, self.planes, 1, int(self.rgb), self.sub_w, self.sub_h)


def _fmts() -> Dict[str, Format]:
    out = {}
    for bits, tag in ((8, "8"), (10, "10"), (12, "12"), (14, "14"), (16, "16"), (32, "S")):
        out[f"Y{tag if bits != 32 else '32'}"] = Format(f"Y{tag if bits != 32 else '32'}", bits, 1)
        for fam, sw, sh in (("420", 1, 1), ("422", 1, 0), ("444", 0, 0), ("411", 2, 0)):
            out[f"YUV{fam}P{tag}"] = Format(f"YUV{fam}P{tag}", bits, 3, sw, sh)
            out[f"YUVA{fam}P{tag}"] = Format(f"YUVA{fam}P{tag}", bits, 4, sw, sh)
        out[f"RGBP{tag}"] = Format(f"RGBP{tag}", bits, 3, rgb=True)
        out[f"RGBAP{tag}"] = Format(f"RGBAP{tag}", bits, 4, rgb=True)
    out["YV12"], out["YV16"], out["YV24"], out["YV411"] = out["YUV420P8"], out["YUV422P8"], out["YUV444P8"], out["YUV411P8"]
    # half-precision float planes (beyond the reference: VapourSynth GRAYH / YUV4xxPH / RGBH)
    out["YH"] = Format("YH", 16, 1, half=True)
    for fam, sw, sh in (("420", 1, 1), ("422", 1, 0), ("444", 0, 0), ("411", 2, 0)):
        out[f"YUV{fam}PH"] = Format(f"YUV{fam}PH", 16, 3, sw, sh, half=True)
        out[f"YUVA{fam}PH"] = Format(f"YUVA{fam}PH", 16, 4, sw, sh, half=True)
    out["RGBPH"] = Format("RGBPH", 16, 3, rgb=True, half=True)
    out["RGBAPH"] = Format("RGBAPH", 16, 4, rgb=True, half=True)
    # bfloat16 planes (the upper halves of fp32 values; numpy has no such dtype: planes are np.uint16 holding the bit patterns)
    out["YBF"] = Format("YBF", 16, 1, bfloat16=True)
    for fam, sw, sh in (("420", 1, 1), ("422", 1, 0), ("444", 0, 0), ("411", 2, 0)):
        out[f"YUV{fam}PBF"] = Format(f"YUV{fam}PBF", 16, 3, sw, sh, bfloat16=True)
        out[f"YUVA{fam}PBF"] = Format(f"YUVA{fam}PBF", 16, 4, sw, sh, bfloat16=True)
    out["RGBPBF"] = Format("RGBPBF", 16, 3, rgb=True, bfloat16=True)
    out["RGBAPBF"] = Format("RGBAPBF", 16, 4, rgb=True, bfloat16=True)
    return out


FORMATS = _fmts()


def alloc_plane(w: int, h: int, dtype, align: int = 64) -> np.ndarray:
    """Host plane with an AviSynth+-style pitch (row size rounded up to 64 bytes)."""
    isz = np.dtype(dtype).itemsize
    pitch = (w * isz + align - 1) // align * align
    return np.zeros((h, pitch // isz), dtype=dtype)


@dataclass
class Clip:
    """Minimal stand-in for an AviSynth clip: format, size, and a frame source returning planes in the
    reference's processing order (Y,U,V,A or G,B,R,A; ref JincResize.cpp:539-541)."""
    fmt: Format
    width: int
    height: int
    num_frames: int
    source: Callable[[int], Sequence[np.ndarray]]
    props: Dict[str, int] = field(default_factory=dict)  # frame properties of frame 0 (e.g. _ChromaLocation)
    planar: bool = True

    def get_frame(self, n: int) -> Sequence[np.ndarray]:
        return self.source(n)


def _out_format(fmt: "Format", out_sub) -> "Format":
    """The format of a filter's output planes: `fmt` with the chroma sub-sampling of out_sub=(w, h) (None or -1s: fmt itself)."""
    if out_sub is None or tuple(out_sub) == (-1, -1) or tuple(out_sub) == (fmt.sub_w, fmt.sub_h):
        return fmt
    return dataclasses.replace(fmt, name=f"{fmt.name}>sub{out_sub[0]}{out_sub[1]}", sub_w=int(out_sub[0]), sub_h=int(out_sub[1]))


def _build_args(fmt, width, height, target_width, target_height, frame0_chroma_location, planar, cpu_flags, alias_taps, kw):
    """jinc_video_info + jinc_args of a JincResize() call (keyword names = the script arguments)."""
    vi = fmt.video_info(width, height)
    vi.is_planar = int(planar)
    a = Args()
    a.target_width, a.target_height = int(target_width), int(target_height)
    a.frame0_chroma_location = int(frame0_chroma_location)
    a.cpu_has_sse41, a.cpu_has_avx2, a.cpu_has_avx512f = (int(bool(x)) for x in cpu_flags)
    keep = []
    for k, v in kw.items():
        if k not in ARG_BITS:
            raise TypeError(f"JincResize: unknown argument {k!r}")
        if v is None:
            continue
        a.defined |= ARG_BITS[k]
        if k == "cplace":
            b = str(v).encode()
            keep.append(b)
            a.cplace = b
        else:
            setattr(a, k, v)
    if alias_taps is not None:
        b = Args()
        rc = lib().jinc_alias_args(int(alias_taps), C.byref(a), C.byref(b))
        if rc != 0:
            raise JincError(rc, lib().jinc_last_error().decode())
        a = b
    return vi, a, keep


# register_host_buffers of set_pipeline / Batch (include/jincresize_hip.h): pageable planes copied by the CPU through pinned buffers of
# the library's own (the default) / registered once and cached (any other non-zero value) / pageable planes handed to the HIP runtime
# as they are (which maps them into the device itself behind every copy)
PIN_NONE, PIN_POOL, PIN_RUNTIME = 0, 2, 3


def numa_cpus(sysfs_root: str, bdf: str) -> List[int]:
    """batch.cpp's NUMA lookup against a sysfs tree of the caller's (test header)."""
    buf = (C.c_int * 4096)()
    n = int(lib().jinc_debug_numa_cpus(sysfs_root.encode(), bdf.encode(), buf, 4096))
    return [int(buf[i]) for i in range(max(0, min(n, 4096)))]


class Batch:
    """Frames of one clip sharded over the node's HIP devices (jinc_batch_*: frame n -> device n mod G, a plan replica
    and `streams` frames in flight per device, no exchange between devices)."""

    def __init__(self, fmt: Format, width: int, height: int, target_width: int, target_height: int, *, ndevices: int = 0,
                 streams: int = 2, register_host_buffers: bool = False, out_sub: Optional[Tuple[int, int]] = None, **kw):
        """out_sub=(w, h): the output's chroma sub-sampling (jinc_batch_create_out); None: the input's (jinc_batch_create_ex)."""
        self.fmt = fmt
        vi, a, self._keep = _build_args(fmt, width, height, target_width, target_height, -1, True, (True, True, True), None, kw)
        self._h = C.c_void_p()
        err = C.create_string_buffer(512)
        if out_sub is None:
            rc = lib().jinc_batch_create_ex(C.byref(vi), C.byref(a), fmt.sample_type, int(ndevices), int(streams), int(register_host_buffers),
                                            C.byref(self._h), err, len(err))
        else:
            rc = lib().jinc_batch_create_out(C.byref(vi), C.byref(a), fmt.sample_type, int(out_sub[0]), int(out_sub[1]), int(ndevices),
                                             int(streams), int(register_host_buffers), C.byref(self._h), err, len(err))
        if rc != 0:
            raise JincError(rc, err.value.decode())
        self.out_fmt = _out_format(fmt, out_sub)
        self.dst_w, self.dst_h = int(target_width), int(target_height)

    @property
    def devices(self) -> int:
        return int(lib().jinc_batch_devices(self._h))

    def set_affinity(self, on: bool) -> None:
        """Workers / registrars of device d on the CPUs of d's NUMA node (default) or wherever the scheduler puts them."""
        lib().jinc_batch_set_affinity(self._h, int(bool(on)))

    def set_registrars(self, n: int) -> None:
        """Test header: n registrar threads per process() call instead of one per device."""
        if lib().jinc_debug_batch_set_registrars(self._h, int(n)) != 0:
            raise JincError(-1, lib().jinc_batch_last_error().decode())

    def refused(self) -> Tuple[int, str]:
        """Test header: (host ranges hipHostRegister refused so far, what the first one was told)."""
        buf = C.create_string_buffer(256)
        return int(lib().jinc_debug_batch_refused(self._h, buf, len(buf))), buf.value.decode()

    def device_cpus(self, device_index: int) -> List[int]:
        buf = (C.c_int * 4096)()
        n = int(lib().jinc_batch_device_cpus(self._h, int(device_index), buf, 4096))
        return [int(buf[i]) for i in range(max(0, min(n, 4096)))]

    def device_of_frame(self, n: int) -> int:
        return int(lib().jinc_batch_device_of_frame(self._h, int(n)))

    def out_dims(self) -> List[Tuple[int, int]]:
        return self.out_fmt.plane_dims(self.dst_w, self.dst_h)

    def process(self, frames: Sequence[Sequence[np.ndarray]], outs: Optional[Sequence[Sequence[np.ndarray]]] = None):
        """frames[n] = the planes of frame n (all with the same pitches); returns outs[n] = its output planes."""
        n, np_ = len(frames), self.fmt.planes
        if outs is None:
            outs = [[alloc_plane(w, h, self.fmt.dtype) for (w, h) in self.out_dims()] for _ in range(n)]
        sp, dp = (C.c_void_p * (4 * n))(), (C.c_void_p * (4 * n))()
        spitch, dpitch = _I4(), _I4()
        for k in range(n):
            for i in range(np_):
                sp[4 * k + i], dp[4 * k + i] = frames[k][i].ctypes.data, outs[k][i].ctypes.data
                if frames[k][i].strides[0] != frames[0][i].strides[0] or outs[k][i].strides[0] != outs[0][i].strides[0]:
                    raise ValueError("all frames of a batch must share their pitches")
        for i in range(np_):
            if n:
                spitch[i], dpitch[i] = frames[0][i].strides[0], outs[0][i].strides[0]
        rc = lib().jinc_batch_process(self._h, n, sp, spitch, dp, dpitch)
        if rc != 0:
            raise JincError(rc, lib().jinc_batch_last_error().decode())
        return outs

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().jinc_batch_free(self._h)
            self._h = C.c_void_p()

    __del__ = close


def shard_device(frame: int, ndevices: int) -> int:
    """Device of frame `frame` in a shard over `ndevices` devices (jinc_shard_device; needs no GPU)."""
    return int(lib().jinc_shard_device(int(frame), int(ndevices)))


class Filter:
    """One filter instance (= one `JincResize` object of the reference)."""

    def __init__(self, fmt: Format, width: int, height: int, target_width: int, target_height: int, *,
                 device: int = 0, frame0_chroma_location: int = -1, planar: bool = True,
                 cpu_flags: Tuple[bool, bool, bool] = (True, True, True), alias_taps: Optional[int] = None,
                 out_sub: Optional[Tuple[int, int]] = None, **kw):
        """out_sub=(w, h): the output's chroma sub-sampling (jinc_filter_create_out: 4:2:0 in, 4:4:4 out and the like); None: the
        input's (jinc_filter_create_ex).  `out_fmt` is the format of the planes the filter writes."""
        self.fmt = fmt
        vi, a, self._keep = _build_args(fmt, width, height, target_width, target_height, frame0_chroma_location, planar,
                                        cpu_flags, alias_taps, kw)
        self._h = C.c_void_p()
        err = C.create_string_buffer(512)
        if out_sub is None:
            rc = lib().jinc_filter_create_ex(C.byref(vi), C.byref(a), fmt.sample_type, int(device), C.byref(self._h), err, len(err))
        else:
            rc = lib().jinc_filter_create_out(C.byref(vi), C.byref(a), fmt.sample_type, int(out_sub[0]), int(out_sub[1]), int(device),
                                              C.byref(self._h), err, len(err))
        if rc != 0:
            raise JincError(rc, err.value.decode())
        out = VideoInfo()
        lib().jinc_filter_output_info(self._h, C.byref(out))
        self.out_fmt = _out_format(fmt, (out.sub_w, out.sub_h) if out_sub is not None else None)
        self.src_w, self.src_h = width, height
        self.dst_w, self.dst_h = out.width, out.height
        self.device = device

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().jinc_filter_free(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def _check(self, rc: int):
        if rc != 0:
            raise JincError(rc, lib().jinc_last_error().decode())

    @property
    def chroma_location(self) -> int:
        """What GetFrame writes to _ChromaLocation: 2 for every sub-sampled format (the reference binary's behaviour, ref
        :617-625 with d->cplace never assigned), -1 = not written; 0 / 1 / 2 by siting after set_chroma_location_mode(1)."""
        return int(lib().jinc_filter_chroma_location(self._h))

    def set_chroma_location_mode(self, mode: int) -> None:
        """0: as the reference binary (default); 1: by the siting in use (private switch, a deliberate deviation)."""
        self._check(lib().jinc_filter_set_chroma_location_mode(self._h, int(mode)))

    def out_dims(self) -> List[Tuple[int, int]]:
        return self.out_fmt.plane_dims(self.dst_w, self.dst_h)

    def set_kernel_mode(self, mode: int) -> None:
        self._check(lib().jinc_filter_set_kernel_mode(self._h, mode))

    def set_simd_order(self, order: int) -> None:
        """0: opt=0 results (default); 1 / 2 / 3: summation order of the reference's SSE4.1 / AVX2 / AVX-512 path."""
        self._check(lib().jinc_filter_set_simd_order(self._h, int(order)))

    def set_output_matrix(self, m=None, offset=None) -> None:
        """jinc_filter_set_output_matrix: every process_device* call hands its destination side o = M r + offset of the result planes
        0 .. 2 (nine row-major values, three offsets or None for zeros; each product and sum rounded to float32).  m=None clears it."""
        mm = None if m is None else (C.c_float * 9)(*[float(v) for v in np.asarray(m, dtype=np.float32).reshape(9)])
        self._check(lib().jinc_filter_set_output_matrix(self._h, mm, _three_floats(offset)))

    # -- GetFrame on host planes (H2D, kernels, D2H) --
    def get_frame(self, src_planes: Sequence[np.ndarray]) -> List[np.ndarray]:
        n = self.fmt.planes
        outs = [alloc_plane(w, h, self.fmt.dtype) for (w, h) in self.out_dims()]
        sp, spitch, dp, dpitch = _P4(), _I4(), _P4(), _I4()
        for i in range(n):
            s = src_planes[i]
            if s.dtype != self.fmt.dtype:
                raise TypeError("plane dtype does not match the clip format")
            sp[i], spitch[i] = s.ctypes.data, s.strides[0]
            dp[i], dpitch[i] = outs[i].ctypes.data, outs[i].strides[0]
        self._check(lib().jinc_filter_get_frame(self._h, sp, spitch, dp, dpitch))
        return outs

    # -- look-ahead pipeline: several frames in flight per instance --
    def set_pipeline(self, depth: int, register_host_buffers: int = 0, group: int = 0) -> None:
        """Up to `depth` frames in flight; `group` of them coalesced into one launch (0: automatic = depth / 2).
        register_host_buffers: PIN_NONE (0 / False: the CPU copies the planes through the library's pinned buffers), PIN_POOL (non-zero /
        True: pinned once and cached by address; the caller keeps the buffers allocated) or PIN_RUNTIME (3: handed to the runtime)."""
        self._check(lib().jinc_filter_set_pipeline_group(self._h, int(depth), int(group), int(register_host_buffers)))

    @property
    def pipeline_group(self) -> int:
        return int(lib().jinc_filter_pipeline_group(self._h))

    def adopt_host_range(self, base: int, nbytes: int) -> None:
        """[base, base + nbytes) is pinned by the caller (hipHostMalloc / hipHostRegister) and stays so until close() or
        release_host_range()."""
        self._check(lib().jinc_filter_adopt_host_range(self._h, C.c_void_p(base), C.c_size_t(nbytes)))

    def release_host_range(self, base: int, nbytes: int) -> None:
        """The caller is about to unpin / free the range: frames in flight are waited for, adopted ranges touching it are forgotten."""
        self._check(lib().jinc_filter_release_host_range(self._h, C.c_void_p(base), C.c_size_t(nbytes)))

    @property
    def direct_premise(self) -> int:
        return int(lib().jinc_filter_direct_premise(self._h))

    def flush(self) -> None:
        """Launch the frames submitted so far (a client that knows no more are coming)."""
        self._check(lib().jinc_filter_flush(self._h))

    def submit(self, src_planes: Sequence[np.ndarray], dst_planes: Sequence[np.ndarray]) -> int:
        """Enqueue one frame; dst_planes (from alloc_plane) are filled when wait(ticket) returns."""
        sp, spitch, dp, dpitch = _P4(), _I4(), _P4(), _I4()
        for i in range(self.fmt.planes):
            sp[i], spitch[i] = src_planes[i].ctypes.data, src_planes[i].strides[0]
            dp[i], dpitch[i] = dst_planes[i].ctypes.data, dst_planes[i].strides[0]
        t = C.c_longlong()
        self._check(lib().jinc_filter_submit(self._h, sp, spitch, dp, dpitch, C.byref(t)))
        return t.value

    def wait(self, ticket: int) -> None:
        self._check(lib().jinc_filter_wait(self._h, C.c_longlong(ticket)))

    # -- device-resident batch (pointers are raw device addresses) --
    def process_device(self, src_ptrs, src_pitches, src_strides, dst_ptrs, dst_pitches, dst_strides, nframes: int,
                       stream: int = 0) -> None:
        sp, spitch, ss, dp, dpitch, ds = _P4(), _I4(), _S4(), _P4(), _I4(), _S4()
        for i in range(self.fmt.planes):
            sp[i], spitch[i], ss[i] = src_ptrs[i], src_pitches[i], src_strides[i]
            dp[i], dpitch[i], ds[i] = dst_ptrs[i], dst_pitches[i], dst_strides[i]
        self._check(lib().jinc_filter_process_device(self._h, sp, spitch, ss, dp, dpitch, ds, int(nframes),
                                                     C.c_void_p(stream)))

    def process_device_strided(self, src_ptrs, src_pitches, src_steps, src_strides, dst_ptrs, dst_pitches, dst_steps, dst_strides,
                               nframes: int, stream: int = 0) -> None:
        """process_device on planes with a sample step (jinc_filter_process_device_strided): sample x of plane i lies x * step[i]
        samples behind the row's start.  NV12: U = uv, V = uv + 1 sample, both step 2; BGRA: B = p, G = p + 1, R = p + 2, A = p + 3, all
        step 4 (planes in the library's order G, B, R, A).  Steps and frame strides may be None (all ones; one frame).  The dense
        planes behind a call are capped by the knob strided_scratch_bytes."""
        n = self.fmt.planes

        def arr(kind, values):
            if values is None:
                return None
            a = kind()
            for i in range(n):
                a[i] = values[i]
            return a
        self._check(lib().jinc_filter_process_device_strided(
            self._h, arr(_P4, src_ptrs), arr(_I4, src_pitches), arr(_I4, src_steps), arr(_S4, src_strides), arr(_P4, dst_ptrs),
            arr(_I4, dst_pitches), arr(_I4, dst_steps), arr(_S4, dst_strides), int(nframes), C.c_void_p(stream)))

    def process_device_shifted(self, src_ptrs, src_pitches, src_steps, src_shifts, src_strides, dst_ptrs, dst_pitches, dst_steps,
                               dst_shifts, dst_strides, nframes: int, stream: int = 0) -> None:
        """process_device_strided on 16-bit words that keep their sample in the high bits (jinc_filter_process_device_shifted): a
        source sample's value is raw >> shift[i], a result is stored as value << shift[i].  P010: Y step 1, U and V step 2, all
        shift 6; P012: shift 4; Y210: Y step 2, U and V step 4, shift 6.  Steps, shifts and frame strides may be None."""
        n = self.fmt.planes

        def arr(kind, values):
            if values is None:
                return None
            a = kind()
            for i in range(n):
                a[i] = values[i]
            return a
        self._check(lib().jinc_filter_process_device_shifted(
            self._h, arr(_P4, src_ptrs), arr(_I4, src_pitches), arr(_I4, src_steps), arr(_I4, src_shifts), arr(_S4, src_strides),
            arr(_P4, dst_ptrs), arr(_I4, dst_pitches), arr(_I4, dst_steps), arr(_I4, dst_shifts), arr(_S4, dst_strides), int(nframes),
            C.c_void_p(stream)))

    def process_device_packed10(self, src_ptrs, src_pitches, src_offsets, src_strides, dst_ptrs, dst_pitches, dst_offsets, dst_fill,
                                dst_strides, nframes: int, stream: int = 0) -> None:
        """process_device on 10:10:10:2 words (jinc_filter_process_device_packed10): a side whose offsets are given is ONE buffer of
        32-bit words, one per pixel (element 0 of its pointers, pitches and strides), plane i's value is (word >> offsets[i]) & 1023;
        a side whose offsets are None is dense planes.  Stored words are the three results | (dst_fill & ~fields).  packed10_layout
        names the usual words.  Frame strides may be None (one frame)."""
        n = self.fmt.planes

        def arr(kind, values, count):
            if values is None:
                return None
            a = kind()
            for i in range(min(count, len(values))):
                a[i] = values[i]
            return a
        self._check(lib().jinc_filter_process_device_packed10(
            self._h, arr(_P4, src_ptrs, n), arr(_I4, src_pitches, n), arr(C.c_int * 3, src_offsets, 3), arr(_S4, src_strides, n),
            arr(_P4, dst_ptrs, n), arr(_I4, dst_pitches, n), arr(C.c_int * 3, dst_offsets, 3), C.c_uint(int(dst_fill) & 0xFFFFFFFF),
            arr(_S4, dst_strides, n), int(nframes), C.c_void_p(stream)))

    def process_device_v210(self, src_ptrs, src_pitches, src_is_v210, src_strides, dst_ptrs, dst_pitches, dst_is_v210, dst_strides,
                            nframes: int, stream: int = 0) -> None:
        """process_device on v210 frames (jinc_filter_process_device_v210; YUV422P10 filters): a side whose flag is set is ONE buffer
        of 16-byte blocks of six pixels (element 0 of its pointers, pitches and strides; a row is v210_row_bytes(width) bytes), a side
        whose flag is clear is dense planes.  Stored blocks have zeros in bits 30 - 31 and in the unused fields of a partial last
        block.  Frame strides may be None (one frame)."""
        n = self.fmt.planes

        def arr(kind, values):
            if values is None:
                return None
            a = kind()
            for i in range(min(n, len(values))):
                a[i] = values[i]
            return a
        self._check(lib().jinc_filter_process_device_v210(
            self._h, arr(_P4, src_ptrs), arr(_I4, src_pitches), int(bool(src_is_v210)), arr(_S4, src_strides), arr(_P4, dst_ptrs),
            arr(_I4, dst_pitches), int(bool(dst_is_v210)), arr(_S4, dst_strides), int(nframes), C.c_void_p(stream)))

    def process_device_widened(self, src_ptrs, src_pitches, src_steps, src_shifts, src_bits: int, src_strides, dst_ptrs, dst_pitches,
                               dst_steps, dst_strides, nframes: int, stream: int = 0) -> None:
        """INTEGER device samples into this fp32 / binary16 / bfloat16 filter (jinc_filter_process_device_widened): the source is addressed as in
        process_device_shifted, its sample size comes from src_bits (8: bytes; 9 .. 16: 16-bit words) and a sample's value is
        (raw >> shift[i]) & ((1 << src_bits) - 1); the destination side is process_device_strided's on this filter.  The result is
        process_device's on dense planes of those values as float / half.  NV12 into YUV420PS: Y step 1, U = uv, V = uv + 1
        sample, both step 2, src_bits 8; P010 into YUV420PH / PS: the same with src_bits 10, shifts 6.  Half filters take
        src_bits <= 11 and bfloat16 filters src_bits 8 only (NV12 into YUV420PBF, BGRA8 into RGBPBF): wider samples are not exact
        in those types and are refused.  Steps, shifts and frame strides may be None."""
        n = self.fmt.planes

        def arr(kind, values):
            if values is None:
                return None
            a = kind()
            for i in range(n):
                a[i] = values[i]
            return a
        self._check(lib().jinc_filter_process_device_widened(
            self._h, arr(_P4, src_ptrs), arr(_I4, src_pitches), arr(_I4, src_steps), arr(_I4, src_shifts), int(src_bits),
            arr(_S4, src_strides), arr(_P4, dst_ptrs), arr(_I4, dst_pitches), arr(_I4, dst_steps), arr(_S4, dst_strides), int(nframes),
            C.c_void_p(stream)))

    def process_device_widened_packed10(self, src_ptr: int, src_pitch: int, src_offsets, src_stride: int, dst_ptrs, dst_pitches, dst_steps,
                                        dst_strides, nframes: int, stream: int = 0) -> None:
        """10:10:10:2 words into this fp32 / binary16 filter (jinc_filter_process_device_widened_packed10; three components, no
        sub-sampling): the source is ONE buffer of 32-bit words, one per pixel, plane i's value is (word >> src_offsets[i]) & 1023
        (packed10_layout names the usual words); the destination side is process_device_strided's on this filter.  The result is
        process_device's on dense planes of those values as float / half.  Steps and frame strides may be None."""
        n = self.fmt.planes

        def arr(kind, values, count=n):
            if values is None:
                return None
            a = kind()
            for i in range(min(count, len(values))):
                a[i] = values[i]
            return a
        self._check(lib().jinc_filter_process_device_widened_packed10(
            self._h, C.c_void_p(src_ptr), int(src_pitch), arr(C.c_int * 3, src_offsets, 3), C.c_size_t(int(src_stride or 0)),
            arr(_P4, dst_ptrs), arr(_I4, dst_pitches), arr(_I4, dst_steps), arr(_S4, dst_strides), int(nframes), C.c_void_p(stream)))

    def process_device_widened_v210(self, src_ptr: int, src_pitch: int, src_stride: int, dst_ptrs, dst_pitches, dst_steps, dst_strides,
                                    nframes: int, stream: int = 0) -> None:
        """v210 blocks into this fp32 / binary16 4:2:2 filter (jinc_filter_process_device_widened_v210; YUV422PS, YUV422PH): the
        source is ONE buffer of 16-byte blocks of six pixels, a row is v210_row_bytes(width) bytes; the destination side is
        process_device_strided's on this filter.  The result is process_device's on dense planes of the field values as float /
        half.  Steps and frame strides may be None."""
        n = self.fmt.planes

        def arr(kind, values):
            if values is None:
                return None
            a = kind()
            for i in range(min(n, len(values))):
                a[i] = values[i]
            return a
        self._check(lib().jinc_filter_process_device_widened_v210(
            self._h, C.c_void_p(src_ptr), int(src_pitch), C.c_size_t(int(src_stride or 0)), arr(_P4, dst_ptrs), arr(_I4, dst_pitches),
            arr(_I4, dst_steps), arr(_S4, dst_strides), int(nframes), C.c_void_p(stream)))

    def process_device_widened_packed10_scaled(self, src_ptr: int, src_pitch: int, src_offsets, src_scales, src_offsets_add, src_stride: int,
                                               dst_ptrs, dst_pitches, dst_steps, dst_strides, nframes: int, stream: int = 0) -> None:
        """process_device_widened_packed10 with a scale and an offset per plane (jinc_filter_process_device_widened_packed10_scaled):
        plane i holds fl32(fl32(float((word >> src_offsets[i]) & 1023) * src_scales[i]) + src_offsets_add[i]), rounded to nearest even
        for half and bfloat16 filters -- bfloat16 filters are accepted here.  src_scales None means all 1.0, src_offsets_add None all
        0.0; both None IS process_device_widened_packed10.  code_range(10, ...) gives the usual pairs."""
        n = self.fmt.planes

        def arr(kind, values, count=n):
            if values is None:
                return None
            a = kind()
            for i in range(min(count, len(values))):
                a[i] = values[i]
            return a
        self._check(lib().jinc_filter_process_device_widened_packed10_scaled(
            self._h, C.c_void_p(src_ptr), int(src_pitch), arr(C.c_int * 3, src_offsets, 3), _three_floats(src_scales),
            _three_floats(src_offsets_add), C.c_size_t(int(src_stride or 0)), arr(_P4, dst_ptrs), arr(_I4, dst_pitches), arr(_I4, dst_steps),
            arr(_S4, dst_strides), int(nframes), C.c_void_p(stream)))

    def process_device_widened_v210_scaled(self, src_ptr: int, src_pitch: int, src_scales, src_offsets_add, src_stride: int, dst_ptrs,
                                           dst_pitches, dst_steps, dst_strides, nframes: int, stream: int = 0) -> None:
        """process_device_widened_v210 with a scale and an offset per plane (jinc_filter_process_device_widened_v210_scaled; planes
        Y, Cb, Cr): as process_device_widened_packed10_scaled, on 4:2:2 filters -- fp32, half and bfloat16."""
        n = self.fmt.planes

        def arr(kind, values):
            if values is None:
                return None
            a = kind()
            for i in range(min(n, len(values))):
                a[i] = values[i]
            return a
        self._check(lib().jinc_filter_process_device_widened_v210_scaled(
            self._h, C.c_void_p(src_ptr), int(src_pitch), _three_floats(src_scales), _three_floats(src_offsets_add),
            C.c_size_t(int(src_stride or 0)), arr(_P4, dst_ptrs), arr(_I4, dst_pitches), arr(_I4, dst_steps), arr(_S4, dst_strides),
            int(nframes), C.c_void_p(stream)))

    def process_device_narrowed(self, src_ptrs, src_pitches, src_steps, src_strides, dst_ptrs, dst_pitches, dst_steps, dst_shifts,
                                dst_bits: int, dst_strides, nframes: int, stream: int = 0) -> None:
        """This fp32 / binary16 / bfloat16 filter's results into INTEGER device samples (jinc_filter_process_device_narrowed): the
        source side is process_device_strided's on this filter; the destination is addressed as in process_device_shifted, its
        sample size comes from dst_bits (8: bytes; 9 .. 16: 16-bit words) and a stored sample is
        rint(clip(r, 0, 2^dst_bits - 1)) << shift[i] with r what process_device stores for the same source planes (NaN -> 0).  NV12
        from YUV420PS: Y step 1, U = uv, V = uv + 1 sample, both step 2, dst_bits 8; P010: the same with dst_bits 10, shifts 6;
        BGRA8 from RGBPS: G = p + 1, B = p, R = p + 2, step 4.  Steps, shifts and frame strides may be None."""
        n = self.fmt.planes

        def arr(kind, values):
            if values is None:
                return None
            a = kind()
            for i in range(n):
                a[i] = values[i]
            return a
        self._check(lib().jinc_filter_process_device_narrowed(
            self._h, arr(_P4, src_ptrs), arr(_I4, src_pitches), arr(_I4, src_steps), arr(_S4, src_strides), arr(_P4, dst_ptrs),
            arr(_I4, dst_pitches), arr(_I4, dst_steps), arr(_I4, dst_shifts), int(dst_bits), arr(_S4, dst_strides), int(nframes),
            C.c_void_p(stream)))

    def process_device_widened_scaled(self, src_ptrs, src_pitches, src_steps, src_shifts, src_bits: int, src_scales, src_offsets,
                                      src_strides, dst_ptrs, dst_pitches, dst_steps, dst_strides, nframes: int, stream: int = 0) -> None:
        """process_device_widened with a scale and an offset per plane (jinc_filter_process_device_widened_scaled): plane i holds
        fl32(fl32(float(value) * src_scales[i]) + src_offsets[i]), narrowed round-to-nearest-even for half and bfloat16 filters, which
        take every src_bits 8 .. 16 here.  src_scales None means all 1.0, src_offsets None all 0.0; both None IS
        process_device_widened.  code_range gives the usual pairs."""
        n = self.fmt.planes

        def arr(kind, values):
            if values is None:
                return None
            a = kind()
            for i in range(n):
                a[i] = values[i]
            return a
        self._check(lib().jinc_filter_process_device_widened_scaled(
            self._h, arr(_P4, src_ptrs), arr(_I4, src_pitches), arr(_I4, src_steps), arr(_I4, src_shifts), int(src_bits),
            arr(_F4, src_scales), arr(_F4, src_offsets), arr(_S4, src_strides), arr(_P4, dst_ptrs), arr(_I4, dst_pitches),
            arr(_I4, dst_steps), arr(_S4, dst_strides), int(nframes), C.c_void_p(stream)))

    def process_device_narrowed_scaled(self, src_ptrs, src_pitches, src_steps, src_strides, dst_ptrs, dst_pitches, dst_steps, dst_shifts,
                                       dst_bits: int, dst_scales, dst_offsets, dst_strides, nframes: int, stream: int = 0) -> None:
        """process_device_narrowed with a scale and an offset per plane (jinc_filter_process_device_narrowed_scaled): a stored sample
        is rint(clip(fl32(fl32(r * dst_scales[i]) + dst_offsets[i]), 0, 2^dst_bits - 1)) << shift[i].  dst_scales None means all 1.0,
        dst_offsets None all 0.0; both None IS process_device_narrowed.  code_range gives the usual pairs."""
        n = self.fmt.planes

        def arr(kind, values):
            if values is None:
                return None
            a = kind()
            for i in range(n):
                a[i] = values[i]
            return a
        self._check(lib().jinc_filter_process_device_narrowed_scaled(
            self._h, arr(_P4, src_ptrs), arr(_I4, src_pitches), arr(_I4, src_steps), arr(_S4, src_strides), arr(_P4, dst_ptrs),
            arr(_I4, dst_pitches), arr(_I4, dst_steps), arr(_I4, dst_shifts), int(dst_bits), arr(_F4, dst_scales), arr(_F4, dst_offsets),
            arr(_S4, dst_strides), int(nframes), C.c_void_p(stream)))

    def process_device_narrowed_packed10(self, src_ptrs, src_pitches, src_steps, src_strides, dst_ptr: int, dst_pitch: int, dst_offsets,
                                         dst_fill: int, dst_scales, dst_offsets_add, dst_stride: int, nframes: int, stream: int = 0) -> None:
        """This fp32 / binary16 / bfloat16 filter's results into 10:10:10:2 words (jinc_filter_process_device_narrowed_packed10; three
        components, no sub-sampling): the source side is process_device_strided's on this filter; the destination is ONE buffer of
        32-bit words, one per pixel, and a stored word is (v0 << dst_offsets[0]) | (v1 << dst_offsets[1]) | (v2 << dst_offsets[2]) |
        (dst_fill & ~fields) with v_i = rint(clip(fl32(fl32(r_i * dst_scales[i]) + dst_offsets_add[i]), 0, 1023)) and r_i what
        process_device stores (packed10_layout names the usual words).  dst_scales None means all 1.0, dst_offsets_add None all 0.0;
        steps and source frame strides may be None."""
        n = self.fmt.planes

        def arr(kind, values, count=n):
            if values is None:
                return None
            a = kind()
            for i in range(min(count, len(values))):
                a[i] = values[i]
            return a
        self._check(lib().jinc_filter_process_device_narrowed_packed10(
            self._h, arr(_P4, src_ptrs), arr(_I4, src_pitches), arr(_I4, src_steps), arr(_S4, src_strides), C.c_void_p(dst_ptr),
            int(dst_pitch), arr(C.c_int * 3, dst_offsets, 3), int(dst_fill) & 0xFFFFFFFF, arr(C.c_float * 3, dst_scales, 3),
            arr(C.c_float * 3, dst_offsets_add, 3), C.c_size_t(int(dst_stride or 0)), int(nframes), C.c_void_p(stream)))

    def process_device_narrowed_v210(self, src_ptrs, src_pitches, src_steps, src_strides, dst_ptr: int, dst_pitch: int, dst_scales,
                                     dst_offsets_add, dst_stride: int, nframes: int, stream: int = 0) -> None:
        """This fp32 / binary16 / bfloat16 4:2:2 filter's results into v210 blocks (jinc_filter_process_device_narrowed_v210;
        YUV422PS, YUV422PH, YUV422PBF): the source side is process_device_strided's on this filter; the destination is ONE buffer of
        16-byte blocks of six pixels, a row is v210_row_bytes(width) bytes, every field rint(clip(fl32(fl32(r * dst_scales[i]) +
        dst_offsets_add[i]), 0, 1023)) of its plane i.  dst_scales None means all 1.0, dst_offsets_add None all 0.0; steps and source
        frame strides may be None."""
        n = self.fmt.planes

        def arr(kind, values, count=n):
            if values is None:
                return None
            a = kind()
            for i in range(min(count, len(values))):
                a[i] = values[i]
            return a
        self._check(lib().jinc_filter_process_device_narrowed_v210(
            self._h, arr(_P4, src_ptrs), arr(_I4, src_pitches), arr(_I4, src_steps), arr(_S4, src_strides), C.c_void_p(dst_ptr),
            int(dst_pitch), arr(C.c_float * 3, dst_scales, 3), arr(C.c_float * 3, dst_offsets_add, 3), C.c_size_t(int(dst_stride or 0)),
            int(nframes), C.c_void_p(stream)))

    def process_device_shifted_packed10(self, src_ptrs, src_pitches, src_steps, src_shifts, src_strides, dst_ptr: int, dst_pitch: int,
                                        dst_offsets, dst_fill: int, dst_stride: int, nframes: int, stream: int = 0) -> None:
        """P010-style source planes (process_device_shifted's source side) into ONE buffer of 10:10:10:2 words (process_device_packed10's
        destination side) on a 10-bit integer filter whose output is 4:4:4 (jinc_filter_process_device_shifted_packed10)."""
        n = self.fmt.planes

        def arr(kind, values, count=n):
            if values is None:
                return None
            a = kind()
            for i in range(min(count, len(values))):
                a[i] = values[i]
            return a
        self._check(lib().jinc_filter_process_device_shifted_packed10(
            self._h, arr(_P4, src_ptrs), arr(_I4, src_pitches), arr(_I4, src_steps), arr(_I4, src_shifts), arr(_S4, src_strides),
            C.c_void_p(dst_ptr), int(dst_pitch), arr(C.c_int * 3, dst_offsets, 3), C.c_uint(dst_fill & 0xFFFFFFFF), C.c_size_t(int(dst_stride or 0)),
            int(nframes), C.c_void_p(stream)))

    def process_device_v210_packed10(self, src_ptr: int, src_pitch: int, src_stride: int, dst_ptr: int, dst_pitch: int, dst_offsets,
                                     dst_fill: int, dst_stride: int, nframes: int, stream: int = 0) -> None:
        """v210 blocks into ONE buffer of 10:10:10:2 words on a YUV422P10 filter whose output is 4:4:4
        (jinc_filter_process_device_v210_packed10)."""
        off = (C.c_int * 3)(*[int(o) for o in dst_offsets]) if dst_offsets is not None else None
        self._check(lib().jinc_filter_process_device_v210_packed10(
            self._h, C.c_void_p(src_ptr), int(src_pitch), C.c_size_t(int(src_stride or 0)), C.c_void_p(dst_ptr), int(dst_pitch), off,
            C.c_uint(dst_fill & 0xFFFFFFFF), C.c_size_t(int(dst_stride or 0)), int(nframes), C.c_void_p(stream)))

    def plane_extent_check(self, src_pitches, dst_pitches) -> None:
        """The limits every device call puts on its planes' extent (test header; works without a device): raises the refusal."""
        sp, dp = _I4(), _I4()
        for i in range(self.fmt.planes):
            sp[i], dp[i] = src_pitches[i], dst_pitches[i]
        self._check(lib().jinc_debug_plane_extent_check(self._h, sp, dp))

    last_strided = staticmethod(last_strided)
    last_groups = staticmethod(last_groups)
    strided_groups = staticmethod(strided_groups)

    def periodic_support(self, table: int = 0) -> int:
        """Taps per axis the periodic interior kernels execute (trimmed support on integer planes), 0: no periodic interior."""
        return int(lib().jinc_filter_periodic_support(self._h, int(table)))

    def periodic_taps(self, table: int = 0, rows_kernel=False) -> float:
        """Taps per output sample the periodic interior kernels execute (0: no periodic interior); rows_kernel: False / True = window
        and quad forms / rows kernel, 2 = the direct kernel's interior."""
        return float(lib().jinc_filter_periodic_taps(self._h, int(table), int(rows_kernel)))

    def interior_kernel(self, table: int = 0) -> str:
        return lib().jinc_filter_interior_kernel(self._h, int(table)).decode()

    def last_kernel(self, table: int = 0) -> str:
        """Interior kernel of the most recent frame call (depends on the batch size)."""
        return lib().jinc_filter_last_kernel(self._h, int(table)).decode()

    def last_border(self, table: int = 0) -> int:
        """Border kernels of the most recent frame call as bits (test header: jinc_filter_last_border)."""
        return int(lib().jinc_filter_last_border(self._h, int(table)))

    def last_instance(self, table: int = 0) -> str:
        """... with its template arguments, as rocprofv3 names it (the periodic family; the plain name otherwise)."""
        return lib().jinc_filter_last_instance(self._h, int(table)).decode()

    def last_finite_flags(self, plane: int = 0) -> Optional[np.ndarray]:
        """Float planes on the trimmed support: the flags the most recent frame call raised for `plane`, one uint32 per frame of that
        call (1: a non-finite sample was met and the frame was computed again on the full window); None when that plane's last launch
        did not take the flagged path (test header: jinc_filter_last_finite_flags).  Waits for the device."""
        n = int(lib().jinc_filter_last_finite_flags(self._h, int(plane), None, 0))
        if n < 0:
            self._check(n)
        if n == 0:
            return None
        out = np.zeros(n, np.uint32)
        self._check(min(int(lib().jinc_filter_last_finite_flags(self._h, int(plane), out.ctypes.data, n)), 0))
        return out

    def set_border_strips(self, mode) -> None:
        """Border frame of exactly periodic plans: -1 by call size (default), True/1 strip kernels, 2 rows only, False/0 gather kernel."""
        self._check(lib().jinc_filter_set_border_strips(self._h, int(mode)))

    def set_border_overlap(self, enable) -> None:
        """True / False, or None for the automatic choice."""
        self._check(lib().jinc_filter_set_border_overlap(self._h, -1 if enable is None else int(bool(enable))))

    def set_profiling(self, enable: bool) -> None:
        self._check(lib().jinc_filter_set_profiling(self._h, int(enable)))

    def kernel_times(self):
        """(periodic_ms, periodic_launches, gather_ms, gather_launches) since the last call."""
        pm, gm, pn, gn = C.c_double(), C.c_double(), C.c_int(), C.c_int()
        self._check(lib().jinc_filter_kernel_times(self._h, C.byref(pm), C.byref(pn), C.byref(gm), C.byref(gn)))
        return pm.value, pn.value, gm.value, gn.value

    def sync(self) -> None:
        self._check(lib().jinc_filter_sync(self._h))

    # -- plan introspection --
    @property
    def num_tables(self) -> int:
        return int(lib().jinc_filter_num_tables(self._h))

    def plan_info(self, table: int = 0) -> PlanInfo:
        info = PlanInfo()
        self._check(lib().jinc_filter_plan_info(self._h, table, C.byref(info)))
        return info

    def plan_dump(self, table: int = 0):
        info = self.plan_info(table)
        sx = np.zeros(info.dst_width, np.int32)
        sy = np.zeros(info.dst_height, np.int32)
        ids = np.zeros((info.dst_height, info.dst_width), np.int32)
        self._check(lib().jinc_filter_plan_dump(self._h, table, sx.ctypes.data, sy.ctypes.data, ids.ctypes.data))
        return sx, sy, ids

    def plan_runs(self, table: int = 0):
        """Rectangles of a drifting plan (what the runs form of the direct kernel walks): (array [n, 8] of set, x0, y0, sx0, sy0,
        ni, nj, first_item; number of items).  Empty for plans without runs.  Works without a device."""
        n, items = C.c_int(0), C.c_int(0)
        self._check(lib().jinc_filter_plan_runs(self._h, table, C.byref(n), C.byref(items), None, 0))
        runs = np.zeros((n.value, 8), np.int32)
        if n.value:
            self._check(lib().jinc_filter_plan_runs(self._h, table, C.byref(n), C.byref(items), runs.ctypes.data, n.value))
        return runs, items.value

    def plan_sets(self, table: int = 0) -> np.ndarray:
        info = self.plan_info(table)
        fs = info.filter_size
        out = np.zeros((info.num_sets, fs, fs), np.float32)
        for s in range(info.num_sets):
            self._check(lib().jinc_filter_plan_set(self._h, table, s, out[s].ctypes.data))
        return out

    def lut(self) -> np.ndarray:
        a = np.zeros(1024, np.float64)
        self._check(lib().jinc_filter_lut(self._h, a.ctypes.data))
        return a


# ---- script-level functions (ref JincResize.cpp:1044-1108) ---------------------------------------
def _make(clip: Clip, target_width: int, target_height: int, device: int, alias_taps: Optional[int], **kw) -> Clip:
    cl = clip.props.get("_ChromaLocation", -1)
    flt = Filter(clip.fmt, clip.width, clip.height, target_width, target_height, device=device,
                 frame0_chroma_location=cl if isinstance(cl, int) else -1, planar=clip.planar,
                 alias_taps=alias_taps, **kw)
    props = dict(clip.props)
    if flt.chroma_location >= 0:
        props["_ChromaLocation"] = flt.chroma_location  # ref :617-625

    out = Clip(clip.fmt, flt.dst_w, flt.dst_h, clip.num_frames, lambda n: flt.get_frame(clip.get_frame(n)), props)
    out.filter = flt
    return out


def JincResize(clip: Clip, target_width: int, target_height: int, src_left=None, src_top=None, src_width=None,
               src_height=None, quant_x=None, quant_y=None, tap=None, blur=None, cplace=None, threads=None, opt=None,
               initial_capacity=None, initial_factor=None, *, device: int = 0) -> Clip:
    return _make(clip, target_width, target_height, device, None, src_left=src_left, src_top=src_top,
                 src_width=src_width, src_height=src_height, quant_x=quant_x, quant_y=quant_y, tap=tap, blur=blur,
                 cplace=cplace, threads=threads, opt=opt, initial_capacity=initial_capacity,
                 initial_factor=initial_factor)


def _alias(taps: int):
    def fn(clip: Clip, target_width: int, target_height: int, src_left=None, src_top=None, src_width=None,
           src_height=None, quant_x=None, quant_y=None, cplace=None, threads=None, *, device: int = 0) -> Clip:
        return _make(clip, target_width, target_height, device, taps, src_left=src_left, src_top=src_top,
                     src_width=src_width, src_height=src_height, quant_x=quant_x, quant_y=quant_y, cplace=cplace,
                     threads=threads)
    return fn


Jinc36Resize = _alias(3)
Jinc64Resize = _alias(4)
Jinc144Resize = _alias(6)
Jinc256Resize = _alias(8)
