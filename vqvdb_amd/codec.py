"""Host-side mirror of the reference's codec interface over the C ABI of libvqvdb_hip.so.

Mirrors src/core/IVQVAECodec.hpp (``BackendType``, ``DataType``, ``TensorView``, ``Tensor``,
``CodecConfig``, ``IVQVAECodec.create/encode/decode/getLatentShape``) with the same names,
argument meaning and error behaviour, so the parity tests read like the reference's call
sites (src/orchestrator/VQVAECodec.cpp:108-127,166-196).  The C++ adapter a maintainer would
compile into the reference tree is include/vqvdb_hip_backend.hpp; this module is the same
thing for Python callers, tests and bench.py.

There is NO CPU fallback: if the shared library or a gfx950 device is missing, ``create``
reports the failure and returns ``None`` exactly like the reference factory
(src/core/IVQVAECodec.cpp:106-109), and ``HipCodec`` raises.
"""
from __future__ import annotations

import ctypes
import enum
import os
import sys
from dataclasses import dataclass, field
from typing import Optional, Sequence, Union

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvqvdb_hip.so")

LEAF_VOXELS = 512
LATENT_VOXELS = 64


class BackendType(enum.Enum):   # IVQVAECodec.hpp:21, HIP appended (existing values unchanged)
    LibTorch = 0
    ONNX = 1
    HIP = 2


class DataType(enum.Enum):      # IVQVAECodec.hpp:38-41
    FLOAT32 = 0
    UINT8 = 1


class EmbeddedModel:            # IVQVAECodec.hpp:27
    pass


EMBEDDED_PACK_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "embedded_model.vqw")


@dataclass
class TensorView:               # IVQVAECodec.hpp:49-53 — non-owning view of host data
    data: np.ndarray
    shape: Sequence[int]
    dtype: DataType


@dataclass
class Tensor:                   # IVQVAECodec.hpp:61-80 — owning result
    buffer: np.ndarray          # flat uint8 bytes
    shape: list
    dtype: DataType

    def getData(self) -> np.ndarray:
        t = np.float32 if self.dtype == DataType.FLOAT32 else np.uint8
        return self.buffer.view(t).reshape(self.shape)


@dataclass
class CodecConfig:              # IVQVAECodec.hpp:85-89
    class Device(enum.Enum):
        CPU = 0
        CUDA = 1                # read as "GPU": the HIP backend only accepts this value

    device: "CodecConfig.Device" = None
    source: Union[EmbeddedModel, str, os.PathLike, bytes] = field(default_factory=EmbeddedModel)
    device_id: int = 0          # extension: HIP device ordinal (reference hard-codes 0, OnnxBackend_Cuda.cpp:21)

    def __post_init__(self):
        if self.device is None:
            self.device = CodecConfig.Device.CPU


class _KernelStat(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 48), ("launches", ctypes.c_int64), ("total_ms", ctypes.c_double),
                ("flops_per_leaf", ctypes.c_double), ("eff_flops_per_leaf", ctypes.c_double), ("leaves", ctypes.c_int64)]


# every symbol include/vqvdb_hip.h declares
ABI_SYMBOLS = [
    "vqhip_create", "vqhip_destroy", "vqhip_last_error", "vqhip_latent_shape", "vqhip_encode", "vqhip_decode",
    "vqhip_encode_device", "vqhip_decode_device", "vqhip_encode_leaves", "vqhip_decode_leaves", "vqhip_set_chunk_leaves", "vqhip_profile_enable",
    "vqhip_profile_read", "vqhip_debug_enable", "vqhip_debug_fetch", "vqhip_selftest_mfma", "vqhip_version",
    "vqhip_multi_create", "vqhip_multi_destroy", "vqhip_multi_last_error", "vqhip_multi_encode", "vqhip_multi_decode",
    "vqhip_decompress_file", "vqhip_compress_file", "vqhip_reserve",
    "vqhip_train_begin", "vqhip_train_vq_stats_device", "vqhip_train_vq_update_device", "vqhip_train_get_state", "vqhip_train_set_state",
    "vqhip_train_commit", "vqhip_set_small_batch_tiles", "vqhip_train_eval_device",
    "vqhip_fulltrain_begin", "vqhip_fulltrain_param_count", "vqhip_fulltrain_forward_device", "vqhip_fulltrain_fwdbwd_device",
    "vqhip_fulltrain_apply_device", "vqhip_fulltrain_get_params", "vqhip_fulltrain_set_params",
    "vqhip_fulltrain_get_opt_state", "vqhip_fulltrain_set_opt_state", "vqhip_workspace_bytes", "vqhip_chunk_leaves", "vqhip_multi_worker_info", "vqhip_fulltrain_fwdbwd_overlap_device", "vqhip_fulltrain_decoder_offset", "vqhip_fulltrain_ready_stream", "vqhip_fulltrain_set_folded_tail",
    "vqhip_compute_units",
    "vqhip_vec3_create", "vqhip_vec3_destroy", "vqhip_vec3_last_error", "vqhip_vec3_model_info", "vqhip_vec3_encode", "vqhip_vec3_decode",
    "vqhip_vec3_encode_device", "vqhip_vec3_decode_device", "vqhip_vec3_set_chunk_leaves", "vqhip_vec3_chunk_leaves",
    "vqhip_vec3_debug_enable", "vqhip_vec3_debug_fetch",
]

# every symbol include/vqvdb_hip_vec3_train.h declares (Vec3 codebook training; kept apart from ABI_SYMBOLS)
VEC3_TRAIN_SYMBOLS = [
    "vqhip_vec3_train_stats_floats", "vqhip_vec3_train_begin", "vqhip_vec3_train_vq_stats_device", "vqhip_vec3_train_eval_device",
    "vqhip_vec3_train_vq_update_device", "vqhip_vec3_train_get_state", "vqhip_vec3_train_set_state",
]

# every symbol include/vqvdb_hip_vec3_fulltrain.h declares (Vec3 full training; kept apart from both lists above)
VEC3_FULLTRAIN_SYMBOLS = [
    "vqhip_vec3_fulltrain_param_count", "vqhip_vec3_fulltrain_decoder_offset", "vqhip_vec3_fulltrain_aux_floats",
    "vqhip_vec3_fulltrain_begin", "vqhip_vec3_fulltrain_fwdbwd_device", "vqhip_vec3_fulltrain_forward_device",
    "vqhip_vec3_fulltrain_apply_device", "vqhip_vec3_fulltrain_get_params", "vqhip_vec3_fulltrain_set_params",
    "vqhip_vec3_fulltrain_get_opt_state", "vqhip_vec3_fulltrain_set_opt_state",
]
# every symbol include/vqvdb_hip_vec3_precision.h declares (Vec3 inference precision mode; kept apart from the lists above)
VEC3_PRECISION_SYMBOLS = ["vqhip_vec3_set_precision", "vqhip_vec3_get_precision"]
VEC3_PRECISIONS = {"fp32": 0, "bf16": 1}   # VQHIP_VEC3_PRECISION_*
# every symbol include/vqvdb_hip_precision.h declares (decode precision mode of the scalar handle; kept apart from the lists above)
PRECISION_SYMBOLS = ["vqhip_set_decode_mode", "vqhip_get_decode_mode"]
PRECISIONS = {"fp32": 0, "bf16": 1}   # VQHIP_PRECISION_*
# every symbol include/vqvdb_hip_encode_mode.h declares (encode operand mode of the scalar handle; the values are PRECISIONS)
ENCODE_MODE_SYMBOLS = ["vqhip_set_encode_mode", "vqhip_get_encode_mode"]
# every symbol include/vqvdb_hip_vec3_bounded.h declares (Vec3 error-bounded round trip; kept apart from the lists above)
VEC3_BOUNDED_SYMBOLS = ["vqhip_vec3_roundtrip_device", "vqhip_vec3_select_outliers_device", "vqhip_vec3_compress_bounded"]
VEC3_ERR_FLOATS = 2   # VQHIP_VEC3_ERR_FLOATS: per leaf max |x - x^|, sum (x - x^)^2
# every symbol include/vqvdb_hip_vec3_residual.h declares (quantised residuals of the Vec3 handle; kept apart from the lists above)
VEC3_RESIDUAL_SYMBOLS = ["vqhip_vec3_residual_encode_device", "vqhip_vec3_residual_apply_device", "vqhip_vec3_residual_compress",
                         "vqhip_vec3_residual_decompress"]
VEC3_RES_KEPT, VEC3_RES_RAW = 0xFFFE, 0xFFFF   # VQHIP_VEC3_RES_KEPT, VQHIP_VEC3_RES_RAW
# every symbol include/vqvdb_hip_vec3_rate.h declares (size sweep and byte-budget compress of the Vec3 handle; kept apart from the lists above)
VEC3_RATE_SYMBOLS = ["vqhip_vec3_rate_payload_bytes", "vqhip_vec3_rate_sweep_device", "vqhip_vec3_rate_sweep", "vqhip_vec3_rate_compress",
                     "vqhip_vec3_rate_pick"]
# VQHIP_VEC3_RATE_MAX_TOLS, VQHIP_VEC3_RATE_CLASSES: columns 0 .. 48 quantised by b0 + b1 + b2, 49 raw, 50 kept
VEC3_RATE_MAX_TOLS, VEC3_RATE_CLASSES = 64, 51

# every symbol include/vqvdb_hip_bounded.h declares (error-bounded compression on the scalar handle; kept apart from the lists above)
BOUNDED_SYMBOLS = ["vqhip_roundtrip_device", "vqhip_select_outliers_device", "vqhip_compress_bounded", "vqhip_decompress_bounded",
                   "vqhip_compress_file_bounded", "vqhip_decompress_file_bounded"]
# every symbol include/vqvdb_hip_residual.h declares (quantised residuals of the scalar handle; kept apart from the lists above)
RESIDUAL_SYMBOLS = ["vqhip_residual_encode_device", "vqhip_residual_apply_device", "vqhip_compress_residual", "vqhip_decompress_residual",
                    "vqhip_compress_file_residual", "vqhip_decompress_file_residual"]
RES_KEPT, RES_RAW = 254, 255   # VQHIP_RES_KEPT, VQHIP_RES_RAW
# every symbol include/vqvdb_hip_rate.h declares (size sweep and byte-budget compress of the scalar handle; kept apart from the lists above)
RATE_SYMBOLS = ["vqhip_rate_payload_bytes", "vqhip_rate_sidecar_bytes", "vqhip_rate_sweep_device", "vqhip_rate_sweep", "vqhip_rate_sweep_file",
                "vqhip_rate_compress_file"]
RATE_MAX_TOLS, RATE_CLASSES = 64, 19   # VQHIP_RATE_MAX_TOLS, VQHIP_RATE_CLASSES: columns 0 .. 16 quantised, 17 raw, 18 kept
ERR_FLOATS = 2   # VQHIP_ERR_FLOATS: per leaf max |x - x^|, sum (x - x^)^2
# every symbol include/vqvdb_hip_vec3_mask.h declares (active-voxel masks of the Vec3 handle's residual codec; kept apart from the lists above)
VEC3_MASK_SYMBOLS = ["vqhip_vec3_mask_leaf_err_device", "vqhip_vec3_mask_residual_encode_device", "vqhip_vec3_mask_sweep_device",
                     "vqhip_vec3_mask_compress_residual", "vqhip_vec3_mask_sweep"]
MASK_WORDS = 8   # VQHIP_VEC3_MASK_WORDS: uint64 words of one leaf's mask, bit L of word j = voxel 64 j + L
# every symbol include/vqvdb_hip_vec3_active.h declares (records that hold only the active voxels; kept apart from the lists above)
VEC3_ACTIVE_SYMBOLS = ["vqhip_vec3_active_record_bytes", "vqhip_vec3_active_encode_device", "vqhip_vec3_active_apply_device",
                       "vqhip_vec3_active_sweep_device", "vqhip_vec3_active_compress", "vqhip_vec3_active_decompress",
                       "vqhip_vec3_active_sweep"]
# every symbol include/vqvdb_hip_vec3_file.h declares (leaf-pointer calls and the .vqv3 container of the Vec3 handle; kept apart from the lists above)
VEC3_FILE_SYMBOLS = ["vqhip_vec3_encode_leaves", "vqhip_vec3_decode_leaves", "vqhip_vec3_file_compress", "vqhip_vec3_file_compress_active",
                     "vqhip_vec3_file_decompress", "vqhip_vec3_file_info"]
# every symbol include/vqvdb_hip_vec3_budget.h declares (byte-budget compress on compact records, in memory and into a .vqv3 file; kept
# apart from the lists above)
VEC3_BUDGET_SYMBOLS = ["vqhip_vec3_budget_pick", "vqhip_vec3_budget_file_bytes", "vqhip_vec3_budget_compress", "vqhip_vec3_budget_file_sweep",
                       "vqhip_vec3_budget_file_compress"]
VEC3_LEAF_FLOATS = 1536   # one Vec3f leaf buffer: [512][3] float32

_VEC3_FULLTRAIN_I64 = ("vqhip_vec3_fulltrain_param_count", "vqhip_vec3_fulltrain_decoder_offset", "vqhip_vec3_fulltrain_aux_floats")


class _GridInfo(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("transform", ctypes.c_float * 16), ("latent_shape", ctypes.c_int64 * 3),
                ("num_embeddings", ctypes.c_uint32), ("total_blocks", ctypes.c_uint64), ("grid_index", ctypes.c_int)]


class StreamStats(ctypes.Structure):
    """vqhip_stream_stats: where a whole-file compress/decompress spent its time."""
    _fields_ = [("leaves", ctypes.c_int64), ("grids", ctypes.c_int32), ("wall_s", ctypes.c_double), ("read_s", ctypes.c_double),
                ("alloc_s", ctypes.c_double), ("copy_s", ctypes.c_double), ("io_wait_s", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class BoundedStats(ctypes.Structure):
    """vqhip_bounded_stats: what a bounded whole-file compress kept and what it stored raw."""
    _fields_ = [("leaves", ctypes.c_int64), ("outliers", ctypes.c_int64), ("max_err_kept", ctypes.c_float), ("sum_sq_kept", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ResidualStats(ctypes.Structure):
    """vqhip_residual_stats: how a residual whole-file compress stored the leaves it selected."""
    _fields_ = [("quantised", ctypes.c_int64), ("raw", ctypes.c_int64), ("payload_bytes", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class _GridSource(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("transform", ctypes.POINTER(ctypes.c_float)), ("leaf_ptrs", ctypes.c_void_p),
                ("origins", ctypes.c_void_p), ("n_leaves", ctypes.c_int64)]


class _Vec3GridSource(ctypes.Structure):
    """vqhip_vec3_grid_source"""
    _fields_ = [("name", ctypes.c_char_p), ("transform", ctypes.c_void_p), ("leaf_ptrs", ctypes.c_void_p), ("origins", ctypes.c_void_p),
                ("n_leaves", ctypes.c_int64), ("masks", ctypes.c_void_p), ("background", ctypes.c_void_p)]


class _Vec3GridInfo(ctypes.Structure):
    """vqhip_vec3_grid_info"""
    _fields_ = [("name", ctypes.c_char_p), ("transform", ctypes.c_float * 16), ("num_codes", ctypes.c_uint32), ("total_blocks", ctypes.c_uint64),
                ("grid_index", ctypes.c_int), ("kind", ctypes.c_int), ("mode", ctypes.c_int), ("tol", ctypes.c_float),
                ("has_background", ctypes.c_int), ("background", ctypes.c_float * 3)]


VEC3_GRID_BEGIN_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(_Vec3GridInfo))
VEC3_LEAF_ALLOC_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64),
                                      ctypes.c_int64, ctypes.POINTER(ctypes.c_void_p))
GRID_BEGIN_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(_GridInfo))
LEAF_ALLOC_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_int64,
                                 ctypes.POINTER(ctypes.c_void_p))

PHASE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p)

_lib = None


def load_library() -> ctypes.CDLL:
    """dlopen libvqvdb_hip.so (built in-tree by ``python -m vqvdb_amd.build``) and type its ABI."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -m vqvdb_amd.build` (no CPU fallback exists)")
    lib = ctypes.CDLL(LIB_PATH)
    vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.vqhip_create.argtypes = [ctypes.c_char_p, vp, ctypes.c_size_t, ci, ctypes.POINTER(vp)]
    lib.vqhip_destroy.argtypes = [vp]
    lib.vqhip_destroy.restype = None
    lib.vqhip_last_error.argtypes = [vp]
    lib.vqhip_last_error.restype = ctypes.c_char_p
    lib.vqhip_latent_shape.argtypes = [vp, ctypes.POINTER(i64)]
    lib.vqhip_encode.argtypes = [vp, vp, i64, vp]
    lib.vqhip_decode.argtypes = [vp, vp, i64, vp]
    lib.vqhip_encode_device.argtypes = [vp, vp, i64, vp, vp]
    lib.vqhip_decode_device.argtypes = [vp, vp, i64, vp, vp]
    lib.vqhip_encode_leaves.argtypes = [vp, vp, i64, vp]
    lib.vqhip_decode_leaves.argtypes = [vp, vp, i64, vp]
    lib.vqhip_set_chunk_leaves.argtypes = [vp, i64]
    lib.vqhip_reserve.argtypes = [vp, i64]
    lib.vqhip_set_small_batch_tiles.argtypes = [vp, ci]
    lib.vqhip_train_begin.argtypes = [vp, vp, vp]
    lib.vqhip_train_vq_stats_device.argtypes = [vp, vp, i64, vp, vp, vp, vp]
    lib.vqhip_train_vq_update_device.argtypes = [vp, vp, ctypes.c_float, ctypes.c_float, vp]
    lib.vqhip_train_eval_device.argtypes = [vp, vp, i64, vp, vp, vp, vp]
    lib.vqhip_train_get_state.argtypes = [vp, vp, vp, vp]
    lib.vqhip_train_set_state.argtypes = [vp, vp, vp, vp]
    lib.vqhip_train_commit.argtypes = [vp]
    lib.vqhip_fulltrain_begin.argtypes = [vp]
    lib.vqhip_fulltrain_param_count.argtypes = [vp]
    lib.vqhip_fulltrain_param_count.restype = i64
    lib.vqhip_fulltrain_forward_device.argtypes = [vp, vp, i64, vp]
    lib.vqhip_fulltrain_fwdbwd_device.argtypes = [vp, vp, i64, i64, vp, vp, vp]
    cf = ctypes.c_float
    lib.vqhip_fulltrain_apply_device.argtypes = [vp, vp, vp, cf, i64, cf, cf, cf, cf, cf, cf, vp]
    lib.vqhip_fulltrain_get_params.argtypes = [vp, vp]
    lib.vqhip_fulltrain_set_params.argtypes = [vp, vp]
    lib.vqhip_multi_worker_info.argtypes = [vp, ci, ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ci)]
    lib.vqhip_fulltrain_fwdbwd_overlap_device.argtypes = [vp, vp, i64, i64, vp, vp, vp, PHASE_FN, vp]
    lib.vqhip_fulltrain_set_folded_tail.argtypes = [vp, ci]
    lib.vqhip_fulltrain_decoder_offset.argtypes = [vp]
    lib.vqhip_fulltrain_decoder_offset.restype = ctypes.c_int64
    lib.vqhip_fulltrain_ready_stream.argtypes = [vp]
    lib.vqhip_fulltrain_ready_stream.restype = ctypes.c_void_p
    lib.vqhip_workspace_bytes.argtypes = [vp]
    lib.vqhip_workspace_bytes.restype = ctypes.c_int64
    lib.vqhip_chunk_leaves.argtypes = [vp]
    lib.vqhip_chunk_leaves.restype = ctypes.c_int64
    lib.vqhip_compute_units.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    lib.vqhip_fulltrain_get_opt_state.argtypes = [vp, vp, vp]
    lib.vqhip_fulltrain_set_opt_state.argtypes = [vp, vp, vp]
    lib.vqhip_profile_enable.argtypes = [vp, ci]
    lib.vqhip_profile_read.argtypes = [vp, ctypes.POINTER(_KernelStat), ci, ctypes.POINTER(ci)]
    lib.vqhip_debug_enable.argtypes = [vp, ci]
    lib.vqhip_debug_fetch.argtypes = [vp, ctypes.c_char_p, i64, vp]
    lib.vqhip_selftest_mfma.argtypes = [vp, ctypes.POINTER(i64)]
    lib.vqhip_version.restype = ctypes.c_char_p
    lib.vqhip_multi_create.argtypes = [ctypes.c_char_p, vp, ctypes.c_size_t, ctypes.POINTER(ci), ci, ctypes.POINTER(vp)]
    lib.vqhip_multi_destroy.argtypes = [vp]
    lib.vqhip_multi_destroy.restype = None
    lib.vqhip_multi_last_error.argtypes = [vp]
    lib.vqhip_multi_last_error.restype = ctypes.c_char_p
    lib.vqhip_multi_encode.argtypes = [vp, vp, i64, vp]
    lib.vqhip_multi_decode.argtypes = [vp, vp, i64, vp]
    lib.vqhip_decompress_file.argtypes = [vp, ctypes.c_char_p, i64, GRID_BEGIN_FN, LEAF_ALLOC_FN, vp, ctypes.POINTER(StreamStats)]
    lib.vqhip_compress_file.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(_GridSource), ci, i64, ctypes.POINTER(StreamStats)]
    lib.vqhip_vec3_create.argtypes = [ctypes.c_char_p, vp, ctypes.c_size_t, ci, ctypes.POINTER(vp)]
    lib.vqhip_vec3_destroy.argtypes = [vp]
    lib.vqhip_vec3_destroy.restype = None
    lib.vqhip_vec3_last_error.argtypes = [vp]
    lib.vqhip_vec3_last_error.restype = ctypes.c_char_p
    lib.vqhip_vec3_model_info.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i64)]
    lib.vqhip_vec3_encode.argtypes = [vp, vp, i64, vp]
    lib.vqhip_vec3_decode.argtypes = [vp, vp, i64, vp]
    lib.vqhip_vec3_encode_device.argtypes = [vp, vp, i64, vp, vp]
    lib.vqhip_vec3_decode_device.argtypes = [vp, vp, i64, vp, vp]
    lib.vqhip_vec3_set_chunk_leaves.argtypes = [vp, i64]
    lib.vqhip_vec3_chunk_leaves.argtypes = [vp]
    lib.vqhip_vec3_chunk_leaves.restype = i64
    lib.vqhip_vec3_debug_enable.argtypes = [vp, ci]
    lib.vqhip_vec3_debug_fetch.argtypes = [vp, ctypes.c_char_p, i64, vp]
    # include/vqvdb_hip_vec3_train.h
    lib.vqhip_vec3_train_stats_floats.argtypes = [vp]
    lib.vqhip_vec3_train_stats_floats.restype = i64
    lib.vqhip_vec3_train_begin.argtypes = [vp, vp, vp]
    lib.vqhip_vec3_train_vq_stats_device.argtypes = [vp, vp, i64, vp, vp, vp, vp]
    lib.vqhip_vec3_train_eval_device.argtypes = [vp, vp, i64, vp, vp, vp, vp]
    lib.vqhip_vec3_train_vq_update_device.argtypes = [vp, vp, ctypes.c_float, ctypes.c_float, vp]
    lib.vqhip_vec3_train_get_state.argtypes = [vp, vp, vp, vp]
    lib.vqhip_vec3_train_set_state.argtypes = [vp, vp, vp, vp]
    # include/vqvdb_hip_vec3_fulltrain.h
    for name in _VEC3_FULLTRAIN_I64:
        getattr(lib, name).argtypes = [vp]
        getattr(lib, name).restype = i64
    lib.vqhip_vec3_fulltrain_begin.argtypes = [vp]
    lib.vqhip_vec3_fulltrain_fwdbwd_device.argtypes = [vp, vp, i64, i64, vp, vp, vp, vp]
    lib.vqhip_vec3_fulltrain_forward_device.argtypes = [vp, vp, i64, vp, vp, vp]
    lib.vqhip_vec3_fulltrain_apply_device.argtypes = [vp, vp, vp, cf, i64, cf, cf, cf, cf, cf, cf, vp]
    lib.vqhip_vec3_fulltrain_get_params.argtypes = [vp, vp]
    lib.vqhip_vec3_fulltrain_set_params.argtypes = [vp, vp]
    lib.vqhip_vec3_fulltrain_get_opt_state.argtypes = [vp, vp, vp]
    lib.vqhip_vec3_fulltrain_set_opt_state.argtypes = [vp, vp, vp]
    # include/vqvdb_hip_vec3_precision.h
    lib.vqhip_vec3_set_precision.argtypes = [vp, ci]
    lib.vqhip_vec3_get_precision.argtypes = [vp, vp]
    for name in VEC3_PRECISION_SYMBOLS:
        getattr(lib, name).restype = ci
    # include/vqvdb_hip_precision.h
    lib.vqhip_set_decode_mode.argtypes = [vp, ci]
    lib.vqhip_get_decode_mode.argtypes = [vp, vp]
    for name in PRECISION_SYMBOLS:
        getattr(lib, name).restype = ci
    # include/vqvdb_hip_encode_mode.h
    lib.vqhip_set_encode_mode.argtypes = [vp, ci]
    lib.vqhip_get_encode_mode.argtypes = [vp, vp]
    for name in ENCODE_MODE_SYMBOLS:
        getattr(lib, name).restype = ci
    # include/vqvdb_hip_vec3_bounded.h
    lib.vqhip_vec3_roundtrip_device.argtypes = [vp, vp, i64, vp, vp, vp, vp]
    lib.vqhip_vec3_select_outliers_device.argtypes = [vp, vp, i64, cf, vp, vp, vp]
    lib.vqhip_vec3_compress_bounded.argtypes = [vp, vp, i64, cf, vp, vp, vp, vp]
    for name in VEC3_BOUNDED_SYMBOLS:
        getattr(lib, name).restype = ci
    # include/vqvdb_hip_vec3_residual.h
    lib.vqhip_vec3_residual_encode_device.argtypes = [vp, vp, vp, vp, i64, cf, vp, vp, vp, i64, vp]
    lib.vqhip_vec3_residual_apply_device.argtypes = [vp, vp, i64, cf, vp, vp, vp, vp]
    lib.vqhip_vec3_residual_compress.argtypes = [vp, vp, i64, cf, vp, vp, vp, vp, vp]
    lib.vqhip_vec3_residual_decompress.argtypes = [vp, vp, i64, cf, vp, vp, i64, vp]
    for name in VEC3_RESIDUAL_SYMBOLS:
        getattr(lib, name).restype = ci
    # include/vqvdb_hip_vec3_rate.h
    lib.vqhip_vec3_rate_payload_bytes.argtypes = [vp]
    lib.vqhip_vec3_rate_sweep_device.argtypes = [vp, vp, vp, vp, i64, vp, ci, vp, vp]
    lib.vqhip_vec3_rate_sweep.argtypes = [vp, vp, i64, vp, ci, vp]
    lib.vqhip_vec3_rate_compress.argtypes = [vp, vp, i64, vp, ci, i64, vp, vp, vp, vp, vp, vp, vp]
    lib.vqhip_vec3_rate_pick.argtypes = [vp, vp, ci, i64]
    for name in VEC3_RATE_SYMBOLS:
        getattr(lib, name).restype = i64 if name.endswith("_bytes") else ci
    # include/vqvdb_hip_bounded.h
    lib.vqhip_roundtrip_device.argtypes = [vp, vp, i64, vp, vp, vp, vp]
    lib.vqhip_select_outliers_device.argtypes = [vp, vp, i64, cf, vp, vp, vp]
    lib.vqhip_compress_bounded.argtypes = [vp, vp, i64, cf, vp, vp, vp, vp]
    lib.vqhip_decompress_bounded.argtypes = [vp, vp, i64, vp, i64, vp, vp]
    lib.vqhip_compress_file_bounded.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(_GridSource), ci, i64, cf,
                                                ctypes.POINTER(StreamStats), ctypes.POINTER(BoundedStats)]
    lib.vqhip_decompress_file_bounded.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, i64, GRID_BEGIN_FN, LEAF_ALLOC_FN, vp, ctypes.POINTER(StreamStats)]
    for name in BOUNDED_SYMBOLS:
        getattr(lib, name).restype = ci
    # include/vqvdb_hip_residual.h
    lib.vqhip_residual_encode_device.argtypes = [vp, vp, vp, vp, i64, cf, vp, vp, vp, i64, vp]
    lib.vqhip_residual_apply_device.argtypes = [vp, vp, i64, cf, vp, vp, vp, vp]
    lib.vqhip_compress_residual.argtypes = [vp, vp, i64, cf, vp, vp, vp, vp, vp]
    lib.vqhip_decompress_residual.argtypes = [vp, vp, i64, cf, vp, vp, i64, vp]
    lib.vqhip_compress_file_residual.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(_GridSource), ci, i64, cf,
                                                 ctypes.POINTER(StreamStats), ctypes.POINTER(BoundedStats), ctypes.POINTER(ResidualStats)]
    lib.vqhip_decompress_file_residual.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, i64, GRID_BEGIN_FN, LEAF_ALLOC_FN, vp, ctypes.POINTER(StreamStats)]
    for name in RESIDUAL_SYMBOLS:
        getattr(lib, name).restype = ci
    # include/vqvdb_hip_rate.h
    lib.vqhip_rate_payload_bytes.argtypes = [vp]
    lib.vqhip_rate_sidecar_bytes.argtypes = [vp, ci]
    lib.vqhip_rate_sweep_device.argtypes = [vp, vp, vp, vp, i64, vp, ci, vp, vp]
    lib.vqhip_rate_sweep.argtypes = [vp, vp, i64, vp, ci, vp]
    lib.vqhip_rate_sweep_file.argtypes = [vp, ctypes.POINTER(_GridSource), ci, i64, vp, ci, vp, ctypes.POINTER(StreamStats)]
    lib.vqhip_rate_compress_file.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(_GridSource), ci, i64, vp, ci, i64, vp, vp,
                                             ctypes.POINTER(StreamStats), ctypes.POINTER(BoundedStats), ctypes.POINTER(ResidualStats)]
    for name in RATE_SYMBOLS:
        getattr(lib, name).restype = i64 if name.endswith("_bytes") else ci
    # include/vqvdb_hip_vec3_mask.h
    lib.vqhip_vec3_mask_leaf_err_device.argtypes = [vp, vp, vp, vp, i64, vp, vp]
    lib.vqhip_vec3_mask_residual_encode_device.argtypes = [vp, vp, vp, vp, vp, i64, cf, vp, vp, vp, i64, vp]
    lib.vqhip_vec3_mask_sweep_device.argtypes = [vp, vp, vp, vp, vp, i64, vp, ci, vp, vp]
    lib.vqhip_vec3_mask_compress_residual.argtypes = [vp, vp, vp, i64, cf, vp, vp, vp, vp, vp]
    lib.vqhip_vec3_mask_sweep.argtypes = [vp, vp, vp, i64, vp, ci, vp]
    for name in VEC3_MASK_SYMBOLS:
        getattr(lib, name).restype = ci
    # include/vqvdb_hip_vec3_active.h
    lib.vqhip_vec3_active_record_bytes.argtypes = [ci, ci]
    lib.vqhip_vec3_active_encode_device.argtypes = [vp, vp, vp, vp, vp, i64, cf, vp, vp, vp, i64, vp]
    lib.vqhip_vec3_active_apply_device.argtypes = [vp, vp, vp, i64, cf, vp, vp, vp, vp, vp]
    lib.vqhip_vec3_active_sweep_device.argtypes = [vp, vp, vp, vp, vp, i64, vp, ci, vp, vp]
    lib.vqhip_vec3_active_compress.argtypes = [vp, vp, vp, i64, cf, vp, vp, vp, vp, vp]
    lib.vqhip_vec3_active_decompress.argtypes = [vp, vp, vp, i64, cf, vp, vp, i64, vp, vp]
    lib.vqhip_vec3_active_sweep.argtypes = [vp, vp, vp, i64, vp, ci, vp]
    for name in VEC3_ACTIVE_SYMBOLS:
        getattr(lib, name).restype = i64 if name.endswith("_bytes") else ci
    # include/vqvdb_hip_vec3_file.h
    lib.vqhip_vec3_encode_leaves.argtypes = [vp, vp, i64, vp]
    lib.vqhip_vec3_decode_leaves.argtypes = [vp, vp, i64, vp]
    lib.vqhip_vec3_file_compress.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(_Vec3GridSource), ci, i64, ctypes.POINTER(StreamStats)]
    lib.vqhip_vec3_file_compress_active.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(_Vec3GridSource), ci, cf, i64, ctypes.POINTER(StreamStats), vp]
    lib.vqhip_vec3_file_decompress.argtypes = [vp, ctypes.c_char_p, i64, VEC3_GRID_BEGIN_FN, VEC3_LEAF_ALLOC_FN, vp, ctypes.POINTER(StreamStats)]
    lib.vqhip_vec3_file_info.argtypes = [ctypes.c_char_p, ctypes.POINTER(ci), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ci), ctypes.POINTER(ci),
                                         ctypes.POINTER(cf), ctypes.POINTER(i64), ctypes.POINTER(i64)]
    for name in VEC3_FILE_SYMBOLS:
        getattr(lib, name).restype = ci
    # include/vqvdb_hip_vec3_budget.h
    lib.vqhip_vec3_budget_pick.argtypes = [vp, vp, ci, i64]
    lib.vqhip_vec3_budget_file_bytes.argtypes = [ctypes.POINTER(_Vec3GridSource), ci, ci, vp]
    lib.vqhip_vec3_budget_compress.argtypes = [vp, vp, vp, i64, vp, ci, i64, vp, vp, vp, vp, vp, vp, vp]
    lib.vqhip_vec3_budget_file_sweep.argtypes = [vp, ctypes.POINTER(_Vec3GridSource), ci, vp, ci, i64, vp]
    lib.vqhip_vec3_budget_file_compress.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(_Vec3GridSource), ci, vp, ci, i64, i64,
                                                    ctypes.POINTER(StreamStats), vp, vp, vp]
    for name in VEC3_BUDGET_SYMBOLS:
        getattr(lib, name).restype = i64 if name.endswith("_bytes") else ci
    for name in VEC3_FULLTRAIN_SYMBOLS:
        if getattr(lib, name).argtypes is None:
            raise RuntimeError(f"codec.py: no argtypes declared for {name} (pointers would be truncated to 32 bits)")
        if name not in _VEC3_FULLTRAIN_I64:
            getattr(lib, name).restype = ci
    for name in VEC3_TRAIN_SYMBOLS:
        if getattr(lib, name).argtypes is None:
            raise RuntimeError(f"codec.py: no argtypes declared for {name} (pointers would be truncated to 32 bits)")
        if name != "vqhip_vec3_train_stats_floats":
            getattr(lib, name).restype = ci
    for name in ABI_SYMBOLS:
        if getattr(lib, name).argtypes is None and name not in ("vqhip_version",):
            raise RuntimeError(f"codec.py: no argtypes declared for {name} (pointers would be truncated to 32 bits)")
        if name not in ("vqhip_destroy", "vqhip_last_error", "vqhip_version", "vqhip_multi_destroy", "vqhip_multi_last_error",
                        "vqhip_fulltrain_param_count", "vqhip_workspace_bytes", "vqhip_chunk_leaves", "vqhip_fulltrain_decoder_offset",
                        "vqhip_fulltrain_ready_stream", "vqhip_vec3_destroy", "vqhip_vec3_last_error", "vqhip_vec3_chunk_leaves"):
            getattr(lib, name).restype = ci
    _lib = lib
    return lib


def pack_masks(active) -> np.ndarray:
    """bool [n,512] or [n,8,8,8] (voxel offset d*64 + h*8 + w) -> uint64 [n,8]: bit L of word j of a leaf is voxel 64 j + L, the
    words of OpenVDB's NodeMask<3> (leaf.valueMask()) that the masked calls take."""
    a = np.asarray(active)
    if a.dtype != np.bool_:
        raise TypeError("active must be a bool array")
    if not ((a.ndim == 2 and a.shape[1] == 512) or (a.ndim == 4 and a.shape[1:] == (8, 8, 8))):
        raise ValueError(f"active must have shape [n,512] or [n,8,8,8], got {list(a.shape)}")
    bits = np.packbits(a.reshape(-1, MASK_WORDS, 8, 8), axis=-1, bitorder="little")    # [n, word, byte, 1]: byte b holds the voxels 8 b .. 8 b + 7
    return np.ascontiguousarray(bits.reshape(-1, MASK_WORDS, 8)).view("<u8").reshape(-1, MASK_WORDS).astype(np.uint64)


def check_masks(masks, n: int) -> np.ndarray:
    """uint64, C-contiguous, [n,8] (what pack_masks returns; OpenVDB's mask words unconverted) -> the same array."""
    if not isinstance(masks, np.ndarray) or masks.dtype != np.uint64:
        raise TypeError("masks must be a uint64 numpy array (pack_masks turns a bool array into one)")
    if masks.ndim != 2 or masks.shape[1] != MASK_WORDS:
        raise ValueError(f"masks must have shape [n,8], got {list(masks.shape)}")
    if masks.shape[0] != n:
        raise ValueError(f"{n} leaves but {masks.shape[0]} masks")
    if not masks.flags.c_contiguous:
        raise ValueError("masks must be C-contiguous")
    return masks


VEC3_LEAF_SHAPE = (512, 3)
# debug_fetch names of the Vec3 handle -> (channels, positions) of one leaf
VEC3_DEBUG_LAYERS = {
    "encoder.pre.0": (64, 512), "encoder.pre.2": (64, 512), "encoder.pre": (64, 512), "encoder.down1": (128, 64),
    "encoder.res_stack.0": (128, 64), "encoder.res_stack.1": (128, 64), "encoder.proj": (64, 64),
    "decoder.stem.0": (128, 64), "decoder.stem": (128, 64), "decoder.res_stack.0": (128, 64), "decoder.res_stack.1": (128, 64),
    "decoder.up_conv": (256, 64),
}


class HipVec3Codec:
    """Owner of a ``vqhip_vec3_codec*``: the Vec3 model VQVAE(3, 64, K) (leaves float32 [n,512,3] channels last,
    indices uint16 [n,64]).  Arguments are checked here, before any C call."""

    def __init__(self, pack: Union[str, os.PathLike, bytes], device_id: int = 0, precision: str = "fp32"):
        self.check_precision(precision)
        self._lib = load_library()
        self._h = ctypes.c_void_p()
        if isinstance(pack, (bytes, bytearray, memoryview)):
            self._pack = bytes(pack)
            rc = self._lib.vqhip_vec3_create(None, self._pack, len(self._pack), device_id, ctypes.byref(self._h))
        else:
            rc = self._lib.vqhip_vec3_create(os.fspath(pack).encode(), None, 0, device_id, ctypes.byref(self._h))
        if rc != 0:
            raise RuntimeError(self._lib.vqhip_vec3_last_error(None).decode())
        if precision != "fp32":
            self.precision = precision

    @staticmethod
    def check_precision(precision) -> int:
        """"fp32" / "bf16" -> VQHIP_VEC3_PRECISION_* (include/vqvdb_hip_vec3_precision.h)."""
        if precision not in VEC3_PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(VEC3_PRECISIONS)}, got {precision!r}")
        return VEC3_PRECISIONS[precision]

    @property
    def precision(self) -> str:
        """Operand precision of the convolutions of encode / decode / debug_fetch: "fp32" (default) or "bf16" (DESIGN §14)."""
        mode = ctypes.c_int(-1)
        self._check(self._lib.vqhip_vec3_get_precision(self._h, ctypes.byref(mode)))
        return {v: k for k, v in VEC3_PRECISIONS.items()}[mode.value]

    @precision.setter
    def precision(self, precision: str):
        self._check(self._lib.vqhip_vec3_set_precision(self._h, self.check_precision(precision)))

    def _check(self, rc: int):
        if rc != 0:
            raise RuntimeError(self._lib.vqhip_vec3_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.vqhip_vec3_destroy(self._h)
            self._h = ctypes.c_void_p()

    __del__ = close

    def model_info(self) -> dict:
        k, d, lat = ctypes.c_int64(), ctypes.c_int64(), (ctypes.c_int64 * 3)()
        self._check(self._lib.vqhip_vec3_model_info(self._h, ctypes.byref(k), ctypes.byref(d), lat))
        return {"num_codes": k.value, "embedding_dim": d.value, "latent_shape": list(lat)}

    @staticmethod
    def check_leaves(leaves) -> np.ndarray:
        """float32, C-contiguous, [n,512,3] or [n,8,8,8,3] -> [n,512,3] view."""
        if not isinstance(leaves, np.ndarray) or leaves.dtype != np.float32:
            raise TypeError("vec3 leaves must be a float32 numpy array")
        if not leaves.flags.c_contiguous:
            raise ValueError("vec3 leaves must be C-contiguous")
        if leaves.ndim == 3 and leaves.shape[1:] == (512, 3):
            return leaves
        if leaves.ndim == 5 and leaves.shape[1:] == (8, 8, 8, 3):
            return leaves.reshape(-1, 512, 3)
        raise ValueError(f"vec3 leaves must have shape [n,512,3] or [n,8,8,8,3], got {list(leaves.shape)}")

    @staticmethod
    def check_indices(indices) -> np.ndarray:
        """uint16, C-contiguous, [n,64] or [n,4,4,4] -> [n,64] view."""
        if not isinstance(indices, np.ndarray) or indices.dtype != np.uint16:
            raise TypeError("vec3 indices must be a uint16 numpy array")
        if not indices.flags.c_contiguous:
            raise ValueError("vec3 indices must be C-contiguous")
        if indices.ndim == 2 and indices.shape[1] == 64:
            return indices
        if indices.ndim == 4 and indices.shape[1:] == (4, 4, 4):
            return indices.reshape(-1, 64)
        raise ValueError(f"vec3 indices must have shape [n,64] or [n,4,4,4], got {list(indices.shape)}")

    def encode(self, leaves: np.ndarray) -> np.ndarray:
        leaves = self.check_leaves(leaves)
        idx = np.empty((leaves.shape[0], 64), dtype=np.uint16)
        self._check(self._lib.vqhip_vec3_encode(self._h, leaves.ctypes.data, leaves.shape[0], idx.ctypes.data))
        return idx

    def decode(self, indices: np.ndarray) -> np.ndarray:
        indices = self.check_indices(indices)
        out = np.empty((indices.shape[0], 512, 3), dtype=np.float32)
        self._check(self._lib.vqhip_vec3_decode(self._h, indices.ctypes.data, indices.shape[0], out.ctypes.data))
        return out

    def encode_device(self, leaves_ptr: int, n: int, idx_ptr: int, stream: int = 0):
        self._check(self._lib.vqhip_vec3_encode_device(self._h, leaves_ptr, n, idx_ptr, stream or None))

    def decode_device(self, idx_ptr: int, n: int, leaves_ptr: int, stream: int = 0):
        self._check(self._lib.vqhip_vec3_decode_device(self._h, idx_ptr, n, leaves_ptr, stream or None))

    def set_chunk_leaves(self, n: int):
        self._check(self._lib.vqhip_vec3_set_chunk_leaves(self._h, n))

    def chunk_leaves(self) -> int:
        return int(self._lib.vqhip_vec3_chunk_leaves(self._h))

    def debug_enable(self, on: bool = True):
        self._check(self._lib.vqhip_vec3_debug_enable(self._h, 1 if on else 0))

    def debug_fetch(self, name: str, n: int) -> np.ndarray:
        """Activation ``name`` of the last chunk's first n leaves as float32 [n, C, positions]."""
        if name not in VEC3_DEBUG_LAYERS:
            raise KeyError(f"unknown vec3 layer {name!r}; one of {sorted(VEC3_DEBUG_LAYERS)}")
        ch, npos = VEC3_DEBUG_LAYERS[name]
        out = np.empty((n, ch, npos), dtype=np.float32)
        self._check(self._lib.vqhip_vec3_debug_fetch(self._h, name.encode(), n, out.ctypes.data))
        return out

    # ---- codebook (EMA) training: include/vqvdb_hip_vec3_train.h ----
    @staticmethod
    def check_train_batch(n: int, stats_ptr: int):
        if not isinstance(n, (int, np.integer)) or n < 0:
            raise ValueError(f"n must be a non-negative leaf count, got {n!r}")
        if not stats_ptr:
            raise ValueError("stats_ptr is NULL: the statistics need a device buffer of train_stats_floats() float32")

    @staticmethod
    def check_ema(decay: float, eps: float):
        if not (0.0 <= decay <= 1.0):
            raise ValueError(f"decay must be in [0, 1], got {decay}")
        if not eps > 0.0:
            raise ValueError(f"eps must be > 0, got {eps}")

    @staticmethod
    def check_state(k_codes: int, embedding=None, cluster_size=None, embed_avg=None) -> list:
        """float32 C-contiguous copies of the given buffers (None stays None), sizes K*64 / K / K*64."""
        out = []
        for a, size, what in zip((embedding, cluster_size, embed_avg), (k_codes * 64, k_codes, k_codes * 64),
                                 ("embedding", "cluster_size", "embed_avg")):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float32)
                if a.size != size:
                    raise ValueError(f"{what}: expected {size} float32 values, got {a.size}")
            out.append(a)
        return out

    def train_stats_floats(self) -> int:
        return int(self._lib.vqhip_vec3_train_stats_floats(self._h))

    def train_begin(self, cluster_size=None, embed_avg=None):
        _, cs, av = self.check_state(self.model_info()["num_codes"], None, cluster_size, embed_avg)
        self._check(self._lib.vqhip_vec3_train_begin(self._h, None if cs is None else cs.ctypes.data, None if av is None else av.ctypes.data))

    def train_vq_stats_device(self, leaves_ptr: int, n: int, stats_ptr: int, idx_ptr: int = 0, latent_ptr: int = 0, stream: int = 0):
        self.check_train_batch(n, stats_ptr)
        self._check(self._lib.vqhip_vec3_train_vq_stats_device(self._h, leaves_ptr, n, stats_ptr, idx_ptr or None, latent_ptr or None, stream or None))

    def train_eval_device(self, leaves_ptr: int, n: int, stats_ptr: int, recon_sums_ptr: int, recon_ptr: int = 0, stream: int = 0):
        self.check_train_batch(n, stats_ptr)
        if not recon_sums_ptr:
            raise ValueError("recon_sums_ptr is NULL: the reconstruction sums need a device buffer of 3 float32")
        self._check(self._lib.vqhip_vec3_train_eval_device(self._h, leaves_ptr, n, stats_ptr, recon_sums_ptr, recon_ptr or None, stream or None))

    def train_vq_update_device(self, stats_ptr: int, decay: float = 0.95, eps: float = 1e-4, stream: int = 0):
        self.check_ema(decay, eps)
        if not stats_ptr:
            raise ValueError("stats_ptr is NULL")
        self._check(self._lib.vqhip_vec3_train_vq_update_device(self._h, stats_ptr, decay, eps, stream or None))

    def train_get_state(self) -> dict:
        k = self.model_info()["num_codes"]
        emb, cs, avg = np.empty((k, 64), np.float32), np.empty(k, np.float32), np.empty((k, 64), np.float32)
        self._check(self._lib.vqhip_vec3_train_get_state(self._h, emb.ctypes.data, cs.ctypes.data, avg.ctypes.data))
        return {"embedding": emb, "cluster_size": cs, "embed_avg": avg}

    def train_set_state(self, embedding=None, cluster_size=None, embed_avg=None):
        arrs = self.check_state(self.model_info()["num_codes"], embedding, cluster_size, embed_avg)
        self._check(self._lib.vqhip_vec3_train_set_state(self._h, *[None if a is None else a.ctypes.data for a in arrs]))

    # ---- error-bounded round trip: include/vqvdb_hip_vec3_bounded.h ----
    @staticmethod
    def check_tol(tol) -> float:
        """A real number, NaN included (NaN selects every leaf) -> the float32 value the kernel compares with; the selection
        is ``~(leaf_err[:, 0] <= tol)``."""
        if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)):
            raise TypeError(f"tol must be a real number, got {tol!r}")
        with np.errstate(over="ignore"):
            t = np.float32(tol)
        if float(t) > float(tol):   # the kernel compares in float32: round down, so that err <= t implies err <= tol
            t = np.nextafter(t, np.float32(-np.inf))
        return float(t)

    def roundtrip_device(self, leaves_ptr: int, n: int, leaf_err_ptr: int, idx_ptr: int = 0, recon_ptr: int = 0, stream: int = 0):
        if not leaf_err_ptr:
            raise ValueError("leaf_err_ptr is NULL: the leaf errors need a device buffer of n * 2 float32")
        self._check(self._lib.vqhip_vec3_roundtrip_device(self._h, leaves_ptr, n, idx_ptr or None, recon_ptr or None, leaf_err_ptr, stream or None))

    def select_outliers_device(self, leaf_err_ptr: int, n: int, tol: float, ids_ptr: int, count_ptr: int, stream: int = 0):
        if not count_ptr:
            raise ValueError("count_ptr is NULL: the count needs a device buffer of one int64")
        self._check(self._lib.vqhip_vec3_select_outliers_device(self._h, leaf_err_ptr, n, self.check_tol(tol), ids_ptr, count_ptr, stream or None))

    def _compress_bounded_host(self, leaves: np.ndarray, tol: float):
        n = leaves.shape[0]
        idx, err = np.empty((n, 64), dtype=np.uint16), np.empty((n, VEC3_ERR_FLOATS), dtype=np.float32)
        ids, count = np.empty(n, dtype=np.int64), ctypes.c_int64(0)
        self._check(self._lib.vqhip_vec3_compress_bounded(self._h, leaves.ctypes.data, n, tol, idx.ctypes.data, err.ctypes.data, ids.ctypes.data,
                                                          ctypes.byref(count)))
        return idx, err, ids[:count.value].copy()

    def roundtrip(self, leaves, return_recon: bool = False):
        """Encode and decode in one pass -> (indices [n,64], leaf_err [n,2] = per leaf max |x - x^| and sum (x - x^)^2
        [, recon [n,512,3]]).  A float32 torch tensor on the handle's device gives device tensors (indices int16, the bits of
        the uint16 codes), ordered on torch's current stream (complete on return where that is the default stream); a numpy
        array goes through the host entry points."""
        if isinstance(leaves, np.ndarray):
            leaves = self.check_leaves(leaves)
            idx, err, _ = self._compress_bounded_host(leaves, float("inf"))
            return (idx, err, self.decode(idx)) if return_recon else (idx, err)
        import torch
        if not (isinstance(leaves, torch.Tensor) and leaves.is_cuda and leaves.dtype == torch.float32 and leaves.is_contiguous()):
            raise TypeError("vec3 leaves must be a float32 numpy array or a contiguous float32 torch tensor on the GPU")
        if tuple(leaves.shape[1:]) not in ((512, 3), (8, 8, 8, 3)):
            raise ValueError(f"vec3 leaves must have shape [n,512,3] or [n,8,8,8,3], got {list(leaves.shape)}")
        n = leaves.shape[0]
        idx = torch.empty((n, 64), dtype=torch.int16, device=leaves.device)
        err = torch.empty((n, VEC3_ERR_FLOATS), dtype=torch.float32, device=leaves.device)
        rec = torch.empty((n, 512, 3), dtype=torch.float32, device=leaves.device) if return_recon else None
        st = torch.cuda.current_stream(leaves.device).cuda_stream
        if st == 0:   # a null handle means the codec's own stream: order it after the producer of `leaves` by hand
            torch.cuda.synchronize(leaves.device)
        self.roundtrip_device(leaves.data_ptr(), n, err.data_ptr(), idx.data_ptr(), rec.data_ptr() if return_recon else 0, st)
        if st == 0:
            torch.cuda.synchronize(leaves.device)
        return (idx, err, rec) if return_recon else (idx, err)

    def compress_bounded(self, leaves: np.ndarray, tol: float, return_leaf_err: bool = False):
        """-> (indices [n,64], outlier_ids int64 ascending, outlier_leaves [m,512,3]): the leaves whose largest error is over
        ``tol`` (or not finite) come back as raw copies, so that decompress_bounded stays within tol on every value."""
        leaves = self.check_leaves(leaves)
        idx, err, ids = self._compress_bounded_host(leaves, self.check_tol(tol))
        out = (idx, ids, leaves[ids].copy())
        return out + (err,) if return_leaf_err else out

    def decompress_bounded(self, indices: np.ndarray, outlier_ids, outlier_leaves) -> np.ndarray:
        """Decoded leaves [n,512,3] with the leaves ``outlier_ids`` overwritten by their raw copies."""
        indices = self.check_indices(indices)
        ids = np.asarray(outlier_ids, dtype=np.int64).reshape(-1)
        raw = np.asarray(outlier_leaves, dtype=np.float32).reshape(-1, 512, 3)
        if len(ids) != len(raw):
            raise ValueError(f"{len(ids)} outlier ids but {len(raw)} outlier leaves")
        if len(ids) and (ids.min() < 0 or ids.max() >= indices.shape[0]):
            raise ValueError(f"outlier ids must be in [0, {indices.shape[0]})")
        out = self.decode(indices)
        out[ids] = raw
        return out

    # ---- quantised residuals: include/vqvdb_hip_vec3_residual.h ----
    @staticmethod
    def residual_record_sizes(leaf_code: np.ndarray) -> np.ndarray:
        """int64 [n]: the record bytes of every code (0 for kept leaves, 6144 for raw ones, 64 * (b0 + b1 + b2) for the code
        b0 | b1 << 5 | b2 << 10); a code that is neither a sentinel nor three widths of 0..16 with bit 15 clear is refused."""
        c = np.asarray(leaf_code).astype(np.int64)
        b = np.stack([c & 31, (c >> 5) & 31, (c >> 10) & 31], axis=-1)
        sentinel = (c == VEC3_RES_KEPT) | (c == VEC3_RES_RAW)
        if (~sentinel & ((c < 0) | (c >= 0x8000) | (b > 16).any(axis=-1))).any():
            raise ValueError("leaf codes must be 0xFFFE (kept), 0xFFFF (raw) or b0 | b1 << 5 | b2 << 10 with every width in 0..16")
        return np.where(c == VEC3_RES_KEPT, 0, np.where(c == VEC3_RES_RAW, 6144, 64 * b.sum(axis=-1)))

    @classmethod
    def check_residual(cls, n: int, leaf_code, payload):
        """-> (code uint16 [n], payload uint8 [bytes]): one valid code per leaf and exactly their records."""
        if not isinstance(leaf_code, np.ndarray) or leaf_code.dtype != np.uint16:
            raise TypeError("leaf_code must be a uint16 numpy array")
        lc = np.ascontiguousarray(leaf_code).reshape(-1)
        if len(lc) != n:
            raise ValueError(f"{n} leaves but {len(lc)} codes")
        if isinstance(payload, (bytes, bytearray, memoryview)):
            payload = np.frombuffer(payload, dtype=np.uint8)
        if not isinstance(payload, np.ndarray) or payload.dtype != np.uint8:
            raise TypeError("payload must be bytes or a uint8 numpy array")
        pl = np.ascontiguousarray(payload).reshape(-1)
        need = int(cls.residual_record_sizes(lc).sum())
        if need != len(pl):
            raise ValueError(f"the codes need {need} payload bytes, got {len(pl)}")
        return lc, pl

    def residual_encode_device(self, leaves_ptr: int, recon_ptr: int, leaf_err_ptr: int, n: int, tol: float, code_ptr: int, offsets_ptr: int,
                               payload_ptr: int, payload_capacity: int, stream: int = 0):
        """vqhip_vec3_residual_encode_device: codes [n] uint16, offsets [n+1] int64 (offsets[n] = the payload's bytes) and the payload."""
        if n > 0 and not (leaves_ptr and recon_ptr and leaf_err_ptr and code_ptr and offsets_ptr):
            raise ValueError("NULL device pointer: leaves, recon, leaf_err, code and offsets are required")
        if payload_capacity < 0:
            raise ValueError("payload_capacity must be >= 0")
        tol = self.check_tol(tol)
        self._check(self._lib.vqhip_vec3_residual_encode_device(self._h, leaves_ptr, recon_ptr, leaf_err_ptr, n, tol, code_ptr, offsets_ptr,
                                                                payload_ptr or None, payload_capacity, stream or None))

    def residual_apply_device(self, leaves_ptr: int, n: int, tol: float, code_ptr: int, offsets_ptr: int, payload_ptr: int, stream: int = 0):
        """vqhip_vec3_residual_apply_device: the decoded leaves at leaves_ptr corrected in place.  The device arrays are trusted."""
        if n > 0 and not (leaves_ptr and code_ptr and offsets_ptr):
            raise ValueError("NULL device pointer: leaves, code and offsets are required")
        tol = self.check_tol(tol)
        self._check(self._lib.vqhip_vec3_residual_apply_device(self._h, leaves_ptr, n, tol, code_ptr, offsets_ptr, payload_ptr or None,
                                                               stream or None))

    def compress_residual(self, leaves: np.ndarray, tol: float, return_leaf_err: bool = False):
        """-> (indices [n,64], leaf_code uint16 [n], payload uint8 [bytes]): a leaf whose largest error is within ``tol`` is kept
        (code 0xFFFE), any other is stored as its residual on a grid of 1.875 * tol with one bit width per channel (code
        b0 | b1 << 5 | b2 << 10, 64 * (b0 + b1 + b2) bytes) or, where that cannot keep it within tol, raw (code 0xFFFF, 6144
        bytes), so that decompress_residual in the same precision mode stays within tol on every value."""
        leaves = self.check_leaves(leaves)
        tol = self.check_tol(tol)
        n = leaves.shape[0]
        idx, err = np.empty((n, 64), dtype=np.uint16), np.empty((n, VEC3_ERR_FLOATS), dtype=np.float32)
        lc, payload, nbytes = np.empty(n, dtype=np.uint16), np.empty(n * 6144, dtype=np.uint8), ctypes.c_int64(0)
        self._check(self._lib.vqhip_vec3_residual_compress(self._h, leaves.ctypes.data, n, tol, idx.ctypes.data, err.ctypes.data, lc.ctypes.data,
                                                           payload.ctypes.data, ctypes.byref(nbytes)))
        out = (idx, lc, payload[:nbytes.value].copy())
        return out + (err,) if return_leaf_err else out

    def decompress_residual(self, indices: np.ndarray, tol: float, leaf_code, payload) -> np.ndarray:
        """Decoded leaves [n,512,3] with the records of compress_residual (same ``tol``, same precision mode) applied."""
        indices = self.check_indices(indices)
        tol = self.check_tol(tol)
        lc, pl = self.check_residual(indices.shape[0], leaf_code, payload)
        out = np.empty((indices.shape[0], 512, 3), dtype=np.float32)
        self._check(self._lib.vqhip_vec3_residual_decompress(self._h, indices.ctypes.data, indices.shape[0], tol, lc.ctypes.data, pl.ctypes.data,
                                                             len(pl), out.ctypes.data))
        return out

    # ---- size sweep and byte-budget compress: include/vqvdb_hip_vec3_rate.h ----
    @classmethod
    def check_tols(cls, tols) -> np.ndarray:
        """1 .. 64 rungs, each a real number >= 0 or NaN, rounded down to float32 by check_tol -> float32 [T]."""
        if isinstance(tols, (str, bytes)) or not hasattr(tols, "__len__"):
            raise TypeError("tols must be a sequence of real numbers")
        if not 1 <= len(tols) <= VEC3_RATE_MAX_TOLS:
            raise ValueError(f"tols must hold 1..{VEC3_RATE_MAX_TOLS} tolerances, got {len(tols)}")
        out = np.array([cls.check_tol(t) for t in tols], dtype=np.float32)
        if (out < 0).any():
            raise ValueError(f"tol must be >= 0 (or NaN: every leaf raw), got {[t for t, v in zip(tols, out) if v < 0][0]!r}")
        return out

    @staticmethod
    def rate_columns(leaf_code) -> np.ndarray:
        """int64 [n]: the histogram column of every code of residual_encode_device / compress_residual: b0 + b1 + b2 for a
        quantised leaf, 49 for a raw one, 50 for a kept one."""
        c = np.asarray(leaf_code).astype(np.int64)
        return np.where(c == VEC3_RES_KEPT, VEC3_RATE_CLASSES - 1,
                        np.where(c == VEC3_RES_RAW, VEC3_RATE_CLASSES - 2, (c & 31) + ((c >> 5) & 31) + ((c >> 10) & 31)))

    def rate_sweep_device(self, leaves_ptr: int, recon_ptr: int, leaf_err_ptr: int, n: int, tols, hist_ptr: int, stream: int = 0):
        """vqhip_vec3_rate_sweep_device: ADDS the histogram of n leaves at every rung to hist_ptr, a device buffer of
        len(tols) x 51 int64 that the caller zeroes before the first call; nothing is read back or synchronised."""
        tols = self.check_tols(tols)
        if n > 0 and not (leaves_ptr and recon_ptr and leaf_err_ptr and hist_ptr):
            raise ValueError("NULL device pointer: leaves, recon, leaf_err and hist are required")
        self._check(self._lib.vqhip_vec3_rate_sweep_device(self._h, leaves_ptr, recon_ptr, leaf_err_ptr, n, tols.ctypes.data, len(tols), hist_ptr,
                                                           stream or None))

    def rate_sweep(self, leaves: np.ndarray, tols) -> np.ndarray:
        """-> hist int64 [T,51]: hist[t, s] leaves would get a record of s = b0 + b1 + b2 planes (64 s bytes) from
        compress_residual at tols[t] (s = 0 .. 48), hist[t, 49] a raw record, hist[t, 50] none (kept), in the handle's
        precision mode.  vec3_rate_payload_bytes turns a row into the bytes of that compress."""
        leaves = self.check_leaves(leaves)
        tols = self.check_tols(tols)
        hist = np.empty((len(tols), VEC3_RATE_CLASSES), dtype=np.int64)
        self._check(self._lib.vqhip_vec3_rate_sweep(self._h, leaves.ctypes.data, leaves.shape[0], tols.ctypes.data, len(tols), hist.ctypes.data))
        return hist

    def rate_compress(self, leaves: np.ndarray, tols, payload_budget: int, return_leaf_err: bool = False):
        """compress_residual at the smallest of ``tols`` whose payload has at most ``payload_budget`` bytes
        (vqhip_vec3_rate_compress: one model round trip with the sweep behind it, then a decode and the encode of the records).
        -> (tol_used, hist int64 [T,51], indices [n,64], leaf_code uint16 [n], payload uint8 [bytes][, leaf_err [n,2]]), the
        last three or four as compress_residual(leaves, tol_used) returns them.  Raises RuntimeError if no rung fits."""
        leaves = self.check_leaves(leaves)
        tols = self.check_tols(tols)
        if isinstance(payload_budget, bool) or not isinstance(payload_budget, (int, np.integer)):
            raise TypeError(f"payload_budget must be an integer number of bytes, got {payload_budget!r}")
        if payload_budget < 0:
            raise ValueError(f"payload_budget must be >= 0, got {payload_budget}")
        n = leaves.shape[0]
        hist, used = np.empty((len(tols), VEC3_RATE_CLASSES), dtype=np.int64), ctypes.c_float(0)
        idx, err = np.empty((n, 64), dtype=np.uint16), np.empty((n, VEC3_ERR_FLOATS), dtype=np.float32)
        lc, payload, nbytes = np.empty(n, dtype=np.uint16), np.empty(n * 6144, dtype=np.uint8), ctypes.c_int64(0)
        self._check(self._lib.vqhip_vec3_rate_compress(self._h, leaves.ctypes.data, n, tols.ctypes.data, len(tols), int(payload_budget),
                                                       ctypes.byref(used), hist.ctypes.data, idx.ctypes.data, err.ctypes.data, lc.ctypes.data,
                                                       payload.ctypes.data, ctypes.byref(nbytes)))
        out = (used.value, hist, idx, lc, payload[:nbytes.value].copy())
        return out + (err,) if return_leaf_err else out

    # ---- active-voxel masks: include/vqvdb_hip_vec3_mask.h ----
    def mask_leaf_err_device(self, leaves_ptr: int, recon_ptr: int, mask_ptr: int, n: int, leaf_err_ptr: int, stream: int = 0):
        """vqhip_vec3_mask_leaf_err_device: leaf_err [n,2] over the active values of masks uint64 [n,8] (one bit per voxel, three channels)."""
        if n > 0 and not (leaves_ptr and recon_ptr and mask_ptr and leaf_err_ptr):
            raise ValueError("NULL device pointer: leaves, recon, mask and leaf_err are required")
        self._check(self._lib.vqhip_vec3_mask_leaf_err_device(self._h, leaves_ptr, recon_ptr, mask_ptr, n, leaf_err_ptr, stream or None))

    def mask_residual_encode_device(self, leaves_ptr: int, recon_ptr: int, mask_ptr: int, leaf_err_ptr: int, n: int, tol: float, code_ptr: int,
                                    offsets_ptr: int, payload_ptr: int, payload_capacity: int, stream: int = 0):
        """vqhip_vec3_mask_residual_encode_device: residual_encode_device on the masked error and the active values."""
        if n > 0 and not (leaves_ptr and recon_ptr and mask_ptr and leaf_err_ptr and code_ptr and offsets_ptr):
            raise ValueError("NULL device pointer: leaves, recon, mask, leaf_err, code and offsets are required")
        if payload_capacity < 0:
            raise ValueError("payload_capacity must be >= 0")
        tol = self.check_tol(tol)
        self._check(self._lib.vqhip_vec3_mask_residual_encode_device(self._h, leaves_ptr, recon_ptr, mask_ptr, leaf_err_ptr, n, tol, code_ptr,
                                                                     offsets_ptr, payload_ptr or None, payload_capacity, stream or None))

    def mask_sweep_device(self, leaves_ptr: int, recon_ptr: int, mask_ptr: int, leaf_err_ptr: int, n: int, tols, hist_ptr: int, stream: int = 0):
        """vqhip_vec3_mask_sweep_device: rate_sweep_device on the masked error and the active values; ADDS to hist_ptr."""
        tols = self.check_tols(tols)
        if n > 0 and not (leaves_ptr and recon_ptr and mask_ptr and leaf_err_ptr and hist_ptr):
            raise ValueError("NULL device pointer: leaves, recon, mask, leaf_err and hist are required")
        self._check(self._lib.vqhip_vec3_mask_sweep_device(self._h, leaves_ptr, recon_ptr, mask_ptr, leaf_err_ptr, n, tols.ctypes.data, len(tols),
                                                           hist_ptr, stream or None))

    def compress_residual_masked(self, leaves: np.ndarray, masks: np.ndarray, tol: float, return_leaf_err: bool = False):
        """compress_residual with value masks uint64 [n,8] (pack_masks): the tolerance holds on the active voxels and inactive
        ones cost nothing.  -> (indices, leaf_code, payload[, masked leaf_err]), read by decompress_residual unchanged."""
        leaves = self.check_leaves(leaves)
        n = leaves.shape[0]
        masks = check_masks(masks, n)
        tol = self.check_tol(tol)
        idx, err = np.empty((n, 64), dtype=np.uint16), np.empty((n, VEC3_ERR_FLOATS), dtype=np.float32)
        lc, payload, nbytes = np.empty(n, dtype=np.uint16), np.empty(n * 6144, dtype=np.uint8), ctypes.c_int64(0)
        self._check(self._lib.vqhip_vec3_mask_compress_residual(self._h, leaves.ctypes.data, masks.ctypes.data, n, tol, idx.ctypes.data, err.ctypes.data,
                                                                lc.ctypes.data, payload.ctypes.data, ctypes.byref(nbytes)))
        out = (idx, lc, payload[:nbytes.value].copy())
        return out + (err,) if return_leaf_err else out

    def rate_sweep_masked(self, leaves: np.ndarray, masks: np.ndarray, tols) -> np.ndarray:
        """rate_sweep with value masks: hist int64 [T,51] of compress_residual_masked at every rung."""
        leaves = self.check_leaves(leaves)
        masks = check_masks(masks, leaves.shape[0])
        tols = self.check_tols(tols)
        hist = np.empty((len(tols), VEC3_RATE_CLASSES), dtype=np.int64)
        self._check(self._lib.vqhip_vec3_mask_sweep(self._h, leaves.ctypes.data, masks.ctypes.data, leaves.shape[0], tols.ctypes.data, len(tols),
                                                    hist.ctypes.data))
        return hist

    # ---- records that hold only the active voxels: include/vqvdb_hip_vec3_active.h ----
    @staticmethod
    def check_background(background):
        """None, or three real numbers -> float32 [3] (NaN, inf and -0 pass as they are)."""
        if background is None:
            return None
        bg = np.ascontiguousarray(background, dtype=np.float32)
        if bg.shape != (3,):
            raise ValueError(f"background must be None or three numbers, got shape {list(bg.shape)}")
        return bg

    @staticmethod
    def active_counts(masks) -> np.ndarray:
        """int64 [n]: the active voxels of every leaf of masks uint64 [n,8]."""
        return np.unpackbits(np.ascontiguousarray(masks).view(np.uint8).reshape(len(masks), 64), axis=1).sum(axis=1, dtype=np.int64)

    @classmethod
    def active_record_sizes(cls, leaf_code, masks) -> np.ndarray:
        """int64 [n]: the bytes of every leaf's compact record: 0 kept, 8 ceil(3 A / 2) raw, 8 ceil(A / 64) (b0 + b1 + b2) quantised."""
        c = np.asarray(leaf_code).astype(np.int64)
        planes = cls.residual_record_sizes(leaf_code) // 64            # validates the codes; meaningless for the two sentinels
        a = cls.active_counts(masks)
        return np.where(c == VEC3_RES_KEPT, 0, np.where(c == VEC3_RES_RAW, 8 * ((3 * a + 1) // 2), 8 * ((a + 63) // 64) * planes))

    def active_encode_device(self, leaves_ptr: int, recon_ptr: int, mask_ptr: int, leaf_err_ptr: int, n: int, tol: float, code_ptr: int,
                             offsets_ptr: int, payload_ptr: int, payload_capacity: int, stream: int = 0):
        """vqhip_vec3_active_encode_device: the codes of mask_residual_encode_device with records of the active voxels only."""
        if n > 0 and not (leaves_ptr and recon_ptr and mask_ptr and leaf_err_ptr and code_ptr and offsets_ptr):
            raise ValueError("NULL device pointer: leaves, recon, mask, leaf_err, code and offsets are required")
        if payload_capacity < 0:
            raise ValueError("payload_capacity must be >= 0")
        tol = self.check_tol(tol)
        self._check(self._lib.vqhip_vec3_active_encode_device(self._h, leaves_ptr, recon_ptr, mask_ptr, leaf_err_ptr, n, tol, code_ptr, offsets_ptr,
                                                              payload_ptr or None, payload_capacity, stream or None))

    def active_apply_device(self, leaves_ptr: int, mask_ptr: int, n: int, tol: float, code_ptr: int, offsets_ptr: int, payload_ptr: int,
                            background=None, stream: int = 0):
        """vqhip_vec3_active_apply_device: the decoded leaves at leaves_ptr corrected in place at their active voxels; with a
        ``background`` of three numbers every inactive voxel receives it, with None inactive voxels are not touched.  The device
        arrays are trusted."""
        if n > 0 and not (leaves_ptr and mask_ptr and code_ptr and offsets_ptr):
            raise ValueError("NULL device pointer: leaves, mask, code and offsets are required")
        tol = self.check_tol(tol)
        bg = self.check_background(background)
        self._check(self._lib.vqhip_vec3_active_apply_device(self._h, leaves_ptr, mask_ptr, n, tol, code_ptr, offsets_ptr, payload_ptr or None,
                                                             None if bg is None else bg.ctypes.data, stream or None))

    def active_sweep_device(self, leaves_ptr: int, recon_ptr: int, mask_ptr: int, leaf_err_ptr: int, n: int, tols, bytes_ptr: int, stream: int = 0):
        """vqhip_vec3_active_sweep_device: ADDS the compact payload bytes of n leaves at every rung to bytes_ptr, a device buffer of
        len(tols) int64 that the caller zeroes before the first call."""
        tols = self.check_tols(tols)
        if n > 0 and not (leaves_ptr and recon_ptr and mask_ptr and leaf_err_ptr and bytes_ptr):
            raise ValueError("NULL device pointer: leaves, recon, mask, leaf_err and bytes are required")
        self._check(self._lib.vqhip_vec3_active_sweep_device(self._h, leaves_ptr, recon_ptr, mask_ptr, leaf_err_ptr, n, tols.ctypes.data, len(tols),
                                                             bytes_ptr, stream or None))

    def compress_active(self, leaves: np.ndarray, masks: np.ndarray, tol: float, return_leaf_err: bool = False):
        """compress_residual_masked with records that hold only the active voxels: the same indices and codes, a payload that
        shrinks with every leaf's active count.  -> (indices, leaf_code, payload[, masked leaf_err]), read by decompress_active
        with the same masks."""
        leaves = self.check_leaves(leaves)
        n = leaves.shape[0]
        masks = check_masks(masks, n)
        tol = self.check_tol(tol)
        idx, err = np.empty((n, 64), dtype=np.uint16), np.empty((n, VEC3_ERR_FLOATS), dtype=np.float32)
        lc, payload, nbytes = np.empty(n, dtype=np.uint16), np.empty(n * 6144, dtype=np.uint8), ctypes.c_int64(0)
        self._check(self._lib.vqhip_vec3_active_compress(self._h, leaves.ctypes.data, masks.ctypes.data, n, tol, idx.ctypes.data, err.ctypes.data,
                                                         lc.ctypes.data, payload.ctypes.data, ctypes.byref(nbytes)))
        out = (idx, lc, payload[:nbytes.value].copy())
        return out + (err,) if return_leaf_err else out

    def decompress_active(self, indices: np.ndarray, masks: np.ndarray, tol: float, leaf_code, payload, background=None) -> np.ndarray:
        """Decoded leaves [n,512,3] with the records of compress_active (same masks, same ``tol``, same precision mode) applied at
        the active voxels; inactive voxels hold ``background`` (three numbers) or, with None, what the decoder gave."""
        indices = self.check_indices(indices)
        n = indices.shape[0]
        masks = check_masks(masks, n)
        tol = self.check_tol(tol)
        bg = self.check_background(background)
        if not isinstance(leaf_code, np.ndarray) or leaf_code.dtype != np.uint16:
            raise TypeError("leaf_code must be a uint16 numpy array")
        lc = np.ascontiguousarray(leaf_code).reshape(-1)
        if len(lc) != n:
            raise ValueError(f"{n} leaves but {len(lc)} codes")
        if isinstance(payload, (bytes, bytearray, memoryview)):
            payload = np.frombuffer(payload, dtype=np.uint8)
        if not isinstance(payload, np.ndarray) or payload.dtype != np.uint8:
            raise TypeError("payload must be bytes or a uint8 numpy array")
        pl = np.ascontiguousarray(payload).reshape(-1)
        need = int(self.active_record_sizes(lc, masks).sum())
        if need != len(pl):
            raise ValueError(f"the codes and masks need {need} payload bytes, got {len(pl)}")
        out = np.empty((n, 512, 3), dtype=np.float32)
        self._check(self._lib.vqhip_vec3_active_decompress(self._h, indices.ctypes.data, masks.ctypes.data, n, tol, lc.ctypes.data, pl.ctypes.data,
                                                           len(pl), None if bg is None else bg.ctypes.data, out.ctypes.data))
        return out

    def rate_sweep_active(self, leaves: np.ndarray, masks: np.ndarray, tols) -> np.ndarray:
        """-> int64 [T]: the payload bytes of compress_active at every rung of ``tols``."""
        leaves = self.check_leaves(leaves)
        masks = check_masks(masks, leaves.shape[0])
        tols = self.check_tols(tols)
        out = np.empty(len(tols), dtype=np.int64)
        self._check(self._lib.vqhip_vec3_active_sweep(self._h, leaves.ctypes.data, masks.ctypes.data, leaves.shape[0], tols.ctypes.data, len(tols),
                                                      out.ctypes.data))
        return out

    # ---- OpenVDB leaves and the .vqv3 container: include/vqvdb_hip_vec3_file.h ----
    @staticmethod
    def _leaf_ptrs(leaf_arrays: Sequence[np.ndarray], n: int, writable: bool) -> np.ndarray:
        """uint64 [n]: the addresses of n per-leaf buffers, each checked: float32, 1536 elements, C-contiguous (the library reads /
        writes 6 KiB each)."""
        if len(leaf_arrays) != n:
            raise ValueError(f"expected {n} leaf buffers, got {len(leaf_arrays)}")
        for i, a in enumerate(leaf_arrays):
            if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.size != VEC3_LEAF_FLOATS or not a.flags.c_contiguous \
                    or (writable and not a.flags.writeable):
                raise ValueError(f"leaf buffer {i}: need a C-contiguous{' writable' if writable else ''} float32 array of {VEC3_LEAF_FLOATS} elements")
        return np.array([a.ctypes.data for a in leaf_arrays], dtype=np.uint64)

    def encode_leaves(self, leaf_arrays: Sequence[np.ndarray]) -> np.ndarray:
        """Leaf-pointer entry point: one [512,3] float32 buffer per leaf (e.g. the buffers of a Vec3fGrid's leaves) -> indices [n,64]."""
        n = len(leaf_arrays)
        ptrs = self._leaf_ptrs(leaf_arrays, n, writable=False)
        idx = np.empty((n, 64), dtype=np.uint16)
        self._check(self._lib.vqhip_vec3_encode_leaves(self._h, ptrs.ctypes.data, n, idx.ctypes.data))
        return idx

    def decode_leaves(self, indices: np.ndarray, leaf_arrays: Sequence[np.ndarray]) -> None:
        indices = self.check_indices(indices)
        n = indices.shape[0]
        ptrs = self._leaf_ptrs(leaf_arrays, n, writable=True)
        self._check(self._lib.vqhip_vec3_decode_leaves(self._h, indices.ctypes.data, n, ptrs.ctypes.data))

    def _grid_sources(self, grids, need_masks: bool):
        """The grid dicts of the file calls as a vqhip_vec3_grid_source array: _vec3_grid_sources."""
        return _vec3_grid_sources(grids, need_masks)

    def compress_file(self, path, grids, batch_leaves: int = 0) -> dict:
        """Whole-file compress into a .vqv3 file of kind 0 (origins and the indices of encode; masks are not written).  grids: the
        dicts of _grid_sources.  Returns the stream statistics."""
        src, n_g, _keep = self._grid_sources(grids, need_masks=False)
        st = StreamStats()
        self._check(self._lib.vqhip_vec3_file_compress(self._h, os.fspath(path).encode(), src, n_g, batch_leaves, ctypes.byref(st)))
        return st.as_dict()

    def compress_file_active(self, path, grids, tol: float, batch_leaves: int = 0) -> dict:
        """Whole-file compress into a .vqv3 file of kind 1: per grid what compress_active gives on its leaves and masks, in the
        handle's precision mode, which the header records.  Returns the stream statistics and "payload_bytes", one per grid."""
        tol = self.check_tol(tol)
        src, n_g, _keep = self._grid_sources(grids, need_masks=True)
        st, pb = StreamStats(), np.zeros(max(n_g, 1), dtype=np.int64)
        self._check(self._lib.vqhip_vec3_file_compress_active(self._h, os.fspath(path).encode(), src, n_g, tol, batch_leaves, ctypes.byref(st),
                                                              pb.ctypes.data))
        return dict(st.as_dict(), payload_bytes=[int(b) for b in pb[:n_g]])

    # ---- byte budgets on compact records, in memory and into a .vqv3 file: include/vqvdb_hip_vec3_budget.h ----
    @staticmethod
    def check_budget(budget, what: str) -> int:
        if isinstance(budget, bool) or not isinstance(budget, (int, np.integer)):
            raise TypeError(f"{what} must be an integer number of bytes, got {budget!r}")
        if not 0 <= budget < 2**63:
            raise ValueError(f"{what} must be in 0 .. 2^63 - 1, got {budget}")
        return int(budget)

    def rate_compress_active(self, leaves: np.ndarray, masks: np.ndarray, tols, payload_budget: int, return_leaf_err: bool = False):
        """compress_active at the smallest of ``tols`` whose compact payload has at most ``payload_budget`` bytes
        (vqhip_vec3_budget_compress: one model round trip with the size sweep behind it, then a decode and the encode of the selected
        leaves only).  -> (tol_used, bytes int64 [T] as rate_sweep_active gives them, indices [n,64], leaf_code uint16 [n], payload
        uint8 [bytes][, masked leaf_err [n,2]]), the last three or four as compress_active(leaves, masks, tol_used) returns them.
        Raises RuntimeError if no rung fits."""
        leaves = self.check_leaves(leaves)
        n = leaves.shape[0]
        masks = check_masks(masks, n)
        tols = self.check_tols(tols)
        payload_budget = self.check_budget(payload_budget, "payload_budget")
        sizes, used = np.empty(len(tols), dtype=np.int64), ctypes.c_float(0)
        idx, err = np.empty((n, 64), dtype=np.uint16), np.empty((n, VEC3_ERR_FLOATS), dtype=np.float32)
        lc, payload, nbytes = np.empty(n, dtype=np.uint16), np.empty(n * 6144, dtype=np.uint8), ctypes.c_int64(0)
        self._check(self._lib.vqhip_vec3_budget_compress(self._h, leaves.ctypes.data, masks.ctypes.data, n, tols.ctypes.data, len(tols), payload_budget,
                                                         ctypes.byref(used), sizes.ctypes.data, idx.ctypes.data, err.ctypes.data, lc.ctypes.data,
                                                         payload.ctypes.data, ctypes.byref(nbytes)))
        out = (used.value, sizes, idx, lc, payload[:nbytes.value].copy())
        return out + (err,) if return_leaf_err else out

    def rate_sweep_file(self, grids, tols, batch_leaves: int = 0) -> np.ndarray:
        """-> int64 [G,T]: the payloadBytes of every grid in the file that compress_file_active writes at every rung of ``tols``
        (per grid what rate_sweep_active gives on its leaves and masks).  Nothing is written."""
        tols = self.check_tols(tols)
        src, n_g, _keep = self._grid_sources(grids, need_masks=True)
        out = np.zeros((max(n_g, 1), len(tols)), dtype=np.int64)
        self._check(self._lib.vqhip_vec3_budget_file_sweep(self._h, src, n_g, tols.ctypes.data, len(tols), batch_leaves, out.ctypes.data))
        return out[:n_g]

    def compress_file_budget(self, path, grids, tols, file_budget: int, batch_leaves: int = 0) -> dict:
        """compress_file_active at the smallest of ``tols`` whose FILE has at most ``file_budget`` bytes, headers, origins, indices,
        masks and codes included (vqhip_vec3_budget_file_compress; the file has one tolerance for all grids).  Returns the stream
        statistics with "tol_used", "payload_bytes" (one per grid) and "file_bytes".  Raises RuntimeError if no rung fits; the output
        is then not opened and a file at ``path`` keeps its bytes."""
        tols = self.check_tols(tols)
        file_budget = self.check_budget(file_budget, "file_budget")
        src, n_g, _keep = self._grid_sources(grids, need_masks=True)
        st, pb, used, size = StreamStats(), np.zeros(max(n_g, 1), dtype=np.int64), ctypes.c_float(0), ctypes.c_int64(0)
        self._check(self._lib.vqhip_vec3_budget_file_compress(self._h, os.fspath(path).encode(), src, n_g, tols.ctypes.data, len(tols), file_budget,
                                                              batch_leaves, ctypes.byref(st), ctypes.byref(used), pb.ctypes.data, ctypes.byref(size)))
        return dict(st.as_dict(), tol_used=used.value, payload_bytes=[int(b) for b in pb[:n_g]], file_bytes=size.value)

    def decompress_file(self, path, batch_leaves: int = 0, return_stats: bool = False):
        """Whole-file decompress of a .vqv3 file of either kind -> a list of dicts, one per grid: "name", "transform" [16], "origins"
        [n,3], "masks" uint64 [n,8] (None for kind 0), "leaves" float32 [n,512,3], "batches" (the sizes of the leaf_alloc batches) and
        the info fields "num_codes", "total_blocks", "kind", "mode", "tol", "background" (None where the grid has none).  The leaf
        allocator hands out one fresh block per batch, the stand-in for tree.touchLeaf().  return_stats: -> (grids, statistics)."""
        grids = []

        def on_grid(_user, gi):
            g = gi.contents
            grids.append({"name": g.name.decode(), "transform": np.array(g.transform[:], dtype=np.float32), "num_codes": int(g.num_codes),
                          "total_blocks": int(g.total_blocks), "kind": int(g.kind), "mode": int(g.mode),
                          "tol": float(g.tol),
                          "background": np.array(g.background[:], dtype=np.float32) if g.has_background else None, "_blocks": []})
            return 0

        def on_alloc(_user, gidx, origins, masks, n, out_ptrs):
            try:
                org = np.ctypeslib.as_array(origins, shape=(n, 3)).copy()
                msk = np.ctypeslib.as_array(masks, shape=(n, MASK_WORDS)).copy() if masks else None
                buf = np.empty((n, 512, 3), dtype=np.float32)
                dst = np.ctypeslib.as_array(ctypes.cast(out_ptrs, ctypes.POINTER(ctypes.c_uint64)), shape=(n,))
                dst[:] = buf.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(VEC3_LEAF_FLOATS * 4)
                grids[gidx]["_blocks"].append((org, msk, buf))
                return 0
            except Exception as e:  # noqa: BLE001 — an exception must not unwind through the C frames
                print(f"decompress_file allocator: {e}", file=sys.stderr)
                return 1

        cb_g, cb_a = VEC3_GRID_BEGIN_FN(on_grid), VEC3_LEAF_ALLOC_FN(on_alloc)
        st = StreamStats()
        self._check(self._lib.vqhip_vec3_file_decompress(self._h, os.fspath(path).encode(), batch_leaves, cb_g, cb_a, None, ctypes.byref(st)))
        for g in grids:
            bl = g.pop("_blocks")
            g["batches"] = [len(b[0]) for b in bl]
            g["origins"] = np.concatenate([b[0] for b in bl]) if bl else np.zeros((0, 3), np.int32)
            g["masks"] = None if g["kind"] == 0 else (np.concatenate([b[1] for b in bl]) if bl else np.zeros((0, MASK_WORDS), np.uint64))
            g["leaves"] = np.concatenate([b[2] for b in bl]) if bl else np.zeros((0, 512, 3), np.float32)
        return (grids, st.as_dict()) if return_stats else grids

    # ---- full training: include/vqvdb_hip_vec3_fulltrain.h ----
    @staticmethod
    def check_fulltrain_batch(n: int, n_global: int, grads_ptr: int, aux_ptr: int):
        if not isinstance(n, (int, np.integer)) or n < 0:
            raise ValueError(f"n must be a non-negative leaf count, got {n!r}")
        if not isinstance(n_global, (int, np.integer)) or n_global < max(n, 1):
            raise ValueError(f"n_global must be >= n and >= 1, got n_global={n_global!r}, n={n}")
        if not grads_ptr:
            raise ValueError("grads_ptr is NULL: the gradients need a device buffer of fulltrain_param_count() float32")
        if not aux_ptr:
            raise ValueError("aux_ptr is NULL: the statistics need a device buffer of fulltrain_aux_floats() float32")

    @staticmethod
    def check_adamw(lr: float, step: int, betas, adam_eps: float, weight_decay: float):
        if not isinstance(step, (int, np.integer)) or step < 1:
            raise ValueError(f"step must be an integer >= 1, got {step!r}")
        if not lr >= 0.0:
            raise ValueError(f"lr must be >= 0, got {lr}")
        if len(betas) != 2 or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f"betas must be two values in [0, 1), got {betas}")
        if not adam_eps > 0.0:
            raise ValueError(f"adam_eps must be > 0, got {adam_eps}")
        if not weight_decay >= 0.0:
            raise ValueError(f"weight_decay must be >= 0, got {weight_decay}")

    def _check_vector(self, a, what: str) -> np.ndarray:
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.size != self.fulltrain_param_count():
            raise ValueError(f"{what}: expected {self.fulltrain_param_count()} float32 values, got {a.size}")
        return a

    def fulltrain_param_count(self) -> int:
        return int(self._lib.vqhip_vec3_fulltrain_param_count(self._h))

    def fulltrain_decoder_offset(self) -> int:
        return int(self._lib.vqhip_vec3_fulltrain_decoder_offset(self._h))

    def fulltrain_aux_floats(self) -> int:
        return int(self._lib.vqhip_vec3_fulltrain_aux_floats(self._h))

    def fulltrain_begin(self):
        self._check(self._lib.vqhip_vec3_fulltrain_begin(self._h))

    def fulltrain_fwdbwd_device(self, leaves_ptr: int, n: int, n_global: int, grads_ptr: int, aux_ptr: int, latent_ptr: int = 0, stream: int = 0):
        self.check_fulltrain_batch(n, n_global, grads_ptr, aux_ptr)
        self._check(self._lib.vqhip_vec3_fulltrain_fwdbwd_device(self._h, leaves_ptr, n, n_global, grads_ptr, aux_ptr, latent_ptr or None,
                                                                 stream or None))

    def fulltrain_forward_device(self, leaves_ptr: int, n: int, idx_ptr: int = 0, recon_ptr: int = 0, stream: int = 0):
        if not isinstance(n, (int, np.integer)) or n < 0:
            raise ValueError(f"n must be a non-negative leaf count, got {n!r}")
        self._check(self._lib.vqhip_vec3_fulltrain_forward_device(self._h, leaves_ptr, n, idx_ptr or None, recon_ptr or None, stream or None))

    def fulltrain_apply_device(self, grads_ptr: int, aux_ptr: int, lr: float, step: int, betas=(0.9, 0.999), adam_eps: float = 1e-8,
                               weight_decay: float = 1e-4, decay: float = 0.95, eps: float = 1e-4, stream: int = 0):
        if not grads_ptr:
            raise ValueError("grads_ptr is NULL")
        self.check_adamw(lr, step, betas, adam_eps, weight_decay)
        if aux_ptr:
            self.check_ema(decay, eps)
        self._check(self._lib.vqhip_vec3_fulltrain_apply_device(self._h, grads_ptr, aux_ptr or None, lr, step, betas[0], betas[1], adam_eps,
                                                                weight_decay, decay, eps, stream or None))

    def fulltrain_get_params(self) -> np.ndarray:
        out = np.empty(self.fulltrain_param_count(), np.float32)
        self._check(self._lib.vqhip_vec3_fulltrain_get_params(self._h, out.ctypes.data))
        return out

    def fulltrain_set_params(self, params):
        p = self._check_vector(params, "params")
        self._check(self._lib.vqhip_vec3_fulltrain_set_params(self._h, p.ctypes.data))

    def fulltrain_get_opt_state(self) -> tuple:
        m, v = np.empty(self.fulltrain_param_count(), np.float32), np.empty(self.fulltrain_param_count(), np.float32)
        self._check(self._lib.vqhip_vec3_fulltrain_get_opt_state(self._h, m.ctypes.data, v.ctypes.data))
        return m, v

    def fulltrain_set_opt_state(self, exp_avg, exp_avg_sq):
        m, v = self._check_vector(exp_avg, "exp_avg"), self._check_vector(exp_avg_sq, "exp_avg_sq")
        self._check(self._lib.vqhip_vec3_fulltrain_set_opt_state(self._h, m.ctypes.data, v.ctypes.data))


class HipCodec:
    """Thin owner of a ``vqhip_codec*`` — the C ABI one-to-one, numpy/raw pointers in and out."""

    def __init__(self, pack: Union[str, os.PathLike, bytes], device_id: int = 0, decode_precision: str = "fp32",
                 encode_precision: str = "fp32"):
        self.check_decode_precision(decode_precision)
        self.check_encode_precision(encode_precision)
        self._lib = load_library()
        self._h = ctypes.c_void_p()
        if isinstance(pack, (bytes, bytearray, memoryview)):
            self._pack = bytes(pack)
            rc = self._lib.vqhip_create(None, self._pack, len(self._pack), device_id, ctypes.byref(self._h))
        else:
            rc = self._lib.vqhip_create(os.fspath(pack).encode(), None, 0, device_id, ctypes.byref(self._h))
        if rc != 0:
            raise RuntimeError(self._lib.vqhip_last_error(None).decode())
        if decode_precision != "fp32":
            self.decode_precision = decode_precision
        if encode_precision != "fp32":
            self.encode_precision = encode_precision

    @staticmethod
    def check_decode_precision(precision) -> int:
        """"fp32" / "bf16" -> VQHIP_PRECISION_* (include/vqvdb_hip_precision.h)."""
        if precision not in PRECISIONS:
            raise ValueError(f"decode_precision must be one of {sorted(PRECISIONS)}, got {precision!r}")
        return PRECISIONS[precision]

    @property
    def decode_precision(self) -> str:
        """Operand precision of the decoder's two 64-channel convs in decode / decode_device / decode_leaves / decompress_file and
        the debug_fetch after them: "fp32" (default) or "bf16" (DESIGN §23).  Every bounded, residual, rate, round-trip and
        training call decodes in fp32 whatever this says."""
        mode = ctypes.c_int(-1)
        self._check(self._lib.vqhip_get_decode_mode(self._h, ctypes.byref(mode)))
        return {v: k for k, v in PRECISIONS.items()}[mode.value]

    @decode_precision.setter
    def decode_precision(self, precision: str):
        self._check(self._lib.vqhip_set_decode_mode(self._h, self.check_decode_precision(precision)))

    @staticmethod
    def check_encode_precision(precision) -> int:
        """"fp32" / "bf16" -> VQHIP_PRECISION_* (include/vqvdb_hip_encode_mode.h)."""
        if not isinstance(precision, str) or precision not in PRECISIONS:
            raise ValueError(f"encode_precision must be one of {sorted(PRECISIONS)}, got {precision!r}")
        return PRECISIONS[precision]

    @property
    def encode_precision(self) -> str:
        """Operand precision of the encoder's two 16-channel convs in encode / encode_device / encode_leaves / compress_file and
        the debug_fetch after them: "fp32" (default) or "bf16" (DESIGN §24).  Every bounded, residual, rate, round-trip and
        training call encodes in fp32 whatever this says, and decode_precision is a separate switch."""
        mode = ctypes.c_int(-1)
        self._check(self._lib.vqhip_get_encode_mode(self._h, ctypes.byref(mode)))
        return {v: k for k, v in PRECISIONS.items()}[mode.value]

    @encode_precision.setter
    def encode_precision(self, precision: str):
        self._check(self._lib.vqhip_set_encode_mode(self._h, self.check_encode_precision(precision)))

    def _check(self, rc: int):
        if rc != 0:
            raise RuntimeError(self._lib.vqhip_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.vqhip_destroy(self._h)
            self._h = ctypes.c_void_p()

    __del__ = close

    def latent_shape(self) -> list:
        out = (ctypes.c_int64 * 3)()
        self._check(self._lib.vqhip_latent_shape(self._h, out))
        return list(out)

    @staticmethod
    def _out(out, shape, dtype):
        if out is None:
            return np.empty(shape, dtype=dtype)
        if out.dtype != dtype or out.size != shape[0] * shape[1] or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous {np.dtype(dtype).name} array of {shape[0] * shape[1]} elements")
        return out

    def encode(self, leaves: np.ndarray, out: Optional[np.ndarray] = None) -> np.ndarray:
        leaves = np.ascontiguousarray(leaves, dtype=np.float32).reshape(-1, LEAF_VOXELS)
        idx = self._out(out, (leaves.shape[0], LATENT_VOXELS), np.uint8)
        self._check(self._lib.vqhip_encode(self._h, leaves.ctypes.data, leaves.shape[0], idx.ctypes.data))
        return idx

    def decode(self, indices: np.ndarray, out: Optional[np.ndarray] = None) -> np.ndarray:
        indices = np.ascontiguousarray(indices, dtype=np.uint8).reshape(-1, LATENT_VOXELS)
        out = self._out(out, (indices.shape[0], LEAF_VOXELS), np.float32)
        self._check(self._lib.vqhip_decode(self._h, indices.ctypes.data, indices.shape[0], out.ctypes.data))
        return out

    @staticmethod
    def _leaf_ptrs(leaf_arrays: Sequence[np.ndarray], n: int, writable: bool):
        """Addresses of n per-leaf buffers, each checked: float32, 512 elements, C-contiguous (the library reads / writes 2 KiB each)."""
        if len(leaf_arrays) != n:
            raise ValueError(f"expected {n} leaf buffers, got {len(leaf_arrays)}")
        for i, a in enumerate(leaf_arrays):
            if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.size != LEAF_VOXELS or not a.flags.c_contiguous \
                    or (writable and not a.flags.writeable):
                raise ValueError(f"leaf buffer {i}: need a C-contiguous{' writable' if writable else ''} float32 array of {LEAF_VOXELS} elements")
        return (ctypes.c_void_p * n)(*[a.ctypes.data for a in leaf_arrays])

    def encode_leaves(self, leaf_arrays: Sequence[np.ndarray]) -> np.ndarray:
        """Leaf-pointer entry point: one 512-float buffer per leaf (e.g. OpenVDB leaf buffers)."""
        n = len(leaf_arrays)
        ptrs = self._leaf_ptrs(leaf_arrays, n, writable=False)
        idx = np.empty((n, LATENT_VOXELS), dtype=np.uint8)
        self._check(self._lib.vqhip_encode_leaves(self._h, ptrs, n, idx.ctypes.data))
        return idx

    def decode_leaves(self, indices: np.ndarray, leaf_arrays: Sequence[np.ndarray]) -> None:
        indices = np.ascontiguousarray(indices, dtype=np.uint8).reshape(-1, LATENT_VOXELS)
        n = indices.shape[0]
        ptrs = self._leaf_ptrs(leaf_arrays, n, writable=True)
        self._check(self._lib.vqhip_decode_leaves(self._h, indices.ctypes.data, n, ptrs))

    def compress_file(self, path, grids, batch_leaves: int = 0) -> dict:
        """Whole-file compress (vqhip_compress_file).  grids: sequence of (name, origins int32 [n,3], leaves float32 [n,512]
        or a list of n 512-float arrays, transform or None).  Returns the stream statistics."""
        src, n_g, _keep = self._grid_sources(grids)
        st = StreamStats()
        self._check(self._lib.vqhip_compress_file(self._h, os.fspath(path).encode(), src, n_g, batch_leaves, ctypes.byref(st)))
        return st.as_dict()

    def _grid_sources(self, grids):
        """(vqhip_grid_source array, its length, the arrays it points into) of compress_file's grid tuples."""
        n_g = len(grids)
        src = (_GridSource * max(n_g, 1))()
        keep = []
        for i, (name, origins, leaves, transform) in enumerate(grids):
            origins = np.ascontiguousarray(origins, dtype=np.int32).reshape(-1, 3)
            n = origins.shape[0]
            if isinstance(leaves, np.ndarray):
                leaves = np.ascontiguousarray(leaves, dtype=np.float32).reshape(n, LEAF_VOXELS)
                ptrs = leaves.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(LEAF_VOXELS * 4)
            else:
                if len(leaves) != n:
                    raise ValueError("one leaf buffer per origin")
                self._leaf_ptrs(leaves, n, writable=False)   # validates every buffer
                ptrs = np.array([a.ctypes.data for a in leaves], dtype=np.uint64)
            ptrs = np.ascontiguousarray(ptrs, dtype=np.uint64)
            tr = None if transform is None else np.ascontiguousarray(transform, dtype=np.float32).reshape(16)
            bname = name.encode()
            keep += [origins, leaves, ptrs, tr, bname]
            src[i].name = bname
            src[i].transform = tr.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if tr is not None else None
            src[i].leaf_ptrs = ptrs.ctypes.data if n else None
            src[i].origins = origins.ctypes.data if n else None
            src[i].n_leaves = n
        return src, n_g, keep

    def decompress_file(self, path, batch_leaves: int = 0, out: Optional[np.ndarray] = None):
        """Whole-file decompress (vqhip_decompress_file).  Returns ([(name, transform[16], origins [n,3], leaves [n,512])], stats);
        the leaf allocator hands out one fresh 2 KiB-per-leaf block per batch, the stand-in for tree.touchLeaf().
        out: optional preallocated C-contiguous float32 [total_leaves, 512] pool — leaves of all grids are then placed in it in
        file order (no per-batch allocation, no concatenation: multi-million-leaf files) and the returned leaf arrays are views."""
        return self._decompress_file(path, None, batch_leaves, out)

    def _decompress_file(self, path, residual_path, batch_leaves, out, residual_version: int = 1):
        grids, blocks = [], []
        if out is not None and (out.dtype != np.float32 or out.ndim != 2 or out.shape[1] != LEAF_VOXELS or not out.flags.c_contiguous):
            raise ValueError("out must be a C-contiguous float32 [n, 512] array")
        cursor = [0]

        def on_grid(_user, gi):
            g = gi.contents
            grids.append([g.name.decode(), np.array(g.transform[:], dtype=np.float32), int(g.total_blocks)])
            blocks.append([])
            return 0

        def on_alloc(_user, gidx, origins, n, out_ptrs):
            try:
                org = np.ctypeslib.as_array(origins, shape=(n, 3)).copy()
                if out is not None:
                    if cursor[0] + n > out.shape[0]:
                        raise ValueError(f"out holds {out.shape[0]} leaves, the file has more")
                    buf = out[cursor[0]:cursor[0] + n]
                    cursor[0] += n
                else:
                    buf = np.empty((n, LEAF_VOXELS), dtype=np.float32)
                dst = np.ctypeslib.as_array(ctypes.cast(out_ptrs, ctypes.POINTER(ctypes.c_uint64)), shape=(n,))
                dst[:] = buf.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(LEAF_VOXELS * 4)
                blocks[gidx].append((org, buf))
                return 0
            except Exception as e:  # noqa: BLE001 — an exception must not unwind through the C frames
                print(f"decompress_file allocator: {e}", file=sys.stderr)
                return 1

        cb_g, cb_a = GRID_BEGIN_FN(on_grid), LEAF_ALLOC_FN(on_alloc)
        st = StreamStats()
        if residual_path is None:
            self._check(self._lib.vqhip_decompress_file(self._h, os.fspath(path).encode(), batch_leaves, cb_g, cb_a, None, ctypes.byref(st)))
        else:
            call = self._lib.vqhip_decompress_file_residual if residual_version == 2 else self._lib.vqhip_decompress_file_bounded
            self._check(call(self._h, os.fspath(path).encode(), os.fspath(residual_path).encode(), batch_leaves, cb_g, cb_a, None, ctypes.byref(st)))
        result = []
        for (name, tr, _total), bl in zip(grids, blocks):
            org = np.concatenate([b[0] for b in bl]) if bl else np.zeros((0, 3), np.int32)
            if out is not None and len(bl):   # consecutive slices of the pool: one view, no copy
                first = (bl[0][1].ctypes.data - out.ctypes.data) // (LEAF_VOXELS * 4)
                lv = out[first:first + sum(len(b[1]) for b in bl)]
            else:
                lv = np.concatenate([b[1] for b in bl]) if bl else np.zeros((0, LEAF_VOXELS), np.float32)
            result.append((name, tr, org, lv))
        return result, st.as_dict()

    def encode_device(self, leaves_ptr: int, n: int, idx_ptr: int, stream: int = 0):
        self._check(self._lib.vqhip_encode_device(self._h, leaves_ptr, n, idx_ptr, stream or None))

    def decode_device(self, idx_ptr: int, n: int, leaves_ptr: int, stream: int = 0):
        self._check(self._lib.vqhip_decode_device(self._h, idx_ptr, n, leaves_ptr, stream or None))

    def set_chunk_leaves(self, n: int):
        self._check(self._lib.vqhip_set_chunk_leaves(self._h, n))

    # ---- error-bounded compression: include/vqvdb_hip_bounded.h ----
    check_tol = staticmethod(HipVec3Codec.check_tol)

    @classmethod
    def check_bound(cls, tol) -> float:
        """check_tol, and a tolerance below zero is refused: no error is <= it, so it can only be a mistake."""
        t = cls.check_tol(tol)
        if t < 0:
            raise ValueError(f"tol must be >= 0 (or NaN: every leaf raw), got {tol!r}")
        return t

    @staticmethod
    def check_leaves(leaves) -> np.ndarray:
        """float32, C-contiguous, [n,512] or [n,8,8,8] -> [n,512] view."""
        if not isinstance(leaves, np.ndarray) or leaves.dtype != np.float32:
            raise TypeError("leaves must be a float32 numpy array")
        if not leaves.flags.c_contiguous:
            raise ValueError("leaves must be C-contiguous")
        if leaves.ndim == 2 and leaves.shape[1] == LEAF_VOXELS:
            return leaves
        if leaves.ndim == 4 and leaves.shape[1:] == (8, 8, 8):
            return leaves.reshape(-1, LEAF_VOXELS)
        raise ValueError(f"leaves must have shape [n,512] or [n,8,8,8], got {list(leaves.shape)}")

    @staticmethod
    def check_indices(indices) -> np.ndarray:
        """uint8, C-contiguous, [n,64] or [n,4,4,4] -> [n,64] view."""
        if not isinstance(indices, np.ndarray) or indices.dtype != np.uint8:
            raise TypeError("indices must be a uint8 numpy array")
        if not indices.flags.c_contiguous:
            raise ValueError("indices must be C-contiguous")
        if indices.ndim == 2 and indices.shape[1] == LATENT_VOXELS:
            return indices
        if indices.ndim == 4 and indices.shape[1:] == (4, 4, 4):
            return indices.reshape(-1, LATENT_VOXELS)
        raise ValueError(f"indices must have shape [n,64] or [n,4,4,4], got {list(indices.shape)}")

    @staticmethod
    def check_outliers(n: int, outlier_ids, outlier_leaves):
        """-> (ids int64 [m], raw float32 [m,512]): one raw leaf per id, the ids ascending, unique and in [0, n)."""
        ids = np.asarray(outlier_ids)
        if ids.size and not np.issubdtype(ids.dtype, np.integer):
            raise TypeError("outlier ids must be integers")
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        raw = np.asarray(outlier_leaves)
        if raw.size and raw.dtype != np.float32:
            raise TypeError("outlier leaves must be float32")
        if raw.size % LEAF_VOXELS:
            raise ValueError("outlier leaves must hold 512 values each")
        raw = np.ascontiguousarray(raw, dtype=np.float32).reshape(-1, LEAF_VOXELS)
        if len(ids) != len(raw):
            raise ValueError(f"{len(ids)} outlier ids but {len(raw)} outlier leaves")
        if len(ids) and (ids.min() < 0 or ids.max() >= n):
            raise ValueError(f"outlier ids must be in [0, {n})")
        if (np.diff(ids) <= 0).any():
            raise ValueError("outlier ids must be ascending and unique")
        return ids, raw

    def roundtrip_device(self, leaves_ptr: int, n: int, leaf_err_ptr: int, idx_ptr: int = 0, recon_ptr: int = 0, stream: int = 0):
        if not leaf_err_ptr:
            raise ValueError("leaf_err_ptr is NULL: the leaf errors need a device buffer of n * 2 float32")
        self._check(self._lib.vqhip_roundtrip_device(self._h, leaves_ptr, n, idx_ptr or None, recon_ptr or None, leaf_err_ptr, stream or None))

    def select_outliers_device(self, leaf_err_ptr: int, n: int, tol: float, ids_ptr: int, count_ptr: int, stream: int = 0):
        if not count_ptr:
            raise ValueError("count_ptr is NULL: the count needs a device buffer of one int64")
        self._check(self._lib.vqhip_select_outliers_device(self._h, leaf_err_ptr, n, self.check_tol(tol), ids_ptr, count_ptr, stream or None))

    def _compress_bounded_host(self, leaves: np.ndarray, tol: float):
        n = leaves.shape[0]
        idx, err = np.empty((n, LATENT_VOXELS), dtype=np.uint8), np.empty((n, ERR_FLOATS), dtype=np.float32)
        ids, count = np.empty(n, dtype=np.int64), ctypes.c_int64(0)
        self._check(self._lib.vqhip_compress_bounded(self._h, leaves.ctypes.data, n, tol, idx.ctypes.data, err.ctypes.data, ids.ctypes.data,
                                                     ctypes.byref(count)))
        return idx, err, ids[:count.value].copy()

    def _decompress_bounded_host(self, indices: np.ndarray, ids: np.ndarray, raw: np.ndarray) -> np.ndarray:
        out = np.empty((indices.shape[0], LEAF_VOXELS), dtype=np.float32)
        self._check(self._lib.vqhip_decompress_bounded(self._h, indices.ctypes.data, indices.shape[0], ids.ctypes.data, len(ids), raw.ctypes.data,
                                                       out.ctypes.data))
        return out

    def roundtrip(self, leaves, return_recon: bool = False):
        """Encode and decode in one pass -> (indices [n,64], leaf_err [n,2] = per leaf max |x - x^| and sum (x - x^)^2
        [, recon [n,512]]).  A float32 torch tensor on the handle's device gives device tensors, ordered on torch's current
        stream (complete on return where that is the default stream); a numpy array goes through the host entry points."""
        if isinstance(leaves, np.ndarray):
            leaves = self.check_leaves(leaves)
            idx, err, _ = self._compress_bounded_host(leaves, float("inf"))
            if not return_recon:
                return idx, err
            # the reconstruction the errors were measured against: the fp32 decoder whatever decode_precision says (the bounded
            # decompress with no outliers is that decode)
            return idx, err, self._decompress_bounded_host(idx, np.empty(0, np.int64), np.empty((0, LEAF_VOXELS), np.float32))
        import torch
        if not (isinstance(leaves, torch.Tensor) and leaves.is_cuda and leaves.dtype == torch.float32 and leaves.is_contiguous()):
            raise TypeError("leaves must be a float32 numpy array or a contiguous float32 torch tensor on the GPU")
        if tuple(leaves.shape[1:]) not in ((512,), (8, 8, 8)):
            raise ValueError(f"leaves must have shape [n,512] or [n,8,8,8], got {list(leaves.shape)}")
        n = leaves.shape[0]
        idx = torch.empty((n, LATENT_VOXELS), dtype=torch.uint8, device=leaves.device)
        err = torch.empty((n, ERR_FLOATS), dtype=torch.float32, device=leaves.device)
        rec = torch.empty((n, LEAF_VOXELS), dtype=torch.float32, device=leaves.device) if return_recon else None
        st = torch.cuda.current_stream(leaves.device).cuda_stream
        if st == 0:   # a null handle means the codec's own stream: order it after the producer of `leaves` by hand
            torch.cuda.synchronize(leaves.device)
        self.roundtrip_device(leaves.data_ptr(), n, err.data_ptr(), idx.data_ptr(), rec.data_ptr() if return_recon else 0, st)
        if st == 0:
            torch.cuda.synchronize(leaves.device)
        return (idx, err, rec) if return_recon else (idx, err)

    def compress_bounded(self, leaves: np.ndarray, tol: float, return_leaf_err: bool = False):
        """-> (indices [n,64], outlier_ids int64 ascending, outlier_leaves [m,512]): the leaves whose largest error is over
        ``tol`` (or not finite) come back as raw copies, so that decompress_bounded stays within tol on every value."""
        leaves = self.check_leaves(leaves)
        idx, err, ids = self._compress_bounded_host(leaves, self.check_bound(tol))
        out = (idx, ids, leaves[ids].copy())
        return out + (err,) if return_leaf_err else out

    def decompress_bounded(self, indices: np.ndarray, outlier_ids, outlier_leaves) -> np.ndarray:
        """Decoded leaves [n,512] with the leaves ``outlier_ids`` overwritten by their raw copies."""
        indices = self.check_indices(indices)
        ids, raw = self.check_outliers(indices.shape[0], outlier_ids, outlier_leaves)
        return self._decompress_bounded_host(indices, ids, raw)

    def compress_file_bounded(self, path, residual_path, grids, tol: float, batch_leaves: int = 0):
        """compress_file with a tolerance (vqhip_compress_file_bounded): the same .vqvdb bytes, and the leaves over ``tol`` raw
        in the .vqres sidecar ``residual_path`` (vqvdbfile.loads_residual reads it).  Returns (stream statistics, bounded
        statistics: leaves, outliers, max_err_kept, sum_sq_kept)."""
        tol = self.check_bound(tol)
        src, n_g, _keep = self._grid_sources(grids)
        st, bst = StreamStats(), BoundedStats()
        self._check(self._lib.vqhip_compress_file_bounded(self._h, os.fspath(path).encode(), os.fspath(residual_path).encode(), src, n_g, batch_leaves,
                                                          tol, ctypes.byref(st), ctypes.byref(bst)))
        return st.as_dict(), bst.as_dict()

    def decompress_file_bounded(self, path, residual_path, batch_leaves: int = 0, out: Optional[np.ndarray] = None):
        """decompress_file, then the leaves the sidecar names are overwritten with its floats (vqhip_decompress_file_bounded)."""
        return self._decompress_file(path, residual_path, batch_leaves, out)

    # ---- quantised residuals: include/vqvdb_hip_residual.h ----
    @staticmethod
    def residual_record_sizes(leaf_class: np.ndarray) -> np.ndarray:
        """int64 [n]: the record bytes of every class (0 for kept leaves); classes outside 0..16, 254, 255 are refused."""
        c = leaf_class.astype(np.int64)
        if ((c > 16) & (c != RES_KEPT) & (c != RES_RAW)).any():
            raise ValueError("leaf classes must be 0..16, 254 (kept) or 255 (raw)")
        return np.where(c == RES_KEPT, 0, np.where(c == RES_RAW, 2048, 64 * c))

    @classmethod
    def check_residual(cls, n: int, leaf_class, payload):
        """-> (class uint8 [n], payload uint8 [bytes]): one class per leaf, each 0..16, 254 or 255, and exactly their records."""
        if not isinstance(leaf_class, np.ndarray) or leaf_class.dtype != np.uint8:
            raise TypeError("leaf_class must be a uint8 numpy array")
        lc = np.ascontiguousarray(leaf_class).reshape(-1)
        if len(lc) != n:
            raise ValueError(f"{n} leaves but {len(lc)} classes")
        if isinstance(payload, (bytes, bytearray, memoryview)):
            payload = np.frombuffer(payload, dtype=np.uint8)
        if not isinstance(payload, np.ndarray) or payload.dtype != np.uint8:
            raise TypeError("payload must be bytes or a uint8 numpy array")
        pl = np.ascontiguousarray(payload).reshape(-1)
        need = int(cls.residual_record_sizes(lc).sum())
        if need != len(pl):
            raise ValueError(f"the classes need {need} payload bytes, got {len(pl)}")
        return lc, pl

    def residual_encode_device(self, leaves_ptr: int, recon_ptr: int, leaf_err_ptr: int, n: int, tol: float, class_ptr: int, offsets_ptr: int,
                               payload_ptr: int, payload_capacity: int, stream: int = 0):
        """vqhip_residual_encode_device: classes [n] u8, offsets [n+1] int64 (offsets[n] = the payload's bytes) and the payload."""
        if n > 0 and not (leaves_ptr and recon_ptr and leaf_err_ptr and class_ptr and offsets_ptr):
            raise ValueError("NULL device pointer: leaves, recon, leaf_err, class and offsets are required")
        if payload_capacity < 0:
            raise ValueError("payload_capacity must be >= 0")
        tol = self.check_bound(tol)
        self._check(self._lib.vqhip_residual_encode_device(self._h, leaves_ptr, recon_ptr, leaf_err_ptr, n, tol, class_ptr,
                                                           offsets_ptr, payload_ptr or None, payload_capacity, stream or None))

    def residual_apply_device(self, leaves_ptr: int, n: int, tol: float, class_ptr: int, offsets_ptr: int, payload_ptr: int, stream: int = 0):
        """vqhip_residual_apply_device: the decoded leaves at leaves_ptr corrected in place.  The device arrays are trusted."""
        if n > 0 and not (leaves_ptr and class_ptr and offsets_ptr):
            raise ValueError("NULL device pointer: leaves, class and offsets are required")
        tol = self.check_bound(tol)
        self._check(self._lib.vqhip_residual_apply_device(self._h, leaves_ptr, n, tol, class_ptr, offsets_ptr, payload_ptr or None,
                                                          stream or None))

    def compress_residual(self, leaves: np.ndarray, tol: float, return_leaf_err: bool = False):
        """-> (indices [n,64], leaf_class uint8 [n], payload uint8 [bytes]): a leaf whose largest error is within ``tol`` is kept
        (class 254), any other is stored as its residual on a grid of 1.875 * tol in class x 64 bytes (class 0..16) or, where
        that cannot keep it within tol, raw (class 255), so that decompress_residual stays within tol on every value."""
        leaves = self.check_leaves(leaves)
        tol = self.check_bound(tol)
        n = leaves.shape[0]
        idx, err = np.empty((n, LATENT_VOXELS), dtype=np.uint8), np.empty((n, ERR_FLOATS), dtype=np.float32)
        lc, payload, nbytes = np.empty(n, dtype=np.uint8), np.empty(n * 2048, dtype=np.uint8), ctypes.c_int64(0)
        self._check(self._lib.vqhip_compress_residual(self._h, leaves.ctypes.data, n, tol, idx.ctypes.data, err.ctypes.data, lc.ctypes.data,
                                                      payload.ctypes.data, ctypes.byref(nbytes)))
        out = (idx, lc, payload[:nbytes.value].copy())
        return out + (err,) if return_leaf_err else out

    def decompress_residual(self, indices: np.ndarray, tol: float, leaf_class, payload) -> np.ndarray:
        """Decoded leaves [n,512] with the records of compress_residual (same ``tol``) applied."""
        indices = self.check_indices(indices)
        tol = self.check_bound(tol)
        lc, pl = self.check_residual(indices.shape[0], leaf_class, payload)
        out = np.empty((indices.shape[0], LEAF_VOXELS), dtype=np.float32)
        self._check(self._lib.vqhip_decompress_residual(self._h, indices.ctypes.data, indices.shape[0], tol, lc.ctypes.data, pl.ctypes.data, len(pl),
                                                        out.ctypes.data))
        return out

    def compress_file_residual(self, path, residual_path, grids, tol: float, batch_leaves: int = 0):
        """compress_file with a tolerance and quantised records (vqhip_compress_file_residual): the same .vqvdb bytes, and the
        records of the leaves over ``tol`` in the .vqres v2 sidecar ``residual_path`` (vqvdbfile.load_residual_v2 reads it).
        Returns (stream statistics, bounded statistics with outliers = the selected leaves, residual statistics: quantised,
        raw, payload_bytes)."""
        tol = self.check_bound(tol)
        src, n_g, _keep = self._grid_sources(grids)
        st, bst, rst = StreamStats(), BoundedStats(), ResidualStats()
        self._check(self._lib.vqhip_compress_file_residual(self._h, os.fspath(path).encode(), os.fspath(residual_path).encode(), src, n_g, batch_leaves,
                                                           tol, ctypes.byref(st), ctypes.byref(bst), ctypes.byref(rst)))
        return st.as_dict(), bst.as_dict(), rst.as_dict()

    def decompress_file_residual(self, path, residual_path, batch_leaves: int = 0, out: Optional[np.ndarray] = None):
        """decompress_file with the sidecar's records applied to every decoded batch on the GPU (vqhip_decompress_file_residual)."""
        return self._decompress_file(path, residual_path, batch_leaves, out, residual_version=2)

    # ---- size sweep and byte-budget compress: include/vqvdb_hip_rate.h ----
    @classmethod
    def check_tols(cls, tols) -> np.ndarray:
        """1 .. 64 rungs, each a check_bound tolerance (a real number >= 0 or NaN, rounded down to float32) -> float32 [T]."""
        if isinstance(tols, (str, bytes)) or not hasattr(tols, "__len__"):
            raise TypeError("tols must be a sequence of real numbers")
        if not 1 <= len(tols) <= RATE_MAX_TOLS:
            raise ValueError(f"tols must hold 1..{RATE_MAX_TOLS} tolerances, got {len(tols)}")
        return np.array([cls.check_bound(t) for t in tols], dtype=np.float32)

    def rate_sweep_device(self, leaves_ptr: int, recon_ptr: int, leaf_err_ptr: int, n: int, tols, hist_ptr: int, stream: int = 0):
        """vqhip_rate_sweep_device: ADDS the class histogram of n leaves at every rung to hist_ptr, a device buffer of
        len(tols) x 19 int64 that the caller zeroes before the first call; nothing is read back or synchronised."""
        tols = self.check_tols(tols)
        if n > 0 and not (leaves_ptr and recon_ptr and leaf_err_ptr and hist_ptr):
            raise ValueError("NULL device pointer: leaves, recon, leaf_err and hist are required")
        self._check(self._lib.vqhip_rate_sweep_device(self._h, leaves_ptr, recon_ptr, leaf_err_ptr, n, tols.ctypes.data, len(tols), hist_ptr,
                                                      stream or None))

    def rate_sweep(self, leaves: np.ndarray, tols) -> np.ndarray:
        """-> hist int64 [T,19]: hist[t, k] leaves would get class k from compress_residual at tols[t] (k = 0 .. 16 quantised,
        17 raw, 18 kept).  rate_payload_bytes / rate_sidecar_bytes turn a row into the bytes of that compress."""
        leaves = self.check_leaves(leaves)
        tols = self.check_tols(tols)
        hist = np.empty((len(tols), RATE_CLASSES), dtype=np.int64)
        self._check(self._lib.vqhip_rate_sweep(self._h, leaves.ctypes.data, leaves.shape[0], tols.ctypes.data, len(tols), hist.ctypes.data))
        return hist

    def rate_sweep_file(self, grids, tols, batch_leaves: int = 0):
        """The sweep over compress_file's grid tuples, all grids in one histogram (vqhip_rate_sweep_file): no file is written.
        Returns (hist int64 [T,19], stream statistics); row t predicts compress_file_residual at tols[t] to the byte."""
        tols = self.check_tols(tols)
        src, n_g, _keep = self._grid_sources(grids)
        hist, st = np.empty((len(tols), RATE_CLASSES), dtype=np.int64), StreamStats()
        self._check(self._lib.vqhip_rate_sweep_file(self._h, src, n_g, batch_leaves, tols.ctypes.data, len(tols), hist.ctypes.data, ctypes.byref(st)))
        return hist, st.as_dict()

    def rate_compress_file(self, path, residual_path, grids, tols, sidecar_budget: int, batch_leaves: int = 0, rounds: int = 1):
        """compress_file_residual at the smallest of ``tols`` whose .vqres v2 sidecar has at most ``sidecar_budget`` bytes
        (vqhip_rate_compress_file: one sweep over the grids, then the compress, so about twice compress_file_residual).  Raises,
        before a file is opened, if no rung fits.  rounds > 1: before compressing, rounds - 1 further sweeps of 64 rungs, spaced
        geometrically between the largest rung that did not fit and the chosen one, tighten the choice.  Returns (tol_used, hist
        int64 [T,19] of the last ladder, stream, bounded and residual statistics of the compress)."""
        tols = self.check_tols(tols)
        if isinstance(sidecar_budget, bool) or not isinstance(sidecar_budget, (int, np.integer)):
            raise TypeError(f"sidecar_budget must be an integer number of bytes, got {sidecar_budget!r}")
        if sidecar_budget < 0:
            raise ValueError(f"sidecar_budget must be >= 0, got {sidecar_budget}")
        if isinstance(rounds, bool) or not isinstance(rounds, (int, np.integer)) or rounds < 1:
            raise ValueError(f"rounds must be an integer >= 1, got {rounds!r}")
        for _ in range(rounds - 1):
            hist, _st = self.rate_sweep_file(grids, tols, batch_leaves)
            fits = np.array([rate_sidecar_bytes(row, len(grids)) <= sidecar_budget for row in hist]) & ~np.isnan(tols)
            if not fits.any():
                break                                                # the library's call below refuses with both sizes
            hi = tols[fits].min()
            below = tols[~fits & (tols < hi)]
            if not len(below) or not below.max() > 0 or not np.isfinite(hi):
                break                                                # no interval to refine
            tols = self.check_tols(list(np.geomspace(float(below.max()), float(hi), RATE_MAX_TOLS)))
            tols[-1] = hi                                            # the rung known to fit, whatever the spacing rounds to
        src, n_g, _keep = self._grid_sources(grids)
        hist, used = np.empty((len(tols), RATE_CLASSES), dtype=np.int64), ctypes.c_float(0)
        st, bst, rst = StreamStats(), BoundedStats(), ResidualStats()
        self._check(self._lib.vqhip_rate_compress_file(self._h, os.fspath(path).encode(), os.fspath(residual_path).encode(), src, n_g, batch_leaves,
                                                       tols.ctypes.data, len(tols), int(sidecar_budget), ctypes.byref(used), hist.ctypes.data,
                                                       ctypes.byref(st), ctypes.byref(bst), ctypes.byref(rst)))
        return used.value, hist, st.as_dict(), bst.as_dict(), rst.as_dict()

    # ---- codebook training (VectorQuantizerEMA in training mode; see vqvdb_amd/codebook_training.py) ----
    def train_begin(self, cluster_size: Optional[np.ndarray] = None, embed_avg: Optional[np.ndarray] = None):
        cs = None if cluster_size is None else np.ascontiguousarray(cluster_size, dtype=np.float32).reshape(256)
        av = None if embed_avg is None else np.ascontiguousarray(embed_avg, dtype=np.float32).reshape(256, 128)
        self._check(self._lib.vqhip_train_begin(self._h, None if cs is None else cs.ctypes.data, None if av is None else av.ctypes.data))

    def train_vq_stats_device(self, leaves_ptr: int, n: int, stats_ptr: int, idx_ptr: int = 0, latent_ptr: int = 0, stream: int = 0):
        self._check(self._lib.vqhip_train_vq_stats_device(self._h, leaves_ptr, n, stats_ptr, idx_ptr or None, latent_ptr or None, stream or None))

    def train_eval_device(self, leaves_ptr: int, n: int, stats_ptr: int, recon_sums_ptr: int, recon_ptr: int = 0, stream: int = 0):
        self._check(self._lib.vqhip_train_eval_device(self._h, leaves_ptr, n, stats_ptr, recon_sums_ptr, recon_ptr or None, stream or None))

    def train_vq_update_device(self, stats_ptr: int, decay: float = 0.95, eps: float = 1e-4, stream: int = 0):
        self._check(self._lib.vqhip_train_vq_update_device(self._h, stats_ptr, decay, eps, stream or None))

    def train_get_state(self):
        emb, cs, avg = np.empty((256, 128), np.float32), np.empty(256, np.float32), np.empty((256, 128), np.float32)
        self._check(self._lib.vqhip_train_get_state(self._h, emb.ctypes.data, cs.ctypes.data, avg.ctypes.data))
        return {"embedding": emb, "cluster_size": cs, "embed_avg": avg}

    def train_set_state(self, embedding=None, cluster_size=None, embed_avg=None):
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (embedding, cluster_size, embed_avg)]
        for a, size, what in zip(arrs, (256 * 128, 256, 256 * 128), ("embedding", "cluster_size", "embed_avg")):
            if a is not None and a.size != size:
                raise ValueError(f"{what}: expected {size} float32 values, got {a.size}")
        self._check(self._lib.vqhip_train_set_state(self._h, *[None if a is None else a.ctypes.data for a in arrs]))

    def train_commit(self):
        self._check(self._lib.vqhip_train_commit(self._h))

    def set_small_batch_tiles(self, tiles: int):
        """-1: automatic choice between the position-split and the one-wave-per-tile path (default); 0: never split;
        n > 0: split passes of up to n tiles (encode) / 1.25 n (decode)."""
        self._check(self._lib.vqhip_set_small_batch_tiles(self._h, tiles))

    # ---- full training step (stage 2) ----
    def fulltrain_begin(self):
        self._check(self._lib.vqhip_fulltrain_begin(self._h))

    def fulltrain_param_count(self) -> int:
        return int(self._lib.vqhip_fulltrain_param_count(self._h))

    def fulltrain_forward_device(self, leaves_ptr: int, n: int, stream: int = 0):
        self._check(self._lib.vqhip_fulltrain_forward_device(self._h, leaves_ptr, n, stream or None))

    def fulltrain_fwdbwd_device(self, leaves_ptr: int, n: int, n_global: int, grads_ptr: int, aux_ptr: int = 0, stream: int = 0):
        self._check(self._lib.vqhip_fulltrain_fwdbwd_device(self._h, leaves_ptr, n, n_global, grads_ptr, aux_ptr or None, stream or None))

    def fulltrain_fwdbwd_overlap_device(self, leaves_ptr: int, n: int, n_global: int, grads_ptr: int, aux_ptr: int, stream: int, decoder_done):
        """fwdbwd with `decoder_done()` called once the decoder half of the backward pass is enqueued (see vqvdb_hip.h)."""
        def cb(_user):
            try:
                decoder_done()
                return 0
            except Exception as e:  # noqa: BLE001 — an exception must not unwind through the C frames
                print(f"fulltrain decoder_done callback: {e}", file=sys.stderr)
                return 1
        fn = PHASE_FN(cb)
        self._check(self._lib.vqhip_fulltrain_fwdbwd_overlap_device(self._h, leaves_ptr, n, n_global, grads_ptr, aux_ptr or None, stream or None, fn, None))

    def fulltrain_set_folded_tail(self, on: bool):
        self._check(self._lib.vqhip_fulltrain_set_folded_tail(self._h, int(on)))

    def fulltrain_decoder_offset(self) -> int:
        return int(self._lib.vqhip_fulltrain_decoder_offset(self._h))

    def fulltrain_ready_stream(self) -> int:
        """Raw HIP stream on which the decoder's gradients are complete at the decoder_done callback (0: the stream of the call)."""
        return int(self._lib.vqhip_fulltrain_ready_stream(self._h) or 0)

    def fulltrain_apply_device(self, grads_ptr: int, aux_ptr: int, lr: float, step: int, betas=(0.9, 0.999), adam_eps: float = 1e-8,
                               weight_decay: float = 1e-4, ema_decay: float = 0.95, ema_eps: float = 1e-4, stream: int = 0):
        self._check(self._lib.vqhip_fulltrain_apply_device(self._h, grads_ptr, aux_ptr or None, lr, step, betas[0], betas[1], adam_eps, weight_decay,
                                                           ema_decay, ema_eps, stream or None))

    def fulltrain_get_params(self) -> np.ndarray:
        out = np.empty(self.fulltrain_param_count(), dtype=np.float32)
        self._check(self._lib.vqhip_fulltrain_get_params(self._h, out.ctypes.data))
        return out

    def fulltrain_set_params(self, flat: np.ndarray):
        flat = np.ascontiguousarray(flat, dtype=np.float32)
        if flat.size != self.fulltrain_param_count():
            raise ValueError("flat parameter vector has the wrong length")
        self._check(self._lib.vqhip_fulltrain_set_params(self._h, flat.ctypes.data))

    def fulltrain_get_opt_state(self):
        """AdamW moments (exp_avg, exp_avg_sq), flat parameter order."""
        m, v = np.empty(self.fulltrain_param_count(), np.float32), np.empty(self.fulltrain_param_count(), np.float32)
        self._check(self._lib.vqhip_fulltrain_get_opt_state(self._h, m.ctypes.data, v.ctypes.data))
        return m, v

    def fulltrain_set_opt_state(self, exp_avg: np.ndarray, exp_avg_sq: np.ndarray):
        m, v = (np.ascontiguousarray(a, dtype=np.float32) for a in (exp_avg, exp_avg_sq))
        if m.size != self.fulltrain_param_count() or v.size != m.size:
            raise ValueError("optimizer moments have the wrong length")
        self._check(self._lib.vqhip_fulltrain_set_opt_state(self._h, m.ctypes.data, v.ctypes.data))

    def fetch(self, name: str, n: int, channels: int, positions: int) -> np.ndarray:
        """debug_fetch without the debug flag: any named workspace tensor as [n, channels, positions]."""
        out = np.empty((n, channels, positions), dtype=np.float32)
        self._check(self._lib.vqhip_debug_fetch(self._h, name.encode(), n, out.ctypes.data))
        return out

    def workspace_bytes(self) -> int:
        return int(self._lib.vqhip_workspace_bytes(self._h))

    def chunk_leaves(self) -> int:
        return int(self._lib.vqhip_chunk_leaves(self._h))

    def compute_units(self) -> tuple:
        """(the device's compute units, the count the launch geometry is derived from): equal unless VQHIP_CUS was set at create."""
        device, in_use = ctypes.c_int(), ctypes.c_int()
        self._check(self._lib.vqhip_compute_units(self._h, ctypes.byref(device), ctypes.byref(in_use)))
        return device.value, in_use.value

    def reserve(self, n: int):
        self._check(self._lib.vqhip_reserve(self._h, n))

    def profile_enable(self, on: bool):
        self._check(self._lib.vqhip_profile_enable(self._h, int(on)))

    def profile_read(self) -> list:
        stats = (_KernelStat * 256)()
        cnt = ctypes.c_int()
        self._check(self._lib.vqhip_profile_read(self._h, stats, 256, ctypes.byref(cnt)))
        return [dict(name=s.name.decode(), launches=s.launches, total_ms=s.total_ms, flops_per_leaf=s.flops_per_leaf,
                     eff_flops_per_leaf=s.eff_flops_per_leaf, leaves=s.leaves) for s in stats[:cnt.value]]

    def debug_enable(self, on: bool):
        self._check(self._lib.vqhip_debug_enable(self._h, int(on)))

    def debug_fetch(self, name: str, n: int, channels: int, positions: int) -> np.ndarray:
        out = np.empty((n, channels, positions), dtype=np.float32)
        self._check(self._lib.vqhip_debug_fetch(self._h, name.encode(), n, out.ctypes.data))
        return out

    def selftest_mfma(self) -> list:
        out = (ctypes.c_int64 * 2)()
        self._check(self._lib.vqhip_selftest_mfma(self._h, out))
        return list(out)


def _vec3_grid_sources(grids, need_masks: bool):
    """(vqhip_vec3_grid_source array, its length, the arrays it points into) of the file calls' grid dicts: "name", "origins" int32
    [n,3], "leaves" (float32 [n,512,3] or a list of n [512,3] buffers), optional "transform" (16 floats), "masks" (bool [n,512] or
    uint64 [n,8]; required by compress_file_active) and "background" (three numbers)."""
    n_g = len(grids)
    src = (_Vec3GridSource * max(n_g, 1))()
    keep = []
    for i, g in enumerate(grids):
        origins = np.ascontiguousarray(g["origins"], dtype=np.int32).reshape(-1, 3)
        n = origins.shape[0]
        leaves = g["leaves"]
        if isinstance(leaves, np.ndarray):
            leaves = HipVec3Codec.check_leaves(leaves)
            if leaves.shape[0] != n:
                raise ValueError(f"grid {i}: {n} origins but {leaves.shape[0]} leaves")
            ptrs = np.ascontiguousarray(leaves.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(VEC3_LEAF_FLOATS * 4), dtype=np.uint64)
        else:
            ptrs = HipVec3Codec._leaf_ptrs(leaves, n, writable=False)
        masks = g.get("masks")
        if masks is None and need_masks:
            raise ValueError(f"grid {i}: compress_file_active needs masks")
        if masks is not None:
            masks = check_masks(pack_masks(masks) if isinstance(masks, np.ndarray) and masks.dtype == np.bool_ else masks, n)
        tr = None if g.get("transform") is None else np.ascontiguousarray(g["transform"], dtype=np.float32).reshape(16)
        bg = HipVec3Codec.check_background(g.get("background"))
        bname = g["name"].encode()
        keep += [origins, leaves, ptrs, masks, tr, bg, bname]
        src[i].name = bname
        src[i].transform = None if tr is None else tr.ctypes.data
        src[i].leaf_ptrs = ptrs.ctypes.data if n else None
        src[i].origins = origins.ctypes.data if n else None
        src[i].n_leaves = n
        src[i].masks = masks.ctypes.data if masks is not None and n else None
        src[i].background = None if bg is None else bg.ctypes.data
    return src, n_g, keep


def _rate_row(row) -> np.ndarray:
    r = np.asarray(row)
    if r.shape != (RATE_CLASSES,) or not np.issubdtype(r.dtype, np.integer):
        raise ValueError(f"a histogram row holds {RATE_CLASSES} integers")
    return np.ascontiguousarray(r, dtype=np.int64)


def rate_payload_bytes(row) -> int:
    """vqhip_rate_payload_bytes: the record bytes of a compress whose class histogram is ``row`` (int [19])."""
    r = _rate_row(row)
    return int(load_library().vqhip_rate_payload_bytes(r.ctypes.data))


def rate_sidecar_bytes(row, n_grids: int) -> int:
    """vqhip_rate_sidecar_bytes: the size of the .vqres v2 sidecar of ``n_grids`` grids whose class histogram is ``row``."""
    r = _rate_row(row)
    return int(load_library().vqhip_rate_sidecar_bytes(r.ctypes.data, int(n_grids)))


def _vec3_rate_hist(hist, what="a histogram row") -> np.ndarray:
    r = np.ascontiguousarray(hist)
    if r.shape[-1:] != (VEC3_RATE_CLASSES,) or not np.issubdtype(r.dtype, np.integer):
        raise ValueError(f"{what} holds {VEC3_RATE_CLASSES} integers")
    return r.astype(np.int64)


def vec3_rate_payload_bytes(row) -> int:
    """vqhip_vec3_rate_payload_bytes: the record bytes of a Vec3 compress whose histogram row is ``row`` (int [51])."""
    r = _vec3_rate_hist(row)
    if r.ndim != 1:
        raise ValueError(f"a histogram row holds {VEC3_RATE_CLASSES} integers")
    return int(load_library().vqhip_vec3_rate_payload_bytes(r.ctypes.data))


def vec3_rate_pick(hist, tols, payload_budget: int) -> int:
    """vqhip_vec3_rate_pick: the index of the smallest tols[t] by value (NaN never) whose row of ``hist`` (int [T,51]) has a
    payload of at most ``payload_budget`` bytes.  Raises ValueError if no rung fits."""
    t = HipVec3Codec.check_tols(tols)
    h = _vec3_rate_hist(hist, "every histogram row")
    if h.shape != (len(t), VEC3_RATE_CLASSES):
        raise ValueError(f"{len(t)} tolerances need a histogram of shape [{len(t)},{VEC3_RATE_CLASSES}], got {list(h.shape)}")
    if isinstance(payload_budget, bool) or not isinstance(payload_budget, (int, np.integer)):
        raise TypeError(f"payload_budget must be an integer number of bytes, got {payload_budget!r}")
    if payload_budget < 0:
        raise ValueError(f"payload_budget must be >= 0, got {payload_budget}")
    best = int(load_library().vqhip_vec3_rate_pick(h.ctypes.data, t.ctypes.data, len(t), int(payload_budget)))
    if best < 0:
        raise ValueError(f"no rung fits {payload_budget} bytes")
    return best


def vec3_active_record_bytes(code: int, active: int) -> int:
    """vqhip_vec3_active_record_bytes: the bytes of the compact record of ``code`` on a leaf with ``active`` active voxels
    (0 kept, 8 ceil(3 A / 2) raw, 8 ceil(A / 64) (b0 + b1 + b2) quantised).  Raises ValueError for a code that is neither a
    sentinel nor three widths of 0..16 or an ``active`` outside 0..512."""
    for v, what in ((code, "code"), (active, "active")):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{what} must be an integer, got {v!r}")
    if not -2**31 <= code < 2**31 or not -2**31 <= active < 2**31:
        raise ValueError(f"code {code} or active {active} is out of range")
    size = int(load_library().vqhip_vec3_active_record_bytes(int(code), int(active)))
    if size < 0:
        raise ValueError(f"code 0x{int(code) & 0xFFFFFFFF:X} with {active} active voxels has no record size")
    return size


def vec3_file_info(path) -> dict:
    """vqhip_vec3_file_info: the header fields of a .vqv3 file after the whole-file length check; no handle, no GPU."""
    lib = load_library()
    ng, k, kind, mode, tol = ctypes.c_int(), ctypes.c_uint32(), ctypes.c_int(), ctypes.c_int(), ctypes.c_float()
    blocks, pay = ctypes.c_int64(), ctypes.c_int64()
    if lib.vqhip_vec3_file_info(os.fspath(path).encode(), ctypes.byref(ng), ctypes.byref(k), ctypes.byref(kind), ctypes.byref(mode), ctypes.byref(tol),
                                ctypes.byref(blocks), ctypes.byref(pay)) != 0:
        raise RuntimeError(lib.vqhip_vec3_last_error(None).decode())
    return {"n_grids": ng.value, "num_codes": k.value, "kind": kind.value, "mode": mode.value, "tol": tol.value, "total_blocks": blocks.value,
            "payload_bytes": pay.value}


def vec3_active_rate_pick(sizes, tols, budget: int) -> int:
    """vqhip_vec3_budget_pick: the index of the smallest tols[t] by value (NaN never, of duplicates the first) with sizes[t] <=
    ``budget``, on the int [T] that rate_sweep_active returns (or the file sizes made of them).  Raises ValueError if no rung fits."""
    t = HipVec3Codec.check_tols(tols)
    b = np.ascontiguousarray(sizes)
    if b.shape != (len(t),) or not np.issubdtype(b.dtype, np.integer):
        raise ValueError(f"{len(t)} tolerances need {len(t)} integer sizes, got shape {list(b.shape)} of {b.dtype}")
    b = b.astype(np.int64)
    if (b < 0).any():
        raise ValueError("a size is negative")
    budget = HipVec3Codec.check_budget(budget, "budget")
    best = int(load_library().vqhip_vec3_budget_pick(b.ctypes.data, t.ctypes.data, len(t), budget))
    if best < 0:
        raise ValueError(f"no rung fits {budget} bytes")
    return best


def vec3_file_bytes(grids, kind: int, payload_bytes=None) -> int:
    """vqhip_vec3_budget_file_bytes: the size of the .vqv3 file that compress_file (kind 0) or compress_file_active (kind 1) writes
    for the grid dicts ``grids`` when grid g's payload has payload_bytes[g] bytes (kind 0: None).  No handle, no GPU.  Raises
    ValueError on what the writer would refuse and on a size beyond 2^63 - 1."""
    if kind not in (0, 1):
        raise ValueError(f"kind must be 0 or 1, got {kind!r}")
    src, n_g, _keep = _vec3_grid_sources(grids, need_masks=kind == 1)
    pb = None
    if payload_bytes is not None or kind == 1:
        pb = np.ascontiguousarray(payload_bytes if payload_bytes is not None else [], dtype=np.int64).reshape(-1)
        if len(pb) != n_g:
            raise ValueError(f"{n_g} grids need {n_g} payload sizes, got {len(pb)}")
    size = int(load_library().vqhip_vec3_budget_file_bytes(src, n_g, int(kind), None if pb is None else pb.ctypes.data))
    if size < 0:
        raise ValueError("the writer would refuse these grids or payload sizes, or the file's size passes 2^63 - 1")
    return size


class HipMultiCodec:
    """In-process multi-GPU front end: contiguous leaf ranges over several devices, no collective."""

    def __init__(self, pack: Union[str, os.PathLike, bytes], device_ids: Sequence[int]):
        self._lib = load_library()
        self._h = ctypes.c_void_p()
        ids = (ctypes.c_int * len(device_ids))(*device_ids)
        self._n = len(device_ids)
        if isinstance(pack, (bytes, bytearray, memoryview)):
            self._pack = bytes(pack)
            rc = self._lib.vqhip_multi_create(None, self._pack, len(self._pack), ids, len(device_ids), ctypes.byref(self._h))
        else:
            rc = self._lib.vqhip_multi_create(os.fspath(pack).encode(), None, 0, ids, len(device_ids), ctypes.byref(self._h))
        if rc != 0:
            raise RuntimeError(self._lib.vqhip_multi_last_error(None).decode())

    def _check(self, rc: int):
        if rc != 0:
            raise RuntimeError(self._lib.vqhip_multi_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.vqhip_multi_destroy(self._h)
            self._h = ctypes.c_void_p()

    __del__ = close

    def worker_info(self) -> list:
        """Per device worker: (device_id, numa_node or -1, cores bound or 0)."""
        out = []
        for k in range(self._n):
            d, nn, cb = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
            self._check(self._lib.vqhip_multi_worker_info(self._h, k, ctypes.byref(d), ctypes.byref(nn), ctypes.byref(cb)))
            out.append((d.value, nn.value, cb.value))
        return out

    def encode(self, leaves: np.ndarray) -> np.ndarray:
        leaves = np.ascontiguousarray(leaves, dtype=np.float32).reshape(-1, LEAF_VOXELS)
        idx = np.empty((leaves.shape[0], LATENT_VOXELS), dtype=np.uint8)
        self._check(self._lib.vqhip_multi_encode(self._h, leaves.ctypes.data, leaves.shape[0], idx.ctypes.data))
        return idx

    def decode(self, indices: np.ndarray) -> np.ndarray:
        indices = np.ascontiguousarray(indices, dtype=np.uint8).reshape(-1, LATENT_VOXELS)
        out = np.empty((indices.shape[0], LEAF_VOXELS), dtype=np.float32)
        self._check(self._lib.vqhip_multi_decode(self._h, indices.ctypes.data, indices.shape[0], out.ctypes.data))
        return out


class IVQVAECodec:
    """Abstract codec (IVQVAECodec.hpp:99-136)."""

    @staticmethod
    def create(config: CodecConfig, type: BackendType) -> Optional["IVQVAECodec"]:
        """Factory (IVQVAECodec.cpp:76-110): any failure is reported on stderr and yields None."""
        try:
            if type == BackendType.HIP:
                return HipBackend(config)
            raise RuntimeError("Requested backend type is not available or disabled in the build configuration.")
        except Exception as e:  # noqa: BLE001 — mirrors catch (const std::exception&)
            print(f"Failed to create VQ-VAE backend: {e}", file=sys.stderr)
            return None

    def encode(self, leafBatch: TensorView) -> Tensor:
        raise NotImplementedError

    def decode(self, indices: TensorView) -> Tensor:
        raise NotImplementedError

    def getLatentShape(self) -> list:
        raise NotImplementedError


class HipBackend(IVQVAECodec):
    """MI355X backend behind the reference's plugin surface (counterpart of TorchBackend,
    src/backends/torch/TorchBackend.cpp)."""

    def __init__(self, config: CodecConfig):
        if config.device != CodecConfig.Device.CUDA:
            raise RuntimeError("HIP backend requires Device::CUDA (GPU); there is no CPU path in this backend")
        source = config.source
        if isinstance(source, EmbeddedModel):
            # the Python side's bin_model.h: a pack installed beside the package (the C++ adapter compiles one in)
            source = os.environ.get("VQVDB_HIP_EMBEDDED_PACK_FILE", EMBEDDED_PACK_FILE)
            if not os.path.exists(source):
                raise RuntimeError("vqhip_create: no weight pack given (embedded model absent from this build)")
        self._codec = HipCodec(source, config.device_id)
        self._latent = self._codec.latent_shape()

    def encode(self, leafBatch: TensorView) -> Tensor:
        if leafBatch.dtype != DataType.FLOAT32:
            raise RuntimeError("encode expects FLOAT32 data.")          # TorchBackend.cpp:134-136
        shape = list(leafBatch.shape)
        if len(shape) != 5 or shape[1:] != [1, 8, 8, 8] or shape[0] < 1:
            raise RuntimeError("encode expects shape [B,1,8,8,8].")
        idx = self._codec.encode(np.asarray(leafBatch.data).reshape(shape[0], LEAF_VOXELS))
        return Tensor(idx.reshape(-1).view(np.uint8), [shape[0]] + self._latent, DataType.UINT8)

    def decode(self, indices: TensorView) -> Tensor:
        if indices.dtype != DataType.UINT8:
            raise RuntimeError("decode expects UINT8 data.")            # TorchBackend.cpp:167-169
        shape = list(indices.shape)
        if len(shape) != 4 or shape[1:] != self._latent or shape[0] < 1:
            raise RuntimeError("decode expects shape [B,4,4,4].")
        out = self._codec.decode(np.asarray(indices.data).reshape(shape[0], LATENT_VOXELS))
        return Tensor(out.reshape(-1).view(np.uint8), [shape[0], 1, 8, 8, 8], DataType.FLOAT32)

    def getLatentShape(self) -> list:
        return list(self._latent)

    @property
    def raw(self) -> HipCodec:
        return self._codec
