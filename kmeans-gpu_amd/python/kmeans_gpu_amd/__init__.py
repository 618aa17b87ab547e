"""kmeans_gpu_amd -- Python host binding of libkmeans_hip.so (ctypes over the C ABI of
include/kmeans_hip.h).

It mirrors the reference crate's public surface (core/src/lib.rs:24-165):

    ImageProcessor().palette(color_count, image, algo)  -> list of RGBA8
    ImageProcessor().find(image, colors, reduce_mode)   -> image
    ImageProcessor().reduce(color_count, image, algo, reduce_mode) -> image

Images are numpy uint8 arrays of shape (height, width, 4) (tightly packed RGBA8,
core/src/image.rs:20-48).  `Lloyd` exposes the device-pointer building blocks used by the
multi-GPU layer (Group / GroupLloyd over kmg_group_*) and by bench.py; PyTorch only
supplies device memory, streams and torch.distributed there.

There is no CPU fallback: if the shared library is missing or no HIP device is usable, the
constructors raise.
"""
import ctypes as C
import enum
import os

import numpy as np

__all__ = ["ImageProcessor", "Algorithm", "ReduceMode", "OutputFormat", "Diffusion", "DIFFUSION_NAMES", "diffusion_weights", "DitherMap", "DITHER_MAP_NAMES", "dither_map_values", "ErrorStats", "BatchReport", "BatchApplyReport", "BatchQualityReport", "ClipReport", "Sequence", "FrameDelta", "FrameHold", "FRAME_DELTA", "CLIP_FULL_ON_CLEAR", "CLIP_FRAMES", "CLIP_MIN_FRAMES", "LOCAL_WARM", "MAX_TOLERANCE", "tolerance_of", "ERROR_RGB", "ERROR_LAB", "Lloyd", "ApplyPlan", "Group", "GroupLloyd", "GroupOptions", "KmgError", "lib",
           "library_path", "GROUP_FORCE_COLLECTIVES", "GROUP_LOOPBACK", "GROUP_CELLS", "GROUP_OVERLAP", "GROUP_FUSED_UPDATE",
           "resized_dims", "palette_to_centroids", "centroids_to_palette", "dither_threshold",
           "default_options", "Options"]

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG_ROOT = os.path.dirname(os.path.dirname(_HERE))          # .../kmeans-gpu_amd
# KMG_LIBRARY: another build of the same ABI -- tools/ loads lib/libkmeans_hip_tools.so (make tools: tuning switches and
# knock-outs compiled in) through it; the product library reads none of those switches
_LIB_PATH = os.environ.get("KMG_LIBRARY") or os.path.join(_PKG_ROOT, "lib", "libkmeans_hip.so")


class _RawDeviceArray:
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": typestr, "data": (int(ptr), False), "version": 2}


def _alias_tensor(ptr, n, typestr):
    """torch tensor over device memory the library owns (no copy): valid while the owning object lives"""
    import torch
    return torch.as_tensor(_RawDeviceArray(ptr, n, typestr), device="cuda")


class KmgError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"kmeans_hip error {status}: {message}")
        self.status = status


class Algorithm(enum.IntEnum):          # core/src/lib.rs:215-219
    Kmeans = 0
    Octree = 1


class ReduceMode(enum.IntEnum):         # core/src/lib.rs:234-239, plus Diffuse (include/kmeans_hip.h KMG_MODE_DIFFUSE)
    Replace = 0
    Dither = 1
    Meld = 2
    Diffuse = 3                         # Floyd-Steinberg error diffusion (not in the reference; no Group support)


class Diffusion(enum.IntEnum):          # include/kmeans_hip.h kmg_diffusion: the filter of ReduceMode.Diffuse
    FloydSteinberg = 0
    SierraLite = 1
    Atkinson = 2
    Burkes = 3
    Sierra2 = 4
    Sierra3 = 5
    Jarvis = 6
    Stucki = 7


# the CLI's names: the lower-case constant suffixes with - for _
DIFFUSION_NAMES = {"floyd-steinberg": 0, "sierra-lite": 1, "atkinson": 2, "burkes": 3, "sierra2": 4, "sierra3": 5, "jarvis": 6,
                   "stucki": 7}


def _diffusion_value(f):
    """a Diffusion, its number, or one of DIFFUSION_NAMES (case and - / _ do not matter); unknown numbers pass through to the library"""
    if isinstance(f, str):
        key = f.strip().lower().replace("_", "-")
        if key not in DIFFUSION_NAMES:
            raise ValueError(f"unknown diffusion filter {f!r}: one of {', '.join(DIFFUSION_NAMES)}")
        return DIFFUSION_NAMES[key]
    return int(f)


def diffusion_weights(filter):
    """kmg_diffusion_weights (no device needed): (weights, divisor) with weights[0..1] row 0 (dx = +1, +2), [2..6] row 1 and
    [7..11] row 2 (dx = -2 .. +2) as an int32 array"""
    w = (C.c_int32 * 12)()
    d = C.c_int32()
    _check(lib().kmg_diffusion_weights(_diffusion_value(filter), w, C.byref(d)))
    return np.array(w[:], np.int32), int(d.value)


class DitherMap(enum.IntEnum):          # include/kmeans_hip.h kmg_dither_map: the threshold map of ReduceMode.Dither
    Bayer4 = 0                          # the reference's matrix, the default
    Bayer2 = 1
    Bayer8 = 2
    Bayer16 = 3
    Blue64 = 4                          # 64 x 64 void-and-cluster (blue noise)
    Custom = 5                          # the caller's own map (set_dither with an array)


# the CLI's names of the built-in maps
DITHER_MAP_NAMES = {"bayer4": 0, "bayer2": 1, "bayer8": 2, "bayer16": 3, "blue": 4}


def _dither_map_value(m):
    """a DitherMap, its number, or one of DITHER_MAP_NAMES (case does not matter; blue64 = blue); unknown numbers pass through to
    the library"""
    if isinstance(m, str):
        key = m.strip().lower()
        key = "blue" if key == "blue64" else key
        if key not in DITHER_MAP_NAMES:
            raise ValueError(f"unknown dither map {m!r}: one of {', '.join(DITHER_MAP_NAMES)}")
        return DITHER_MAP_NAMES[key]
    return int(m)


def dither_map_values(map):
    """kmg_dither_map_values (no device needed): (levels, n_levels) of a built-in map, levels a (height, width) uint16 array"""
    buf = (C.c_uint16 * 4096)()
    w, h, n = C.c_uint32(), C.c_uint32(), C.c_uint32()
    _check(lib().kmg_dither_map_values(_dither_map_value(map), C.byref(w), C.byref(h), C.byref(n), buf))
    return np.array(buf[:w.value * h.value], np.uint16).reshape(h.value, w.value), int(n.value)


class OutputFormat(enum.IntEnum):       # include/kmeans_hip.h kmg_output_format
    RGBA8 = 0
    Index8 = 1                          # one uint8 palette index per pixel
    Index16 = 2                         # one uint16 palette index per pixel


class Options(C.Structure):             # include/kmeans_hip.h kmg_options
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("shrink_max_dim", C.c_uint32),
                ("max_iterations", C.c_uint32), ("check_period", C.c_uint32), ("convergence", C.c_float),
                ("strategy", C.c_int32), ("alpha_cutoff", C.c_uint32)]


ERROR_RGB, ERROR_LAB = 1, 2             # include/kmeans_hip.h KMG_ERROR_*: the parts of an ErrorStats record


class ErrorStats(C.Structure):          # include/kmeans_hip.h kmg_error_stats: 14 x uint64, exact integers
    _fields_ = [("pixels", C.c_uint64), ("changed", C.c_uint64), ("invalid", C.c_uint64), ("sse", C.c_uint64 * 3),
                ("sad", C.c_uint64 * 3), ("max_abs", C.c_uint64 * 3), ("lab_sse", C.c_uint64), ("lab_max", C.c_uint64)]

    def as_tuple(self):
        """the 14 integers in the order of the C struct"""
        return (int(self.pixels), int(self.changed), int(self.invalid), *map(int, self.sse), *map(int, self.sad),
                *map(int, self.max_abs), int(self.lab_sse), int(self.lab_max))

    @classmethod
    def from_array(cls, a):
        """from 14 uint64 (a record read back from device memory)"""
        return cls.from_buffer_copy(np.ascontiguousarray(a, np.uint64).reshape(14).tobytes())

    @property
    def mse(self):
        """per-channel mean squared error (R, G, B), host floats from the integer sums; nan without counted pixels"""
        n = int(self.pixels)
        return tuple(int(v) / n if n else float("nan") for v in self.sse)

    @property
    def psnr(self):
        """10 log10(255^2 / mean of the three channel MSEs) in dB; inf for identical images"""
        n = int(self.pixels)
        if not n:
            return float("nan")
        m = sum(int(v) for v in self.sse) / (3.0 * n)
        return float("inf") if m == 0 else 10.0 * float(np.log10(65025.0 / m))

    @property
    def delta_e_rms(self):
        """root mean square dE76 on the 1/64 grid: sqrt(lab_sse / (4096 pixels))"""
        n = int(self.pixels)
        return float(np.sqrt(int(self.lab_sse) / (4096.0 * n))) if n else float("nan")

    @property
    def delta_e_max(self):
        return float(np.sqrt(int(self.lab_max) / 4096.0))

    def __repr__(self):
        return "ErrorStats" + repr(self.as_tuple())


FRAME_DELTA = 1                         # include/kmeans_hip.h KMG_FRAME_DELTA
LOCAL_WARM = 1                          # include/kmeans_hip.h KMG_LOCAL_WARM
CLIP_FULL_ON_CLEAR = 1                  # include/kmeans_hip.h KMG_CLIP_FULL_ON_CLEAR
CLIP_FRAMES = 32                        # include/kmeans_hip.h KMG_CLIP_FRAMES: frames one launch of the clip walk takes
CLIP_MIN_FRAMES = 8                     # include/kmeans_hip.h KMG_CLIP_MIN_FRAMES: the shortest clip Sequence.frames sends through the chain


class FrameDelta(C.Structure):          # include/kmeans_hip.h kmg_frame_delta: 32 bytes
    _fields_ = [("changed", C.c_uint64), ("cleared", C.c_uint64), ("x0", C.c_uint32), ("y0", C.c_uint32),
                ("x1", C.c_uint32), ("y1", C.c_uint32)]

    FRESH = (0, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0)        # what the caller writes before a frame

    def as_tuple(self):
        return (int(self.changed), int(self.cleared), int(self.x0), int(self.y0), int(self.x1), int(self.y1))

    @classmethod
    def from_array(cls, a):
        """from the 32 bytes of a record read back from device memory (any dtype)"""
        return cls.from_buffer_copy(np.ascontiguousarray(a).tobytes()[:32])

    @classmethod
    def fresh_bytes(cls):
        """the 32 bytes of the fresh record"""
        return bytes(cls(*cls.FRESH))

    @property
    def rect(self):
        """(x0, y0, x1, y1) of the changed pixels, x1 / y1 exclusive; None when nothing changed"""
        return None if int(self.changed) == 0 else (int(self.x0), int(self.y0), int(self.x1), int(self.y1))

    def __repr__(self):
        return "FrameDelta" + repr(self.as_tuple())


MAX_TOLERANCE = 347973309               # the largest D of two sRGB8 colours (include/kmeans_hip.h at kmg_dev_frame_delta_lossy)


class FrameHold(C.Structure):           # include/kmeans_hip.h kmg_frame_hold: 48 bytes -- a kmg_frame_delta, then held and held_sse
    _fields_ = FrameDelta._fields_ + [("held", C.c_uint64), ("held_sse", C.c_uint64)]

    FRESH = FrameDelta.FRESH + (0, 0)                   # what the caller writes before a frame

    def as_tuple(self):
        return (int(self.changed), int(self.cleared), int(self.x0), int(self.y0), int(self.x1), int(self.y1), int(self.held),
                int(self.held_sse))

    @classmethod
    def from_array(cls, a):
        """from the 48 bytes of a record read back from device memory (any dtype)"""
        return cls.from_buffer_copy(np.ascontiguousarray(a).tobytes()[:48])

    @classmethod
    def fresh_bytes(cls):
        """the 48 bytes of the fresh record"""
        return bytes(cls(*cls.FRESH))

    @property
    def rect(self):
        """(x0, y0, x1, y1) of the pixels sent, x1 / y1 exclusive; None when none was"""
        return None if int(self.changed) == 0 else (int(self.x0), int(self.y0), int(self.x1), int(self.y1))

    @property
    def held_delta_e_rms(self):
        """root mean square dE76 of the held pixels against their anchors: sqrt(held_sse / (4096 held))"""
        n = int(self.held)
        return float(np.sqrt(int(self.held_sse) / (4096.0 * n))) if n else 0.0

    def __repr__(self):
        return "FrameHold" + repr(self.as_tuple())


# include/kmeans_hip.h KMG_INDEX_*: the flags of kmg_index_plan (the low two bits are the order)
INDEX_ORDER_KEEP, INDEX_ORDER_USAGE, INDEX_ORDER_LUMA = 0, 1, 2
INDEX_KEEP_UNUSED, INDEX_KEEP_TRANSPARENT, INDEX_TRANSPARENT_FIRST = 4, 8, 16
INDEX_DROPPED = 0xFFFF                  # remap entry of a palette entry the plan drops


class BatchReport(C.Structure):         # include/kmeans_hip.h kmg_batch_report: 16 bytes
    _fields_ = [("launches", C.c_uint32), ("iterations", C.c_uint32), ("sub_batches", C.c_uint32), ("fallback", C.c_uint32)]

    def as_tuple(self):
        return (self.launches, self.iterations, self.sub_batches, self.fallback)

    def __repr__(self):
        return (f"BatchReport(launches={self.launches}, iterations={self.iterations}, sub_batches={self.sub_batches}, "
                f"fallback={self.fallback})")


class BatchQualityReport(C.Structure):  # include/kmeans_hip.h kmg_batch_quality_report: 32 bytes
    _fields_ = [("rounds", C.c_uint32), ("palette_runs", C.c_uint32), ("launches", C.c_uint32), ("measure_launches", C.c_uint32),
                ("batched", C.c_uint32), ("per_image", C.c_uint32), ("sub_batches", C.c_uint32), ("fallback", C.c_uint32)]

    def __repr__(self):
        return ("BatchQualityReport(" + ", ".join(f"{n}={getattr(self, n)}" for n, _ in self._fields_) + ")")


class BatchApplyReport(C.Structure):    # include/kmeans_hip.h kmg_batch_apply_report: 16 bytes
    _fields_ = [("launches", C.c_uint32), ("batched", C.c_uint32), ("per_image", C.c_uint32), ("sub_batches", C.c_uint32)]

    def as_tuple(self):
        return (self.launches, self.batched, self.per_image, self.sub_batches)

    def __repr__(self):
        return (f"BatchApplyReport(launches={self.launches}, batched={self.batched}, per_image={self.per_image}, "
                f"sub_batches={self.sub_batches})")


class ClipReport(C.Structure):          # include/kmeans_hip.h kmg_clip_report: 16 bytes
    _fields_ = [("launches", C.c_uint32), ("batched", C.c_uint32), ("per_image", C.c_uint32), ("sub_clips", C.c_uint32)]

    def as_tuple(self):
        return (self.launches, self.batched, self.per_image, self.sub_clips)

    def __repr__(self):
        return (f"ClipReport(launches={self.launches}, batched={self.batched}, per_image={self.per_image}, "
                f"sub_clips={self.sub_clips})")


class IndexPlanInfo(C.Structure):       # include/kmeans_hip.h kmg_index_plan_info: 16 bytes
    _fields_ = [("n_colors", C.c_uint32), ("n_slots", C.c_uint32), ("transparent", C.c_int32), ("bits", C.c_uint32)]

    def as_tuple(self):
        return (self.n_colors, self.n_slots, self.transparent, self.bits)

    def __repr__(self):
        return f"IndexPlanInfo(n_colors={self.n_colors}, n_slots={self.n_slots}, transparent={self.transparent}, bits={self.bits})"


def index_plan(usage, palette, flags=INDEX_ORDER_USAGE | INDEX_TRANSPARENT_FIRST):
    """kmg_index_plan (host arithmetic, no device): usage = the k + 2 counts of a map, palette (k, 4) uint8.  Returns (remap (k + 1,)
    uint16 with INDEX_DROPPED for dropped entries, palette_out (n_slots, 4) uint8 with (0, 0, 0, 0) at the transparent slot,
    IndexPlanInfo)."""
    pal = np.ascontiguousarray(palette, np.uint8).reshape(-1, 4)
    k = pal.shape[0]
    use = np.ascontiguousarray(usage, np.uint64).reshape(-1)
    if use.shape[0] != k + 2:
        raise ValueError("usage must hold k + 2 counts for a palette of k colours")
    remap = np.empty(k + 1, np.uint16)
    out = np.empty((k + 1, 4), np.uint8)
    info = IndexPlanInfo()
    _check(lib().kmg_index_plan(_np_ptr(use), _np_ptr(pal), k, int(flags), _np_ptr(remap), _np_ptr(out), C.byref(info)))
    return remap, out[:info.n_slots].copy(), info


def packed_stride(width, bits):
    """bytes of one row of `width` indices at `bits` per pixel (rows start on a byte)"""
    return (int(width) * int(bits) + 7) // 8


def pack_indices(index, bits):
    """a (height, width) index map as PNG stores it at bits = 1, 2 or 4: (height, ceil(width * bits / 8)) uint8, the leftmost
    pixel in the high bits, padding bits zero; bits = 8 / 16: the map as uint8 / uint16.  Every index must fit."""
    a = np.asarray(index)
    if a.ndim != 2:
        raise ValueError("index map must be (height, width)")
    if bits not in (1, 2, 4, 8, 16):
        raise ValueError("bits must be 1, 2, 4, 8 or 16")
    if a.size and int(a.max()) >= (1 << bits):
        raise ValueError(f"an index does not fit {bits} bits")
    if bits >= 8:
        return np.ascontiguousarray(a, np.uint8 if bits == 8 else np.uint16)
    h, w = a.shape
    per = 8 // bits
    stride = packed_stride(w, bits)
    wide = np.zeros((h, stride * per), np.uint8)
    wide[:, :w] = a
    out = np.zeros((h, stride), np.uint8)
    for s in range(per):
        out |= wide[:, s::per] << np.uint8(8 - bits * (s + 1))
    return out


def unpack_indices(packed, width, bits):
    """the inverse of pack_indices: packed rows -> (height, width) uint8 (uint16 at bits = 16)"""
    if bits not in (1, 2, 4, 8, 16):
        raise ValueError("bits must be 1, 2, 4, 8 or 16")
    if bits >= 8:
        return np.ascontiguousarray(packed, np.uint8 if bits == 8 else np.uint16).reshape(-1, int(width))
    stride = packed_stride(width, bits)
    a = np.ascontiguousarray(packed, np.uint8).reshape(-1, stride)
    per = 8 // bits
    out = np.empty((a.shape[0], stride * per), np.uint8)
    for s in range(per):
        out[:, s::per] = (a >> np.uint8(8 - bits * (s + 1))) & np.uint8((1 << bits) - 1)
    return np.ascontiguousarray(out[:, :int(width)])


def tolerance_of(delta_e):
    """a dE76 distance as the `tolerance` of the lossy delta calls: rint(4096 dE^2); ValueError when negative or beyond a uint32"""
    de = float(delta_e)
    if not de >= 0.0:
        raise ValueError(f"a tolerance is a distance >= 0, not {delta_e!r}")
    t = int(np.rint(4096.0 * de * de)) if de * de < 2.0 ** 40 else 1 << 52
    if t > 0xFFFFFFFF:
        raise ValueError(f"dE = {delta_e!r} gives a tolerance beyond 32 bits (every pair of colours is within dE {np.sqrt(MAX_TOLERANCE / 4096.0):.1f})")
    return t


# kmg_options.strategy (include/kmeans_hip.h KMG_STRATEGY_*): results are identical either way, only the time differs
STRATEGY_AUTO, STRATEGY_SCAN, STRATEGY_TABLE, STRATEGY_MASK_WORDS = 0, 1, 2, 4
_STRATEGY_NAMES = {"auto": STRATEGY_AUTO, "scan": STRATEGY_SCAN, "brute": STRATEGY_SCAN, "table": STRATEGY_TABLE}
_default_strategy = STRATEGY_AUTO
_live = None            # weak set of the live ImageProcessor / Group objects (set_strategy reaches them)


def _strategy_value(strategy):
    if isinstance(strategy, str):
        v = 0
        for part in strategy.replace("|", "+").split("+"):
            part = part.strip().lower()
            if part == "mask_words":
                v |= STRATEGY_MASK_WORDS
            elif part in _STRATEGY_NAMES:
                v |= _STRATEGY_NAMES[part]
            else:
                raise ValueError(f"unknown strategy {strategy!r}")
        return v
    return int(strategy)


def set_strategy(strategy):
    """kmg_processor_set_strategy on every live processor of this process (ImageProcessor objects and the members of Group
    objects) and the default of the ones created later: "auto" (the library's cost models), "scan" (alias "brute": per-pixel
    scans), "table" (colour table / candidate lists), optionally "+mask_words".  What the tests and tools flip between runs."""
    global _default_strategy
    _default_strategy = _strategy_value(strategy)
    for obj in list(_live or ()):
        obj.set_strategy(_default_strategy)


def _register(obj):
    global _live
    if _live is None:
        import weakref
        _live = weakref.WeakSet()
    _live.add(obj)


MAX_DEVICES = 16                        # KMG_MAX_DEVICES
UNIQUE_ID_BYTES = 128                   # KMG_UNIQUE_ID_BYTES
GROUP_FORCE_COLLECTIVES, GROUP_LOOPBACK = 1, 2                  # kmg_group_options.flags
GROUP_CELLS, GROUP_OVERLAP, GROUP_FUSED_UPDATE = 1, 2, 4        # kmg_group_lloyd_bind flags


class GroupOptions(C.Structure):        # include/kmeans_hip.h kmg_group_options
    _fields_ = [("struct_size", C.c_uint32), ("n_devices", C.c_uint32), ("devices", C.c_int32 * MAX_DEVICES),
                ("flags", C.c_uint32), ("processor", Options)]


def library_path():
    return _LIB_PATH


_lib = None

# every symbol include/kmeans_hip.h declares
SYMBOLS = [
    "kmg_last_error", "kmg_version", "kmg_host_alloc", "kmg_host_free", "kmg_default_options", "kmg_processor_create",
    "kmg_processor_create_ex", "kmg_processor_destroy", "kmg_processor_set_strategy", "kmg_processor_set_alpha_cutoff", "kmg_processor_set_weighting", "kmg_processor_set_diffusion", "kmg_diffusion_weights", "kmg_processor_set_dither", "kmg_processor_set_dither_custom", "kmg_dither_map_values", "kmg_processor_set_fixed_colors", "kmg_palette", "kmg_find", "kmg_reduce",
    "kmg_palette_to_centroids", "kmg_centroids_to_palette", "kmg_octree_palette", "kmg_dev_rgb_to_lab",
    "kmg_resized_dims", "kmg_dev_alpha_compact",
    "kmg_dev_resize", "kmg_lloyd_create", "kmg_lloyd_destroy", "kmg_lloyd_set_centroids",
    "kmg_lloyd_get_centroids", "kmg_lloyd_init_centroids", "kmg_lloyd_init_centroids_seeded", "kmg_lloyd_set_fixed", "kmg_lloyd_set_weighting", "kmg_lloyd_init_step", "kmg_lloyd_init_pick_band",
    "kmg_lloyd_set_centroid_rgba", "kmg_init_first_key", "kmg_lloyd_assign_accumulate",
    "kmg_lloyd_assign_partials", "kmg_lloyd_reduce_partials", "kmg_lloyd_labels", "kmg_lloyd_reserve_cus", "kmg_lloyd_bind_image",
    "kmg_lloyd_unbind_image", "kmg_debug_bound_image", "kmg_lloyd_prepare", "kmg_debug_check_table", "kmg_debug_table_stats", "kmg_debug_check_pairs", "kmg_debug_check_dither_masks", "kmg_debug_check_meld_masks", "kmg_kernel_name",
    "kmg_lloyd_profile", "kmg_lloyd_profile_read",
    "kmg_lloyd_update", "kmg_lloyd_assign_update", "kmg_lloyd_set_cell_share", "kmg_lloyd_labels_from_tables",
    "kmg_lloyd_table_buffers", "kmg_lloyd_accumulate_into", "kmg_lloyd_labels_from_tables_update", "kmg_lloyd_histogram_buffer", "kmg_lloyd_rebuild_from_histogram", "kmg_debug_block_counts", "kmg_debug_idle_blocks", "kmg_debug_encode_table_check", "kmg_debug_division_check", "kmg_lloyd_converged_count", "kmg_lloyd_iterate", "kmg_lloyd_flush", "kmg_lloyd_run", "kmg_dev_apply", "kmg_apply_plan_create", "kmg_apply_plan_run", "kmg_apply_plan_destroy", "kmg_apply_plan_status",
    "kmg_find_indexed", "kmg_reduce_indexed", "kmg_apply_plan_create_format", "kmg_dev_apply_format",
    "kmg_dev_palette_batch", "kmg_palette_batch", "kmg_reduce_batch",
    "kmg_dev_apply_batch", "kmg_find_batch", "kmg_reduce_indexed_batch",
    "kmg_dev_palette_batch_counts", "kmg_dev_apply_batch_counts", "kmg_dev_compare_batch", "kmg_reduce_quality_batch",
    "kmg_dither_threshold", "kmg_dev_compare", "kmg_compare", "kmg_reduce_quality",
    "kmg_sequence_create", "kmg_sequence_destroy", "kmg_sequence_add", "kmg_sequence_add_device", "kmg_sequence_clear",
    "kmg_sequence_info", "kmg_sequence_centroids", "kmg_sequence_palette", "kmg_dev_frame_delta", "kmg_dev_frame_delta_lossy",
    "kmg_sequence_output_begin", "kmg_sequence_output_frame", "kmg_sequence_output_frame_lossy", "kmg_sequence_output_end",
    "kmg_dev_frame_delta_clip", "kmg_sequence_output_frames",
    "kmg_dev_frame_delta_colour", "kmg_dev_frame_delta_colour_lossy", "kmg_sequence_output_begin_local", "kmg_sequence_output_frame_local",
    "kmg_dev_index_usage", "kmg_index_plan", "kmg_dev_index_remap", "kmg_index_usage", "kmg_index_remap", "kmg_index_optimize",
    "kmg_default_group_options", "kmg_group_create", "kmg_group_unique_id", "kmg_group_create_rank", "kmg_group_destroy",
    "kmg_group_info", "kmg_group_processor", "kmg_group_stream", "kmg_group_palette", "kmg_group_find", "kmg_group_reduce",
    "kmg_group_reduce_batch", "kmg_group_lloyd_create", "kmg_group_lloyd_destroy", "kmg_group_lloyd_bind",
    "kmg_group_lloyd_set_centroids", "kmg_group_lloyd_get_centroids", "kmg_group_lloyd_init", "kmg_group_lloyd_prime",
    "kmg_group_lloyd_step", "kmg_group_lloyd_sync", "kmg_group_lloyd_run", "kmg_group_lloyd_member", "kmg_group_lloyd_create_batch", "kmg_group_lloyd_bind_batch", "kmg_group_lloyd_set_centroids_image",
    "kmg_group_lloyd_get_centroids_image", "kmg_group_lloyd_run_batch",
]


def lib():
    """Load libkmeans_hip.so (built in-tree by `make -C kmeans-gpu_amd`).  Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise ImportError(f"{_LIB_PATH} not found: build it with `make -C {_PKG_ROOT}` "
                          "(or `python -c 'import __graft_entry__ as g; g.build()'`). "
                          "There is no fallback implementation.")
    # When PyTorch shares the process (tests, bench.py, the sharded driver) it must be imported
    # BEFORE libkmeans_hip.so is loaded: torch bundles its own libamdhip64, and two different HIP
    # runtimes in one process cannot both own the GPU ("no ROCm-capable device is detected").
    # With torch's runtime already mapped, our DT_NEEDED libamdhip64 resolves to that same copy.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(_LIB_PATH)
    vp, u8p, u32p, f32p, i64p = C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p
    L.kmg_last_error.restype = C.c_char_p
    L.kmg_version.restype = C.c_char_p
    L.kmg_host_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
    L.kmg_host_free.argtypes = [vp]
    L.kmg_host_free.restype = None
    L.kmg_default_options.argtypes = [C.POINTER(Options)]
    L.kmg_default_options.restype = None
    L.kmg_processor_create.argtypes = [C.POINTER(vp)]
    L.kmg_processor_create_ex.argtypes = [C.POINTER(Options), C.POINTER(vp)]
    L.kmg_processor_destroy.argtypes = [vp]
    L.kmg_processor_destroy.restype = None
    L.kmg_palette.argtypes = [vp, u8p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, u8p, C.POINTER(C.c_uint32)]
    L.kmg_find.argtypes = [vp, u8p, C.c_uint32, C.c_uint32, u8p, C.c_uint32, C.c_int, u8p]
    L.kmg_reduce.argtypes = [vp, u8p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, u8p]
    L.kmg_palette_to_centroids.argtypes = [u8p, C.c_uint32, f32p]
    L.kmg_centroids_to_palette.argtypes = [f32p, C.c_uint32, u8p]
    L.kmg_octree_palette.argtypes = [u8p, C.c_uint64, C.c_uint32, u8p, C.POINTER(C.c_uint32)]
    L.kmg_dev_rgb_to_lab.argtypes = [vp, u8p, C.c_uint64, f32p, vp]
    L.kmg_resized_dims.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.kmg_resized_dims.restype = None
    L.kmg_dev_resize.argtypes = [vp, u8p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u8p, vp]
    L.kmg_lloyd_create.argtypes = [vp, C.c_uint32, C.POINTER(vp)]
    L.kmg_lloyd_destroy.argtypes = [vp]
    L.kmg_lloyd_destroy.restype = None
    L.kmg_lloyd_set_centroids.argtypes = [vp, f32p, vp]
    L.kmg_lloyd_get_centroids.argtypes = [vp, f32p, vp]
    L.kmg_lloyd_init_centroids.argtypes = [vp, u8p, C.c_uint32, C.c_uint32, vp]
    L.kmg_lloyd_init_step.argtypes = [vp, u8p, C.c_uint64, C.c_uint64, C.c_uint32, vp, vp]
    L.kmg_lloyd_init_pick_band.argtypes = [vp, u8p, C.c_uint64, C.c_uint64, vp, vp, vp]
    L.kmg_lloyd_set_centroid_rgba.argtypes = [vp, C.c_uint32, vp, vp]
    L.kmg_init_first_key.argtypes = [C.c_uint32, C.c_uint32]
    L.kmg_init_first_key.restype = C.c_uint64
    L.kmg_lloyd_assign_accumulate.argtypes = [vp, u8p, C.c_uint64, u32p, i64p, vp]
    L.kmg_lloyd_assign_partials.argtypes = [vp, u8p, C.c_uint64, u32p, vp]
    L.kmg_lloyd_reduce_partials.argtypes = [vp, C.c_uint64, i64p, vp]
    L.kmg_lloyd_labels.argtypes = [vp, u8p, C.c_uint64, u32p, vp]
    L.kmg_lloyd_reserve_cus.argtypes = [vp, C.c_uint32]
    L.kmg_lloyd_bind_image.argtypes = [vp, u8p, C.c_uint64, vp]
    L.kmg_debug_table_stats.argtypes = [vp, C.POINTER(C.c_uint64), vp]
    L.kmg_debug_check_pairs.argtypes = [vp, C.POINTER(C.c_uint64), vp]
    L.kmg_debug_bound_image.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.kmg_debug_check_dither_masks.argtypes = [vp, f32p, C.c_uint32, C.POINTER(C.c_uint64), vp]
    L.kmg_debug_check_meld_masks.argtypes = [vp, f32p, C.c_uint32, C.POINTER(C.c_uint64), vp]
    L.kmg_kernel_name.argtypes = [C.c_int]
    L.kmg_kernel_name.restype = C.c_char_p
    L.kmg_lloyd_profile.argtypes = [vp, C.c_int]
    L.kmg_lloyd_profile_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
    L.kmg_lloyd_unbind_image.argtypes = [vp]
    L.kmg_lloyd_prepare.argtypes = [vp, u8p, C.c_uint64, C.c_int, C.POINTER(C.c_int), vp]
    L.kmg_debug_check_table.argtypes = [vp, C.POINTER(C.c_uint64), vp]
    L.kmg_lloyd_update.argtypes = [vp, i64p, vp]
    L.kmg_lloyd_assign_update.argtypes = [vp, u8p, C.c_uint64, u32p, i64p, C.c_int, vp]
    L.kmg_lloyd_set_cell_share.argtypes = [vp, C.c_uint32, C.c_uint32, vp]
    L.kmg_lloyd_labels_from_tables.argtypes = [vp, u8p, C.c_uint64, u32p, vp]
    L.kmg_debug_block_counts.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.kmg_debug_idle_blocks.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.kmg_debug_encode_table_check.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.kmg_debug_division_check.argtypes = [vp, C.c_float, C.POINTER(C.c_uint64)]
    L.kmg_lloyd_histogram_buffer.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.kmg_lloyd_rebuild_from_histogram.argtypes = [vp, C.c_uint64, vp]
    L.kmg_lloyd_table_buffers.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.kmg_lloyd_converged_count.argtypes = [vp, C.POINTER(C.c_uint32), vp]
    L.kmg_lloyd_accumulate_into.argtypes = [vp, u8p, C.c_uint64, i64p, vp]
    L.kmg_lloyd_labels_from_tables_update.argtypes = [vp, u8p, C.c_uint64, u32p, i64p, vp]
    L.kmg_lloyd_iterate.argtypes = [vp, u8p, C.c_uint64, u32p, i64p, C.c_int, vp]
    L.kmg_lloyd_flush.argtypes = [vp, vp]
    L.kmg_lloyd_run.argtypes = [vp, u8p, C.c_uint64, u32p, C.POINTER(C.c_uint32), vp]
    L.kmg_dev_apply.argtypes = [vp, u8p, C.c_uint32, C.c_uint32, C.c_uint32, f32p, C.c_uint32, C.c_int, u8p, vp]
    L.kmg_apply_plan_create.argtypes = [vp, f32p, C.c_uint32, C.c_int, C.c_uint64, vp, C.POINTER(vp)]
    L.kmg_apply_plan_run.argtypes = [vp, u8p, C.c_uint32, C.c_uint32, C.c_uint32, u8p, vp]
    L.kmg_find_indexed.argtypes = [vp, u8p, C.c_uint32, C.c_uint32, u8p, C.c_uint32, C.c_int, C.c_int, vp]
    L.kmg_reduce_indexed.argtypes = [vp, u8p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, u8p, C.POINTER(C.c_uint32), vp]
    L.kmg_apply_plan_create_format.argtypes = [vp, f32p, C.c_uint32, C.c_int, C.c_int, C.c_uint64, vp, C.POINTER(vp)]
    L.kmg_dev_apply_format.argtypes = [vp, u8p, C.c_uint32, C.c_uint32, C.c_uint32, f32p, C.c_uint32, C.c_int, C.c_int, vp, vp]
    L.kmg_apply_plan_destroy.argtypes = [vp, C.c_int]
    L.kmg_apply_plan_destroy.restype = None
    L.kmg_apply_plan_status.argtypes = [vp]
    L.kmg_dither_threshold.argtypes = [f32p, C.c_uint32, C.POINTER(C.c_float)]
    L.kmg_processor_set_strategy.argtypes = [vp, C.c_int]
    L.kmg_processor_set_alpha_cutoff.argtypes = [vp, C.c_uint32]
    L.kmg_processor_set_fixed_colors.argtypes = [vp, u8p, C.c_uint32]
    L.kmg_lloyd_init_centroids_seeded.argtypes = [vp, u8p, C.c_uint32, C.c_uint32, f32p, C.c_uint32, vp]
    L.kmg_lloyd_set_fixed.argtypes = [vp, C.c_uint32]
    L.kmg_processor_set_weighting.argtypes = [vp, C.c_int]
    if hasattr(L, "kmg_processor_set_diffusion"):        # (KMG_LIBRARY may name an older build: tools/diffusion_filters_time.py times one)
        L.kmg_processor_set_diffusion.argtypes = [vp, C.c_int]
        L.kmg_diffusion_weights.argtypes = [C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    if hasattr(L, "kmg_processor_set_dither"):           # (likewise: tools/dither_map_time.py times the build before the maps)
        L.kmg_processor_set_dither.argtypes = [vp, C.c_int, C.c_float]
        L.kmg_processor_set_dither_custom.argtypes = [vp, C.POINTER(C.c_uint16), C.c_uint32, C.c_uint32, C.c_uint32, C.c_float]
        L.kmg_dither_map_values.argtypes = [C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint16)]
    L.kmg_lloyd_set_weighting.argtypes = [vp, C.c_int]
    L.kmg_dev_alpha_compact.argtypes = [vp, u8p, C.c_uint64, C.c_uint32, u8p, vp, vp]
    L.kmg_dev_compare.argtypes = [vp, u8p, vp, C.c_uint64, C.c_int, u8p, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp]
    L.kmg_compare.argtypes = [vp, u8p, vp, C.c_uint32, C.c_uint32, C.c_int, u8p, C.c_uint32, C.c_uint32, C.POINTER(ErrorStats)]
    L.kmg_reduce_quality.argtypes = [vp, u8p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, u8p,
                                     C.POINTER(C.c_uint32), vp, C.POINTER(ErrorStats), C.POINTER(C.c_int)]
    L.kmg_sequence_create.argtypes = [vp, C.POINTER(vp)]
    L.kmg_sequence_destroy.argtypes = [vp]
    L.kmg_sequence_destroy.restype = None
    L.kmg_sequence_add.argtypes = [vp, u8p, C.c_uint32, C.c_uint32]
    L.kmg_sequence_add_device.argtypes = [vp, u8p, C.c_uint32, C.c_uint32, vp]
    L.kmg_sequence_clear.argtypes = [vp]
    L.kmg_sequence_info.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.kmg_sequence_centroids.argtypes = [vp, C.c_uint32, f32p]
    L.kmg_sequence_palette.argtypes = [vp, C.c_uint32, u8p, C.POINTER(C.c_uint32)]
    L.kmg_dev_frame_delta.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, vp, vp, vp]
    L.kmg_sequence_output_begin.argtypes = [vp, C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_uint32, u8p, C.POINTER(C.c_uint32)]
    L.kmg_sequence_output_frame.argtypes = [vp, u8p, C.c_uint32, vp, C.POINTER(FrameDelta), C.POINTER(C.c_int)]
    L.kmg_dev_frame_delta_lossy.argtypes = [vp, u8p, vp, vp, u8p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, vp, vp, vp]
    L.kmg_sequence_output_frame_lossy.argtypes = [vp, u8p, C.c_uint32, C.c_uint32, vp, C.POINTER(FrameHold), C.POINTER(C.c_int)]
    L.kmg_sequence_output_end.argtypes = [vp]
    L.kmg_dev_frame_delta_clip.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.POINTER(vp), vp, vp, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32,
                                           C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(vp), vp, vp, vp]
    L.kmg_sequence_output_frames.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.c_uint32, C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(vp),
                                             C.POINTER(FrameHold), C.POINTER(C.c_int), C.POINTER(ClipReport)]
    L.kmg_dev_frame_delta_colour.argtypes = [vp, vp, u8p, u8p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, vp, vp, vp]
    L.kmg_dev_frame_delta_colour_lossy.argtypes = [vp, u8p, vp, u8p, u8p, u8p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32,
                                                   vp, vp, vp]
    L.kmg_sequence_output_begin_local.argtypes = [vp, C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32]
    L.kmg_sequence_output_frame_local.argtypes = [vp, u8p, C.c_uint32, C.POINTER(C.c_uint32), vp, u8p, C.POINTER(C.c_uint32), C.POINTER(FrameHold),
                                                  C.POINTER(C.c_int)]
    L.kmg_dev_index_usage.argtypes = [vp, vp, C.c_uint64, C.c_int, C.c_uint32, vp, vp]
    L.kmg_index_plan.argtypes = [vp, u8p, C.c_uint32, C.c_uint32, vp, u8p, C.POINTER(IndexPlanInfo)]
    L.kmg_dev_index_remap.argtypes = [vp, vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, vp, vp]
    L.kmg_index_usage.argtypes = [vp, vp, C.c_int, C.c_uint64, C.c_uint32, vp]
    L.kmg_index_remap.argtypes = [vp, vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, C.POINTER(C.c_uint64)]
    L.kmg_index_optimize.argtypes = [vp, vp, C.c_int, C.c_uint32, C.c_uint32, u8p, C.c_uint32, C.c_uint32, C.c_uint32, u8p,
                                     C.POINTER(IndexPlanInfo), vp]
    L.kmg_default_group_options.argtypes = [C.POINTER(GroupOptions)]
    L.kmg_default_group_options.restype = None
    L.kmg_group_create.argtypes = [C.POINTER(GroupOptions), C.POINTER(vp)]
    L.kmg_group_unique_id.argtypes = [vp]
    L.kmg_group_create_rank.argtypes = [C.POINTER(GroupOptions), vp, C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.kmg_group_destroy.argtypes = [vp]
    L.kmg_group_destroy.restype = None
    L.kmg_group_info.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
    L.kmg_group_processor.argtypes = [vp, C.c_uint32]
    L.kmg_group_processor.restype = vp
    L.kmg_group_stream.argtypes = [vp, C.c_uint32]
    L.kmg_group_stream.restype = vp
    L.kmg_group_palette.argtypes = [vp, u8p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, u8p, C.POINTER(C.c_uint32)]
    L.kmg_group_find.argtypes = [vp, u8p, C.c_uint32, C.c_uint32, u8p, C.c_uint32, C.c_int, u8p]
    L.kmg_group_reduce.argtypes = [vp, u8p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, u8p]
    L.kmg_group_reduce_batch.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32,
                                         C.c_int, C.c_int, C.POINTER(vp)]
    L.kmg_dev_palette_batch.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32, f32p,
                                        u32p, C.POINTER(BatchReport), vp]
    L.kmg_palette_batch.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32, C.c_int,
                                    C.c_uint64, C.POINTER(vp), u32p, C.POINTER(BatchReport)]
    L.kmg_reduce_batch.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32, C.c_int,
                                   C.c_int, C.c_uint64, C.POINTER(vp), C.POINTER(BatchReport)]
    L.kmg_dev_apply_batch.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), f32p, C.c_uint32,
                                      C.c_uint32, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(BatchApplyReport), vp]
    L.kmg_find_batch.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), u8p, C.c_uint32, C.c_int,
                                 C.c_int, C.c_uint64, C.POINTER(vp), C.POINTER(BatchApplyReport)]
    L.kmg_reduce_indexed_batch.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32, C.c_int,
                                           C.c_int, C.c_int, C.c_uint64, C.POINTER(vp), u32p, C.POINTER(vp), C.POINTER(BatchReport),
                                           C.POINTER(BatchApplyReport)]
    L.kmg_group_lloyd_create.argtypes = [vp, C.c_uint32, C.POINTER(vp)]
    L.kmg_group_lloyd_destroy.argtypes = [vp]
    L.kmg_group_lloyd_destroy.restype = None
    L.kmg_group_lloyd_bind.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32,
                                       C.POINTER(vp), C.c_uint32]
    L.kmg_group_lloyd_set_centroids.argtypes = [vp, f32p]
    L.kmg_group_lloyd_get_centroids.argtypes = [vp, f32p]
    for name in ("init", "prime", "step", "sync"):
        getattr(L, "kmg_group_lloyd_" + name).argtypes = [vp]
    L.kmg_group_lloyd_run.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.kmg_group_lloyd_member.argtypes = [vp, C.c_uint32, C.POINTER(C.c_int)]
    L.kmg_group_lloyd_member.restype = vp
    L.kmg_dev_palette_batch_counts.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), u32p, f32p, u32p,
                                               C.POINTER(BatchReport), vp]
    L.kmg_dev_apply_batch_counts.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), f32p, u32p, C.c_int,
                                             C.c_int, C.POINTER(vp), C.POINTER(BatchApplyReport), vp]
    L.kmg_dev_compare_batch.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_uint64), C.c_int, u8p, u32p, C.c_uint32,
                                        C.c_uint32, vp, vp]
    L.kmg_reduce_quality_batch.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32,
                                           C.c_uint32, C.c_int, C.c_int, C.c_uint64, C.POINTER(vp), u32p, C.POINTER(vp), C.POINTER(ErrorStats),
                                           C.POINTER(C.c_int), C.POINTER(BatchQualityReport)]
    L.kmg_group_lloyd_create_batch.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.kmg_group_lloyd_bind_batch.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                             C.POINTER(C.c_uint32), C.POINTER(vp), C.c_uint32]
    L.kmg_group_lloyd_set_centroids_image.argtypes = [vp, C.c_uint32, f32p]
    L.kmg_group_lloyd_get_centroids_image.argtypes = [vp, C.c_uint32, f32p]
    L.kmg_group_lloyd_run_batch.argtypes = [vp, C.POINTER(C.c_uint32)]
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise KmgError(rc, lib().kmg_last_error().decode("utf-8", "replace"))


def _np_ptr(a):
    return C.c_void_p(a.ctypes.data)


def default_options():
    o = Options()
    lib().kmg_default_options(C.byref(o))
    return o


def resized_dims(width, height, max_size=256):
    """InputTexture::resized dimension rule (core/src/structures.rs:79-89)."""
    nw, nh = C.c_uint32(), C.c_uint32()
    lib().kmg_resized_dims(width, height, max_size, C.byref(nw), C.byref(nh))
    return nw.value, nh.value


def palette_to_centroids(colors):
    """CentroidsBuffer::fixed_centroids (core/src/structures.rs:523-553): RGBA8 -> (L,a,b,1)."""
    pal = np.ascontiguousarray(colors, np.uint8).reshape(-1, 4)
    out = np.empty((pal.shape[0], 4), np.float32)
    _check(lib().kmg_palette_to_centroids(_np_ptr(pal), pal.shape[0], _np_ptr(out)))
    return out


def centroids_to_palette(centroids4):
    """CentroidsBuffer::pull_values (core/src/structures.rs:581-617)."""
    c = np.ascontiguousarray(centroids4, np.float32).reshape(-1, 4)
    out = np.empty((c.shape[0], 4), np.uint8)
    _check(lib().kmg_centroids_to_palette(_np_ptr(c), c.shape[0], _np_ptr(out)))
    return out


def octree_palette(pixels, color_count):
    """ColorTree::{add_color, reduce} (core/src/octree.rs): the reference's CPU octree quantiser."""
    px = np.ascontiguousarray(pixels, np.uint8).reshape(-1, 4)
    out = np.empty((max(min(int(color_count), px.shape[0]), 1), 4), np.uint8)
    cnt = C.c_uint32()
    _check(lib().kmg_octree_palette(_np_ptr(px), px.shape[0], int(color_count), _np_ptr(out), C.byref(cnt)))
    return out[:cnt.value].copy()


def dither_threshold(centroids4):
    c = np.ascontiguousarray(centroids4, np.float32).reshape(-1, 4)
    t = C.c_float()
    _check(lib().kmg_dither_threshold(_np_ptr(c), c.shape[0], C.byref(t)))
    return t.value


WEIGHT_NONE, WEIGHT_ALPHA = 0, 1        # include/kmeans_hip.h KMG_WEIGHT_*


def with_weights(image, weights):
    """A copy of `image` ((height, width, 4) uint8) whose alpha byte is `weights`, a (height, width) uint8 map: the importance-map
    route of alpha weighting for opaque images -- ImageProcessor(alpha_weight=True) at alpha_cutoff = 0 then weighs every pixel by
    its entry (0: the pixel does not shape the palette at all) and still writes alpha 255."""
    img = _image(image)
    w = np.asarray(weights)
    if w.dtype != np.uint8:
        raise ValueError("weights must be a uint8 map")
    if w.shape != img.shape[:2]:
        raise ValueError(f"weights of shape {w.shape} do not match the image's {img.shape[:2]}")
    out = img.copy()
    out[:, :, 3] = w
    return out


def _image(image):
    a = np.ascontiguousarray(image, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError("image must be a (height, width, 4) uint8 RGBA array")
    return a


class _PinnedPool:
    """Result arrays of large images in page-locked host memory (kmg_host_alloc): a fresh pageable array of 256 MiB costs the
    call tens of milliseconds of page faults, a pinned block is copied to by DMA.  A block returns to the pool when the array
    that wraps it is garbage collected and serves the next result of the same size; at most `limit` bytes are kept."""

    def __init__(self, limit=1 << 30, threshold=16 << 20):
        self.free, self.kept, self.limit, self.threshold = {}, 0, limit, threshold

    def _give_back(self, ptr, nbytes):
        if self.kept + nbytes <= self.limit:
            self.free.setdefault(nbytes, []).append(ptr)
            self.kept += nbytes
        else:
            lib().kmg_host_free(C.c_void_p(ptr))

    def array(self, shape):
        import weakref
        nbytes = int(np.prod(shape))
        if nbytes < self.threshold or os.environ.get("KMG_PINNED_RESULTS", "1") == "0":
            return None
        blocks = self.free.get(nbytes)
        if blocks:
            ptr = blocks.pop()
            self.kept -= nbytes
        else:
            p = C.c_void_p()
            if lib().kmg_host_alloc(nbytes, C.byref(p)) != 0 or not p.value:
                return None
            ptr = p.value
        buf = (C.c_uint8 * nbytes).from_address(ptr)
        weakref.finalize(buf, self._give_back, ptr, nbytes)      # (the numpy array keeps `buf` alive as its base)
        return np.frombuffer(buf, dtype=np.uint8).reshape(shape)


_pinned = _PinnedPool()


def _result(img, out):
    if out is None:
        pinned = _pinned.array(img.shape)
        return pinned if pinned is not None else np.empty_like(img)
    if out.dtype != np.uint8 or out.shape != img.shape or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous uint8 array of the image's shape")
    return out


class ImageProcessor:
    """Mirror of `kmeans_color_gpu::ImageProcessor` (core/src/lib.rs:24-165)."""

    def __init__(self, device=-1, shrink_max_dim=256, max_iterations=128, check_period=8,
                 convergence=1.0, strategy=None, alpha_cutoff=0, fixed_colors=None, alpha_weight=False, diffusion=0,
                 dither_map=0, dither_strength=1.0):
        """alpha_cutoff: 0 = alpha ignored (the reference's behaviour); 1..255 = alpha mode (include/kmeans_hip.h at
        kmg_options): only pixels whose alpha is >= alpha_cutoff shape the palette, and the outputs keep the input's alpha.
        fixed_colors: colours every k-means palette of this processor keeps, as its first entries (set_fixed_colors)
        alpha_weight: the k-means palettes weigh every pixel by its alpha byte (set_alpha_weight)
        diffusion: the filter of ReduceMode.Diffuse (set_diffusion)
        dither_map, dither_strength: the threshold map and strength of ReduceMode.Dither (set_dither)"""
        self._h = C.c_void_p()
        o = default_options()
        o.device = device
        o.shrink_max_dim = shrink_max_dim
        o.max_iterations = max_iterations
        o.check_period = check_period
        o.convergence = convergence
        o.strategy = _default_strategy if strategy is None else _strategy_value(strategy)
        o.alpha_cutoff = int(alpha_cutoff)
        _check(lib().kmg_processor_create_ex(C.byref(o), C.byref(self._h)))
        self.options = o
        self._sequences = None          # weak set of the live Sequence objects: closed with the processor, which they need
        _register(self)
        self.alpha_weight = False
        self.last_batch_report = None   # BatchReport of the last palette_batch / reduce_batch / palette_batch_device / reduce_indexed_batch
        self.last_quality_report = None   # BatchQualityReport of the last reduce_quality_batch
        self.last_batch_apply_report = None   # BatchApplyReport of the last find_batch / reduce_indexed_batch / apply_batch_device
        if fixed_colors is not None:
            self.set_fixed_colors(fixed_colors)
        if alpha_weight:
            self.set_alpha_weight(True)
        self.diffusion = Diffusion.FloydSteinberg
        if _diffusion_value(diffusion):
            self.set_diffusion(diffusion)

        self.dither_map, self.dither_strength = DitherMap.Bayer4, 1.0
        if not (isinstance(dither_map, (int, DitherMap)) and int(dither_map) == 0 and float(dither_strength) == 1.0):
            self.set_dither(dither_map, dither_strength)

    def set_dither(self, map, strength=1.0, levels=None):
        """kmg_processor_set_dither[_custom]: the threshold map and the strength (0 .. 4) of the ReduceMode.Dither outputs made from
        now on; an apply plan and an open sequence output keep the ones they were made under.  map: a DitherMap, its number, its
        CLI name, or a 2-D integer array (height, width) of levels for a custom map, whose sides are powers of two up to 64;
        levels: the n_levels of a custom map (default: its largest level + 1).  DitherMap.Bayer4 at strength 1 is the default, the
        reference's dither"""
        if isinstance(map, (str, int, enum.IntEnum, np.integer)):
            v = _dither_map_value(map)
            _check(lib().kmg_processor_set_dither(self._h, v, float(strength)))
            self.dither_map = DitherMap(v)
        else:
            a = np.asarray(map)
            if a.ndim != 2 or a.size == 0 or not np.issubdtype(a.dtype, np.integer):
                raise ValueError("a custom dither map is a 2-D integer array (height, width)")
            if a.min() < 0 or a.max() > 65535:
                raise ValueError("the levels of a dither map are 0 .. 65535")
            n_levels = int(a.max()) + 1 if levels is None else int(levels)
            if not 0 <= n_levels <= 0xFFFFFFFF:
                raise ValueError("levels does not fit the call")
            a16 = np.ascontiguousarray(a, np.uint16)
            _check(lib().kmg_processor_set_dither_custom(self._h, a16.ctypes.data_as(C.POINTER(C.c_uint16)), a.shape[1], a.shape[0], n_levels,
                                                         float(strength)))
            self.dither_map = DitherMap.Custom
        self.dither_strength = float(strength)

    def set_diffusion(self, filter):
        """kmg_processor_set_diffusion: the filter (a Diffusion, its number or its CLI name) of the ReduceMode.Diffuse outputs made
        from now on; an apply plan and an open sequence output keep the one they were made under"""
        v = _diffusion_value(filter)
        _check(lib().kmg_processor_set_diffusion(self._h, v))
        self.diffusion = Diffusion(v)

    def set_alpha_weight(self, on):
        """kmg_processor_set_weighting: True = the k-means palette steps of the calls that start from now on weigh every pixel by
        its alpha byte and keep the pixels with alpha >= max(alpha_cutoff, 1) (include/kmeans_hip.h; with_weights makes an
        importance map of an opaque image); False = every kept pixel weighs 1, the default"""
        _check(lib().kmg_processor_set_weighting(self._h, WEIGHT_ALPHA if on else WEIGHT_NONE))
        self.alpha_weight = bool(on)

    def set_fixed_colors(self, colors):
        """kmg_processor_set_fixed_colors: (n, 3) or (n, 4) uint8 colours (alpha ignored) that the k-means palettes of the
        calls that start from now on keep exactly, as entries 0 .. n - 1 in index order; None or an empty list clears them"""
        pal = np.zeros((0, 4), np.uint8)
        if colors is not None and len(colors):
            c = np.asarray(colors, dtype=np.uint8)
            if c.ndim != 2 or c.shape[1] not in (3, 4):
                raise ValueError("fixed colours: an (n, 3) or (n, 4) uint8 array")
            pal = np.full((c.shape[0], 4), 255, np.uint8)
            pal[:, :c.shape[1]] = c
        _check(lib().kmg_processor_set_fixed_colors(self._h, _np_ptr(pal) if pal.shape[0] else None, pal.shape[0]))

    def set_alpha_cutoff(self, alpha_cutoff):
        """kmg_processor_set_alpha_cutoff: 0 (alpha ignored) or 1..255 (alpha mode) for the calls that start from now on"""
        _check(lib().kmg_processor_set_alpha_cutoff(self._h, int(alpha_cutoff)))
        self.options.alpha_cutoff = int(alpha_cutoff)

    def set_strategy(self, strategy):
        """kmg_processor_set_strategy: "auto" | "scan" | "table" [+ "mask_words"] (or the KMG_STRATEGY_* bits)"""
        if self._h.value:
            _check(lib().kmg_processor_set_strategy(self._h, _strategy_value(strategy)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            for seq in list(getattr(self, "_sequences", None) or ()):
                seq.close()
            lib().kmg_processor_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        return self._h

    # lib.rs:67-77
    def palette(self, color_count, image, algo=Algorithm.Kmeans):
        img = _image(image)
        h, w = img.shape[:2]
        out = np.empty((max(int(color_count), 1), 4), np.uint8)     # octree returns <= color_count colours
        cnt = C.c_uint32()
        _check(lib().kmg_palette(self._h, _np_ptr(img), w, h, int(color_count), int(algo), _np_ptr(out), C.byref(cnt)))
        return out[:cnt.value].copy()

    # lib.rs:79-114
    def find(self, image, colors, reduce_mode=ReduceMode.Replace, out=None):
        """out: optional (height, width, 4) uint8 array that receives the result (the C ABI writes into the caller's buffer;
        the reference returns a fresh Vec, which is what out=None does)"""
        img = _image(image)
        h, w = img.shape[:2]
        pal = np.ascontiguousarray(colors, np.uint8).reshape(-1, 4)
        out = _result(img, out)
        _check(lib().kmg_find(self._h, _np_ptr(img), w, h, _np_ptr(pal), pal.shape[0], int(reduce_mode), _np_ptr(out)))
        return out

    # lib.rs:116-164
    def reduce(self, color_count, image, algo=Algorithm.Kmeans, reduce_mode=ReduceMode.Replace, out=None):
        img = _image(image)
        h, w = img.shape[:2]
        out = _result(img, out)
        _check(lib().kmg_reduce(self._h, _np_ptr(img), w, h, int(color_count), int(algo), int(reduce_mode), _np_ptr(out)))
        return out

    # ---- batches: many small images per launch (include/kmeans_hip.h kmg_batch_report) --------
    @staticmethod
    def _batch_arrays(imgs):
        n = len(imgs)
        return ((C.c_void_p * n)(*[im.ctypes.data for im in imgs]), (C.c_uint32 * n)(*[im.shape[1] for im in imgs]),
                (C.c_uint32 * n)(*[im.shape[0] for im in imgs]))

    def palette_batch(self, color_count, images, algo=Algorithm.Kmeans, max_resident_bytes=0):
        """kmg_palette_batch: the palettes of many images, one launch chain for all of them; returns the list of palettes, each
        what palette() returns for that image.  The report of the call: last_batch_report"""
        imgs = [_image(im) for im in images]
        n = len(imgs)
        outs = [np.empty((max(int(color_count), 1), 4), np.uint8) for _ in imgs]
        src, ws, hs = self._batch_arrays(imgs)
        dst = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        counts = np.zeros(max(n, 1), np.uint32)
        rep = BatchReport()
        _check(lib().kmg_palette_batch(self._h, n, src, ws, hs, int(color_count), int(algo), int(max_resident_bytes), dst, _np_ptr(counts),
                                       C.byref(rep)))
        self.last_batch_report = rep
        return [o[:int(c)].copy() for o, c in zip(outs, counts)]

    def reduce_batch(self, color_count, images, algo=Algorithm.Kmeans, reduce_mode=ReduceMode.Replace, max_resident_bytes=0, out=None):
        """kmg_reduce_batch: reduce() of many images with one launch chain for their palettes; returns the list of results (it
        mirrors Group.reduce_batch).  out: optional list of arrays that receive the results, as reduce(out=) takes one.  The
        report of the call: last_batch_report"""
        imgs = [_image(im) for im in images]
        n = len(imgs)
        if out is not None and len(out) != n:
            raise ValueError("out must hold one array per image")
        outs = [_result(im, None if out is None else out[i]) for i, im in enumerate(imgs)]
        src, ws, hs = self._batch_arrays(imgs)
        dst = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        rep = BatchReport()
        _check(lib().kmg_reduce_batch(self._h, n, src, ws, hs, int(color_count), int(algo), int(reduce_mode), int(max_resident_bytes), dst,
                                      C.byref(rep)))
        self.last_batch_report = rep
        return outs

    def palette_batch_device(self, d_images, widths, heights, k, stream=0):
        """kmg_dev_palette_batch: working images in device memory (d_images: their addresses) -> (centroids (n, k, 4) float32 in
        index order, iterations (n,) uint32).  The report of the call: last_batch_report"""
        n = len(d_images)
        src = (C.c_void_p * n)(*[int(d) for d in d_images])
        ws = (C.c_uint32 * n)(*[int(w) for w in widths])
        hs = (C.c_uint32 * n)(*[int(h) for h in heights])
        cent = np.empty((n, int(k), 4), np.float32)
        its = np.zeros(max(n, 1), np.uint32)
        rep = BatchReport()
        _check(lib().kmg_dev_palette_batch(self._h, n, src, ws, hs, int(k), _np_ptr(cent), _np_ptr(its), C.byref(rep), C.c_void_p(stream)))
        self.last_batch_report = rep
        return cent, its[:n]

    # ---- batched output (include/kmeans_hip.h kmg_batch_apply_report) ---------------------------
    def _batch_format(self, k, format):
        """the output format of a batch and the dtype of its arrays: `format`, or what find_indexed / reduce_indexed choose for k"""
        fmt = self._index_format(k) if format is None else OutputFormat(format)
        return fmt, {OutputFormat.RGBA8: np.uint8, OutputFormat.Index8: np.uint8, OutputFormat.Index16: np.uint16}[fmt]

    @staticmethod
    def _batch_outputs(imgs, fmt, dtype, out):
        """the result arrays of a batch: new ones, or the caller's `out` (one C-contiguous array of the right shape per image)"""
        shapes = [im.shape if fmt == OutputFormat.RGBA8 else im.shape[:2] for im in imgs]
        if out is None:
            return [np.empty(s, dtype) for s in shapes]
        if len(out) != len(imgs) or any(o.shape != s or o.dtype != dtype or not o.flags.c_contiguous for o, s in zip(out, shapes)):
            raise ValueError("out must hold one C-contiguous array of the output's shape and type per image")
        return list(out)

    def find_batch(self, images, colors, reduce_mode=ReduceMode.Replace, format=None, max_resident_bytes=0, out=None):
        """kmg_find_batch: find_indexed() of many images onto ONE palette, their output passes in one launch; returns the list of
        index maps, each what find_indexed returns for that image (format=OutputFormat.RGBA8: what find returns).  The report of
        the call: last_batch_apply_report.  out: optional list of arrays that receive the results"""
        imgs = [_image(im) for im in images]
        n = len(imgs)
        pal = np.ascontiguousarray(colors, np.uint8).reshape(-1, 4)
        fmt, dtype = self._batch_format(pal.shape[0], format)
        outs = self._batch_outputs(imgs, fmt, dtype, out)
        src, ws, hs = self._batch_arrays(imgs)
        dst = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        rep = BatchApplyReport()
        _check(lib().kmg_find_batch(self._h, n, src, ws, hs, _np_ptr(pal), pal.shape[0], int(reduce_mode), int(fmt), int(max_resident_bytes),
                                    dst, C.byref(rep)))
        self.last_batch_apply_report = rep
        return outs

    def reduce_indexed_batch(self, color_count, images, algo=Algorithm.Kmeans, reduce_mode=ReduceMode.Replace, format=None,
                             max_resident_bytes=0, out=None):
        """kmg_reduce_indexed_batch: reduce_indexed() of many images -- one launch chain for their palettes, one launch for their
        output passes; returns the list of (palette, index_map), each what reduce_indexed returns for that image
        (format=OutputFormat.RGBA8: the image reduce returns in place of the map).  The reports of the call: last_batch_report and
        last_batch_apply_report.  out: optional list of arrays that receive the maps"""
        imgs = [_image(im) for im in images]
        n = len(imgs)
        fmt, dtype = self._batch_format(int(color_count), format)
        outs = self._batch_outputs(imgs, fmt, dtype, out)
        pals = [np.empty((max(int(color_count), 1), 4), np.uint8) for _ in imgs]
        src, ws, hs = self._batch_arrays(imgs)
        dst = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        pdst = (C.c_void_p * n)(*[q.ctypes.data for q in pals])
        counts = np.zeros(max(n, 1), np.uint32)
        rep, arep = BatchReport(), BatchApplyReport()
        _check(lib().kmg_reduce_indexed_batch(self._h, n, src, ws, hs, int(color_count), int(algo), int(reduce_mode), int(fmt),
                                              int(max_resident_bytes), pdst, _np_ptr(counts), dst, C.byref(rep), C.byref(arep)))
        self.last_batch_report, self.last_batch_apply_report = rep, arep
        return [(q[:int(c)].copy(), o) for q, c, o in zip(pals, counts, outs)]

    def apply_batch_device(self, d_images, widths, heights, centroids4, reduce_mode, format, d_outs, stream=0):
        """kmg_dev_apply_batch: the output pass of images in device memory (d_images, d_outs: their addresses) in one launch;
        centroids4: (k, 4) float32 -- one table for all images -- or (n, k, 4), table i for image i.  Synchronises the stream.
        The report of the call: last_batch_apply_report"""
        n = len(d_images)
        c4 = np.ascontiguousarray(centroids4, np.float32)
        n_tables = 1 if c4.ndim == 2 else c4.shape[0]
        k = c4.shape[-2]
        src = (C.c_void_p * n)(*[int(d) for d in d_images])
        dst = (C.c_void_p * n)(*[int(d) for d in d_outs])
        ws = (C.c_uint32 * n)(*[int(w) for w in widths])
        hs = (C.c_uint32 * n)(*[int(h) for h in heights])
        rep = BatchApplyReport()
        _check(lib().kmg_dev_apply_batch(self._h, n, src, ws, hs, _np_ptr(c4), n_tables, k, int(reduce_mode), int(format), dst,
                                         C.byref(rep), C.c_void_p(stream)))
        self.last_batch_apply_report = rep
        return rep

    # ---- batched quality targets (include/kmeans_hip.h kmg_batch_quality_report) ----------------
    def palette_batch_counts_device(self, d_images, widths, heights, ks, stream=0):
        """kmg_dev_palette_batch_counts: palette_batch_device with a colour count per image -> (list of centroid tables, table i
        (ks[i], 4) float32 in index order, iterations (n,) uint32).  The report of the call: last_batch_report"""
        n = len(d_images)
        src = (C.c_void_p * n)(*[int(d) for d in d_images])
        ws = (C.c_uint32 * n)(*[int(w) for w in widths])
        hs = (C.c_uint32 * n)(*[int(h) for h in heights])
        counts = np.ascontiguousarray(ks, np.uint32).reshape(-1)
        cent = np.empty((max(int(counts.sum()), 1), 4), np.float32)
        its = np.zeros(max(n, 1), np.uint32)
        rep = BatchReport()
        _check(lib().kmg_dev_palette_batch_counts(self._h, n, src, ws, hs, _np_ptr(counts), _np_ptr(cent), _np_ptr(its), C.byref(rep),
                                                  C.c_void_p(stream)))
        self.last_batch_report = rep
        ends = np.cumsum(counts)
        return [cent[e - k:e].copy() for e, k in zip(ends, counts)], its[:n]

    def apply_batch_counts_device(self, d_images, widths, heights, tables, reduce_mode, format, d_outs, stream=0):
        """kmg_dev_apply_batch_counts: apply_batch_device with a table per image of its own size; tables: one (k_i, 4) float32
        array per image.  Synchronises the stream.  The report of the call: last_batch_apply_report"""
        n = len(d_images)
        tabs = [np.ascontiguousarray(t, np.float32).reshape(-1, 4) for t in tables]
        counts = np.array([t.shape[0] for t in tabs], np.uint32)
        c4 = np.ascontiguousarray(np.concatenate(tabs) if tabs else np.zeros((1, 4)), np.float32)
        src = (C.c_void_p * n)(*[int(d) for d in d_images])
        dst = (C.c_void_p * n)(*[int(d) for d in d_outs])
        ws = (C.c_uint32 * n)(*[int(w) for w in widths])
        hs = (C.c_uint32 * n)(*[int(h) for h in heights])
        rep = BatchApplyReport()
        _check(lib().kmg_dev_apply_batch_counts(self._h, n, src, ws, hs, _np_ptr(c4), _np_ptr(counts), int(reduce_mode), int(format), dst,
                                                C.byref(rep), C.c_void_p(stream)))
        self.last_batch_apply_report = rep
        return rep

    def compare_batch_device(self, d_srcs, d_outs, n_pixels, format, palettes, alpha_cutoff, what, d_stats, stream=0):
        """kmg_dev_compare_batch: COMBINES the error record of every image into the n records at d_stats (device memory, 112 bytes
        each).  palettes: one (k_i, 4) uint8 array per image (index formats), or None.  Enqueues on the stream only."""
        n = len(d_srcs)
        src = (C.c_void_p * n)(*[int(d) for d in d_srcs])
        dst = (C.c_void_p * n)(*[int(d) for d in d_outs])
        npx = (C.c_uint64 * n)(*[int(v) for v in n_pixels])
        if palettes is None:
            pal, counts = None, None
        else:
            pals = [np.ascontiguousarray(q, np.uint8).reshape(-1, 4) for q in palettes]
            counts = np.array([q.shape[0] for q in pals], np.uint32)
            pal = np.ascontiguousarray(np.concatenate(pals))
        _check(lib().kmg_dev_compare_batch(self._h, n, src, dst, npx, int(format), None if pal is None else _np_ptr(pal),
                                           None if counts is None else _np_ptr(counts), int(alpha_cutoff), int(what), C.c_void_p(d_stats),
                                           C.c_void_p(stream)))

    def reduce_quality_batch(self, images, max_delta_e, k_min=2, k_max=256, reduce_mode=ReduceMode.Replace, indexed=False, format=None,
                             max_resident_bytes=0):
        """kmg_reduce_quality_batch: reduce_quality() of many images, every round of their searches one launch chain; returns the
        list of (k, colors, image or index map, ErrorStats, reached), each what reduce_quality returns for that image.  format:
        the output format, or None = what reduce_quality chooses (indexed).  The report of the call: last_quality_report"""
        imgs = [_image(im) for im in images]
        n = len(imgs)
        target = min(int(np.floor(4096.0 * float(max_delta_e) * float(max_delta_e))), 0xFFFFFFFF)
        fmt = OutputFormat(format) if format is not None else (self._index_format(int(k_max)) if indexed else OutputFormat.RGBA8)
        dtype = np.uint16 if fmt == OutputFormat.Index16 else np.uint8
        outs = self._batch_outputs(imgs, fmt, dtype, None)
        pals = [np.empty((max(int(k_max), 1), 4), np.uint8) for _ in imgs]
        src, ws, hs = self._batch_arrays(imgs)
        dst = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        pdst = (C.c_void_p * n)(*[q.ctypes.data for q in pals])
        counts = np.zeros(max(n, 1), np.uint32)
        stats = (ErrorStats * max(n, 1))()
        reached = (C.c_int * max(n, 1))()
        rep = BatchQualityReport()
        _check(lib().kmg_reduce_quality_batch(self._h, n, src, ws, hs, int(k_min), int(k_max), target, int(reduce_mode), int(fmt),
                                              int(max_resident_bytes), pdst, _np_ptr(counts), dst, stats, reached, C.byref(rep)))
        self.last_quality_report = rep
        return [(int(counts[i]), pals[i][:int(counts[i])].copy(), outs[i], stats[i], bool(reached[i])) for i in range(n)]

    # ---- palette-index output (include/kmeans_hip.h kmg_output_format) ----------------------
    def _index_format(self, k):
        """INDEX8 when the k labels (and, in alpha mode, the transparent slot k) fit a byte, else INDEX16"""
        return OutputFormat.Index8 if k + (1 if self.options.alpha_cutoff else 0) <= 256 else OutputFormat.Index16

    def find_indexed(self, image, colors, reduce_mode=ReduceMode.Replace):
        """kmg_find_indexed: (height, width) palette indices into `colors` -- uint8, or uint16 when they do not fit a byte
        (alpha mode: index len(colors) marks a pixel below the cutoff)"""
        img = _image(image)
        h, w = img.shape[:2]
        pal = np.ascontiguousarray(colors, np.uint8).reshape(-1, 4)
        fmt = self._index_format(pal.shape[0])
        out = np.empty((h, w), np.uint8 if fmt == OutputFormat.Index8 else np.uint16)
        _check(lib().kmg_find_indexed(self._h, _np_ptr(img), w, h, _np_ptr(pal), pal.shape[0], int(reduce_mode), int(fmt),
                                      out.ctypes.data_as(C.c_void_p)))
        return out

    def reduce_indexed(self, color_count, image, algo=Algorithm.Kmeans, reduce_mode=ReduceMode.Replace):
        """kmg_reduce_indexed: (palette (n, 4) uint8 in index order, (height, width) indices) -- palette[index] is what reduce
        writes for the pixel (its alpha aside in alpha mode, where index n marks a pixel below the cutoff)"""
        img = _image(image)
        h, w = img.shape[:2]
        fmt = self._index_format(int(color_count))
        out = np.empty((h, w), np.uint8 if fmt == OutputFormat.Index8 else np.uint16)
        pal = np.empty((max(int(color_count), 1), 4), np.uint8)
        cnt = C.c_uint32()
        _check(lib().kmg_reduce_indexed(self._h, _np_ptr(img), w, h, int(color_count), int(algo), int(reduce_mode), int(fmt), _np_ptr(pal),
                                        C.byref(cnt), out.ctypes.data_as(C.c_void_p)))
        return pal[:cnt.value].copy(), out

    # ---- error statistics and the quality-targeted colour count (include/kmeans_hip.h kmg_error_stats) --------
    def compare(self, src, out, palette=None, what=ERROR_RGB | ERROR_LAB):
        """kmg_compare: the ErrorStats of `out` against the image `src`.  out: a (height, width, 4) uint8 image, or -- with
        `palette` (n, 4) -- a (height, width) uint8 / uint16 index map into it.  Uses the processor's alpha_cutoff: a pixel counts
        iff the source's alpha reaches it."""
        img = _image(src)
        h, w = img.shape[:2]
        o = np.ascontiguousarray(out)
        if palette is None:
            if o.dtype != np.uint8 or o.shape != img.shape:
                raise ValueError("out must be a uint8 image of the source's shape (or an index map, with palette=)")
            fmt, pal, k = OutputFormat.RGBA8, None, 0
        else:
            if o.shape != (h, w) or o.dtype not in (np.uint8, np.uint16):
                raise ValueError("out must be a (height, width) uint8 or uint16 index map")
            pal = np.ascontiguousarray(palette, np.uint8).reshape(-1, 4)
            fmt, k = (OutputFormat.Index8 if o.dtype == np.uint8 else OutputFormat.Index16), pal.shape[0]
        stats = ErrorStats()
        _check(lib().kmg_compare(self._h, _np_ptr(img), _np_ptr(o), w, h, int(fmt), _np_ptr(pal) if pal is not None else None, k,
                                 int(what), C.byref(stats)))
        return stats

    def compare_device(self, d_src, d_out, n_pixels, d_stats, format=OutputFormat.RGBA8, palette=None, alpha_cutoff=0,
                       what=ERROR_RGB | ERROR_LAB, stream=0):
        """kmg_dev_compare: COMBINES the statistics of n_pixels pixels into the 14 uint64 at d_stats (device; the caller zeroes them
        for a fresh record).  Only enqueues; palette: host (n, 4) uint8 for the index formats."""
        pal = None if palette is None else np.ascontiguousarray(palette, np.uint8).reshape(-1, 4)
        _check(lib().kmg_dev_compare(self._h, C.c_void_p(d_src), C.c_void_p(d_out), int(n_pixels), int(format),
                                     _np_ptr(pal) if pal is not None else None, pal.shape[0] if pal is not None else 0,
                                     int(alpha_cutoff), int(what), C.c_void_p(d_stats), C.c_void_p(stream)))

    # ---- index-map optimisation (include/kmeans_hip.h kmg_index_plan) --------------------------------------
    def index_usage_device(self, d_index, n_pixels, format, k, d_usage, stream=0):
        """kmg_dev_index_usage: ADDS the counts of n_pixels indices to the k + 2 uint64 at d_usage (device; the caller zeroes a
        fresh record): [i] pixels with index i, [k] the transparent slot, [k + 1] indices above k.  Only enqueues."""
        _check(lib().kmg_dev_index_usage(self._h, C.c_void_p(d_index), int(n_pixels), int(format), int(k), C.c_void_p(d_usage),
                                         C.c_void_p(stream)))

    def index_remap_device(self, d_in, in_format, width, rows, k, remap, out_bits, d_out, d_bad, stream=0):
        """kmg_dev_index_remap: d_out = remap[d_in] at out_bits per pixel (1 / 2 / 4: packed rows); remap: host (k + 1,) uint16;
        ADDS the bad pixels (written as 0) to the uint64 at d_bad (device).  Only enqueues."""
        r = np.ascontiguousarray(remap, np.uint16).reshape(-1)
        if r.shape[0] != int(k) + 1:
            raise ValueError("remap must hold k + 1 entries")
        _check(lib().kmg_dev_index_remap(self._h, C.c_void_p(d_in), int(in_format), int(width), int(rows), int(k), _np_ptr(r), int(out_bits),
                                         C.c_void_p(d_out), C.c_void_p(d_bad), C.c_void_p(stream)))

    @staticmethod
    def _index_map(index):
        a = np.ascontiguousarray(index)
        if a.ndim != 2 or a.dtype not in (np.uint8, np.uint16):
            raise ValueError("index map must be a (height, width) uint8 or uint16 array")
        return a, (OutputFormat.Index8 if a.dtype == np.uint8 else OutputFormat.Index16)

    def index_usage(self, index, k, usage=None):
        """kmg_index_usage: the k + 2 counts of a (height, width) uint8 / uint16 map, ADDED to `usage` when given (frames of a
        sequence accumulate into one record)"""
        a, fmt = self._index_map(index)
        use = np.zeros(int(k) + 2, np.uint64) if usage is None else usage
        if use.dtype != np.uint64 or use.shape != (int(k) + 2,) or not use.flags.c_contiguous:
            raise ValueError("usage must be a contiguous (k + 2,) uint64 array")
        _check(lib().kmg_index_usage(self._h, _np_ptr(a), int(fmt), a.size, int(k), _np_ptr(use)))
        return use

    def index_remap(self, index, k, remap, bits):
        """kmg_index_remap: (remap[index] at `bits` per pixel -- (height, stride) uint8 packed rows for 1 / 2 / 4, a (height, width)
        uint8 / uint16 map for 8 / 16 --, the number of bad pixels, written as 0)"""
        a, fmt = self._index_map(index)
        h, w = a.shape
        r = np.ascontiguousarray(remap, np.uint16).reshape(-1)
        if r.shape[0] != int(k) + 1:
            raise ValueError("remap must hold k + 1 entries")
        if bits not in (1, 2, 4, 8, 16):
            raise ValueError("bits must be 1, 2, 4, 8 or 16")
        out = np.empty((h, w), np.uint16) if bits == 16 else np.empty((h, packed_stride(w, bits)), np.uint8)
        bad = C.c_uint64()
        _check(lib().kmg_index_remap(self._h, _np_ptr(a), int(fmt), w, h, int(k), _np_ptr(r), int(bits), _np_ptr(out), C.byref(bad)))
        return out, int(bad.value)

    def optimize_indexed(self, index, palette, flags=INDEX_ORDER_USAGE | INDEX_TRANSPARENT_FIRST, bits=None):
        """kmg_index_optimize: prune and order the palette of a (height, width) index map and rewrite the map for it.  Returns
        (palette_out (n_slots, 4) uint8 -- (0, 0, 0, 0) at info.transparent --, the map at info.bits (bits=None) or `bits` per pixel:
        packed rows (height, stride) uint8 for 1 / 2 / 4, (height, width) uint8 / uint16 for 8 / 16, IndexPlanInfo)."""
        a, fmt = self._index_map(index)
        h, w = a.shape
        pal = np.ascontiguousarray(palette, np.uint8).reshape(-1, 4)
        k = pal.shape[0]
        out_pal = np.empty((k + 1, 4), np.uint8)
        out = np.empty(a.nbytes, np.uint8)
        info = IndexPlanInfo()
        _check(lib().kmg_index_optimize(self._h, _np_ptr(a), int(fmt), w, h, _np_ptr(pal), k, int(flags), int(bits or 0), _np_ptr(out_pal),
                                        C.byref(info), _np_ptr(out)))
        b = int(bits or info.bits)
        if b == 16:
            m = out[:h * w * 2].view(np.uint16).reshape(h, w).copy()
        else:
            stride = packed_stride(w, b)
            m = out[:h * stride].reshape(h, stride).copy()
        return out_pal[:info.n_slots].copy(), m, info

    def reduce_quality(self, image, max_delta_e, k_min=2, k_max=256, reduce_mode=ReduceMode.Replace, indexed=False):
        """kmg_reduce_quality: as few colours in [k_min, k_max] as keep the dE76 RMS of the palette step's working image at or below
        max_delta_e (target = floor(4096 max_delta_e^2)).  Returns (k, colors (k, 4) in index order, image or index map, ErrorStats
        of the working image at k, reached)."""
        img = _image(image)
        h, w = img.shape[:2]
        target = min(int(np.floor(4096.0 * float(max_delta_e) * float(max_delta_e))), 0xFFFFFFFF)
        if indexed:
            fmt = self._index_format(int(k_max))
            out = np.empty((h, w), np.uint8 if fmt == OutputFormat.Index8 else np.uint16)
        else:
            fmt, out = OutputFormat.RGBA8, _result(img, None)
        pal = np.empty((max(int(k_max), 1), 4), np.uint8)
        cnt, reached, stats = C.c_uint32(), C.c_int(), ErrorStats()
        _check(lib().kmg_reduce_quality(self._h, _np_ptr(img), w, h, int(k_min), int(k_max), target, int(reduce_mode), int(fmt), _np_ptr(pal),
                                        C.byref(cnt), out.ctypes.data_as(C.c_void_p), C.byref(stats), C.byref(reached)))
        return int(cnt.value), pal[:cnt.value].copy(), out, stats, bool(reached.value)

    # ---- device-pointer helpers (torch tensors supply the memory) -------------------------
    def rgb_to_lab(self, d_rgba, n_pixels, d_lab3, stream=0):
        _check(lib().kmg_dev_rgb_to_lab(self._h, C.c_void_p(d_rgba), n_pixels, C.c_void_p(d_lab3), C.c_void_p(stream)))

    def resize(self, d_rgba, width, height, new_width, new_height, d_out, stream=0):
        _check(lib().kmg_dev_resize(self._h, C.c_void_p(d_rgba), width, height, new_width, new_height,
                                    C.c_void_p(d_out), C.c_void_p(stream)))

    def alpha_compact(self, d_rgba, n_pixels, cutoff, d_out, d_n_kept, stream=0):
        """kmg_dev_alpha_compact: d_out[0 .. n_kept) = the pixels with alpha >= cutoff, in order; the u64 at d_n_kept (device) = n_kept"""
        _check(lib().kmg_dev_alpha_compact(self._h, C.c_void_p(d_rgba), int(n_pixels), int(cutoff), C.c_void_p(d_out),
                                           C.c_void_p(d_n_kept), C.c_void_p(stream)))

    def apply(self, d_rgba, width, rows, row0, centroids4, mode, d_out, stream=0, format=None):
        """format=None: kmg_dev_apply (RGBA8); an OutputFormat: kmg_dev_apply_format (d_out then holds 4, 1 or 2 bytes per pixel)"""
        c = np.ascontiguousarray(centroids4, np.float32).reshape(-1, 4)
        if format is None:
            _check(lib().kmg_dev_apply(self._h, C.c_void_p(d_rgba), width, rows, row0, _np_ptr(c), c.shape[0],
                                       int(mode), C.c_void_p(d_out), C.c_void_p(stream)))
        else:
            _check(lib().kmg_dev_apply_format(self._h, C.c_void_p(d_rgba), width, rows, row0, _np_ptr(c), c.shape[0],
                                              int(mode), int(format), C.c_void_p(d_out), C.c_void_p(stream)))

    def apply_plan(self, centroids4, mode, n_pixels_hint, stream=0, format=None):
        """the output pass as a plan (kmg_apply_plan_*): tables built once, then `run` per row band, asynchronously.  format: as
        for apply()"""
        return ApplyPlan(self, centroids4, mode, n_pixels_hint, stream, format)

    # ---- frame sequences (include/kmeans_hip.h kmg_sequence) ----------------------------------
    def sequence(self):
        """kmg_sequence_create: a Sequence -- one palette for many frames, and their index maps as delta frames"""
        import weakref
        seq = Sequence(self)
        if self._sequences is None:
            self._sequences = weakref.WeakSet()
        self._sequences.add(seq)
        return seq

    def frame_delta(self, d_index, d_canvas, width, rows, row0, format, k, d_delta, d_info, stream=0):
        """kmg_dev_frame_delta: d_delta = the band's indices where they differ from the canvas, k elsewhere; the canvas takes the
        indices; COMBINES counts and box into the 32-byte record at d_info (device; the caller writes FrameDelta.FRESH before a
        frame).  Only enqueues."""
        _check(lib().kmg_dev_frame_delta(self._h, C.c_void_p(d_index), C.c_void_p(d_canvas), int(width), int(rows), int(row0), int(format),
                                         int(k), C.c_void_p(d_delta), C.c_void_p(d_info), C.c_void_p(stream)))

    def frame_delta_lossy(self, d_src_rgba, d_index, d_canvas, d_held_rgba, width, rows, row0, format, k, tolerance, d_delta, d_info,
                          stream=0):
        """kmg_dev_frame_delta_lossy: the delta pass with a tolerance -- a pixel that shows a colour, stays opaque and whose source
        is within `tolerance` (1/4096 dE76^2) of its held source keeps its canvas index; every other pixel follows the exact rule and
        takes the source as its held source.  COMBINES into the 48-byte record at d_info (device; the caller writes FrameHold.FRESH
        before a frame).  Only enqueues."""
        _check(lib().kmg_dev_frame_delta_lossy(self._h, C.c_void_p(d_src_rgba), C.c_void_p(d_index), C.c_void_p(d_canvas),
                                               C.c_void_p(d_held_rgba), int(width), int(rows), int(row0), int(format), int(k), int(tolerance),
                                               C.c_void_p(d_delta), C.c_void_p(d_info), C.c_void_p(stream)))

    def frame_delta_clip(self, d_src_rgba, d_index, d_canvas, d_held_rgba, width, height, format, k, tolerances, d_out, d_info,
                         d_full=0, flags=0, stream=0):
        """kmg_dev_frame_delta_clip: every frame of a clip through the delta pass in one launch chain -- what len(d_index) calls of
        frame_delta (tolerances=None) or frame_delta_lossy (frame t at tolerances[t]) leave.  d_src_rgba (None for an exact clip),
        d_index, d_out: sequences of device pointers, one per frame; d_info: device, 48 bytes per frame, combined into; flags:
        CLIP_FULL_ON_CLEAR with d_full (device, a word per frame).  Only enqueues."""
        n = len(d_index)
        ptrs = lambda a: None if a is None else (C.c_void_p * max(len(a), 1))(*[int(v) if v else None for v in a])
        tol = None if tolerances is None else (C.c_uint32 * max(n, 1))(*[int(t) for t in tolerances])
        _check(lib().kmg_dev_frame_delta_clip(self._h, n, ptrs(d_src_rgba), ptrs(d_index), C.c_void_p(d_canvas), C.c_void_p(d_held_rgba),
                                              int(width), int(height), int(format), int(k), tol, int(flags), ptrs(d_out), C.c_void_p(d_info),
                                              C.c_void_p(d_full), C.c_void_p(stream)))

    def frame_delta_colour(self, d_index, d_palette_rgba, d_shown_rgba, width, rows, row0, format, k, d_delta, d_info, stream=0):
        """kmg_dev_frame_delta_colour: the delta pass for frames with a palette of their own -- the canvas d_shown_rgba holds the RGBA8
        word each pixel shows (0: nothing), a pixel is sent when palette[index] differs from it.  COMBINES into the 32-byte record at
        d_info (device; the caller writes FrameDelta.FRESH before a frame).  Only enqueues."""
        _check(lib().kmg_dev_frame_delta_colour(self._h, C.c_void_p(d_index), C.c_void_p(d_palette_rgba), C.c_void_p(d_shown_rgba), int(width),
                                                int(rows), int(row0), int(format), int(k), C.c_void_p(d_delta), C.c_void_p(d_info),
                                                C.c_void_p(stream)))

    def frame_delta_colour_lossy(self, d_src_rgba, d_index, d_palette_rgba, d_shown_rgba, d_held_rgba, width, rows, row0, format, k, tolerance,
                                 d_delta, d_info, stream=0):
        """kmg_dev_frame_delta_colour_lossy: the same with the hold rule of frame_delta_lossy -- a pixel that shows a colour, stays
        opaque and whose source is within `tolerance` of its held source keeps what it shows.  COMBINES into the 48-byte record at
        d_info (device; FrameHold.FRESH before a frame).  Only enqueues."""
        _check(lib().kmg_dev_frame_delta_colour_lossy(self._h, C.c_void_p(d_src_rgba), C.c_void_p(d_index), C.c_void_p(d_palette_rgba),
                                                      C.c_void_p(d_shown_rgba), C.c_void_p(d_held_rgba), int(width), int(rows), int(row0),
                                                      int(format), int(k), int(tolerance), C.c_void_p(d_delta), C.c_void_p(d_info),
                                                      C.c_void_p(stream)))

    def debug_block_counts(self):
        """(device blocks allocated with hipMalloc so far, blocks handed out again)"""
        out = (C.c_uint64 * 2)()
        _check(lib().kmg_debug_block_counts(self._h, out))
        return int(out[0]), int(out[1])

    def debug_idle_blocks(self):
        """(blocks the processor holds idle right now, their bytes)"""
        out = (C.c_uint64 * 2)()
        _check(lib().kmg_debug_idle_blocks(self._h, out))
        return int(out[0]), int(out[1])

    def debug_encode_table_check(self):
        """floats whose sRGB8 byte from the meld pass's threshold table differs from the encode's own byte (all floats tried)"""
        out = C.c_uint64(0)
        _check(lib().kmg_debug_encode_table_check(self._h, C.byref(out)))
        return int(out.value)

    def debug_division_check(self, c):
        """(mismatches, smallest |x| bits, largest |x| bits) of the device's x / c against IEEE division over every float x"""
        out = (C.c_uint64 * 3)()
        _check(lib().kmg_debug_division_check(self._h, C.c_float(c), out))
        return int(out[0]), int(out[1]), int(out[2])

    def debug_check_dither_masks(self, centroids4, stream=0):
        """exhaustive check of the pruned dither pass's candidate masks; returns the violation count"""
        c = np.ascontiguousarray(centroids4, np.float32).reshape(-1, 4)
        v = C.c_uint64()
        _check(lib().kmg_debug_check_dither_masks(self._h, _np_ptr(c), c.shape[0], C.byref(v), C.c_void_p(stream)))
        return int(v.value)

    def debug_check_meld_masks(self, centroids4, stream=0):
        """exhaustive check of the pruned meld pass's candidate masks; returns the violation count"""
        c = np.ascontiguousarray(centroids4, np.float32).reshape(-1, 4)
        v = C.c_uint64()
        _check(lib().kmg_debug_check_meld_masks(self._h, _np_ptr(c), c.shape[0], C.byref(v), C.c_void_p(stream)))
        return int(v.value)


class Sequence:
    """kmg_sequence_*: the working sequence of the frames added so far (each shrunk and, in alpha mode, compacted as the palette
    step does), its shared palette, and frame output with that palette as full or delta index maps.  Not re-entrant: one thread
    at a time."""

    def __init__(self, processor):
        self._p = processor
        self._h = C.c_void_p()
        self._out = None                # (k, format, width, height) of the open output
        self.last_clip_report = None    # ClipReport of the last frames() call
        _check(lib().kmg_sequence_create(processor.handle, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().kmg_sequence_destroy(self._h)
            self._h = C.c_void_p()
            self._out = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def add(self, image):
        """kmg_sequence_add: one more frame, a (height, width, 4) uint8 host image of any size"""
        img = _image(image)
        h, w = img.shape[:2]
        _check(lib().kmg_sequence_add(self._h, _np_ptr(img), w, h))

    def add_device(self, d_rgba, width, height, stream=0):
        """kmg_sequence_add_device: the same for a frame in device memory (synchronises `stream`)"""
        _check(lib().kmg_sequence_add_device(self._h, C.c_void_p(d_rgba), int(width), int(height), C.c_void_p(stream)))

    def clear(self):
        _check(lib().kmg_sequence_clear(self._h))

    def info(self):
        """(frames added, pixels of the working sequence)"""
        out = (C.c_uint64 * 2)()
        _check(lib().kmg_sequence_info(self._h, out))
        return int(out[0]), int(out[1])

    def centroids(self, k):
        """kmg_sequence_centroids: (k, 4) float32 in the Lloyd loop's order -- the order the index maps refer to"""
        out = np.empty((max(int(k), 1), 4), np.float32)
        _check(lib().kmg_sequence_centroids(self._h, int(k), _np_ptr(out)))
        return out

    def palette(self, k):
        """kmg_sequence_palette: (k, 4) uint8, sorted as ImageProcessor.palette sorts"""
        out = np.empty((max(int(k), 1), 4), np.uint8)
        cnt = C.c_uint32()
        _check(lib().kmg_sequence_palette(self._h, int(k), _np_ptr(out), C.byref(cnt)))
        return out[:cnt.value].copy()

    def output(self, k, mode=ReduceMode.Replace, format=OutputFormat.Index8, width=0, height=0):
        """kmg_sequence_output_begin: opens the frame output for frames of width x height; returns the palette (k, 4) in index
        order.  Index k of the maps is the transparent slot."""
        pal = np.empty((max(int(k), 1), 4), np.uint8)
        cnt = C.c_uint32()
        self._out = self._local = None
        _check(lib().kmg_sequence_output_begin(self._h, int(k), int(mode), int(format), int(width), int(height), _np_ptr(pal), C.byref(cnt)))
        self._out = (int(k), int(format), int(width), int(height))
        return pal[:cnt.value].copy()

    def frame(self, image, delta=True, tolerance=None):
        """kmg_sequence_output_frame: (map, FrameDelta, is_full).  delta=True: the delta map against the frames shown so far
        (index k = unchanged), or -- is_full -- the full map when a shown pixel turns transparent; delta=False: the full map.
        tolerance (an integer in 1/4096 dE76^2, see tolerance_of): kmg_sequence_output_frame_lossy -- a pixel whose source stays
        within it of the source it was last sent for keeps what it shows; the record then is a FrameHold.  Needs delta=True."""
        if self._out is None:
            raise KmgError(-1, "no output is open (Sequence.output)")
        k, fmt, w, h = self._out
        img = _image(image)
        if img.shape[:2] != (h, w):
            raise KmgError(-1, f"the frame is {img.shape[1]} x {img.shape[0]}, the output was opened for {w} x {h}")
        if fmt == OutputFormat.RGBA8:
            out = np.empty((h, w, 4), np.uint8)
        else:
            out = np.empty((h, w), np.uint8 if fmt == OutputFormat.Index8 else np.uint16)
        if tolerance is not None:
            tol = int(tolerance)
            if tol < 0 or tol > 0xFFFFFFFF:
                raise KmgError(-1, f"tolerance {tolerance!r} is not a uint32")
            hold, full = FrameHold(*FrameHold.FRESH), C.c_int(1)
            _check(lib().kmg_sequence_output_frame_lossy(self._h, _np_ptr(img), FRAME_DELTA if delta else 0, tol,
                                                         out.ctypes.data_as(C.c_void_p), C.byref(hold), C.byref(full)))
            return out, hold, bool(full.value)
        info, full = FrameDelta(*FrameDelta.FRESH), C.c_int(1)
        _check(lib().kmg_sequence_output_frame(self._h, _np_ptr(img), FRAME_DELTA if delta else 0, out.ctypes.data_as(C.c_void_p),
                                               C.byref(info), C.byref(full)))
        return out, info, bool(full.value)

    def frames(self, images, delta=True, tolerance=None, max_resident_bytes=0):
        """kmg_sequence_output_frames: a whole clip through the open output in one launch chain -- a list of (map, FrameDelta |
        FrameHold, is_full), frame by frame what frame() returns for the images one after another, and the same state afterwards.
        tolerance: None (exact), one integer for every frame, or one per frame.  Sets last_clip_report."""
        if self._out is None:
            raise KmgError(-1, "no output is open (Sequence.output)")
        k, fmt, w, h = self._out
        imgs = [_image(im) for im in images]
        for img in imgs:
            if img.shape[:2] != (h, w):
                raise KmgError(-1, f"a frame is {img.shape[1]} x {img.shape[0]}, the output was opened for {w} x {h}")
        n = len(imgs)
        if fmt == OutputFormat.RGBA8:
            outs = [np.empty((h, w, 4), np.uint8) for _ in imgs]
        else:
            outs = [np.empty((h, w), np.uint8 if fmt == OutputFormat.Index8 else np.uint16) for _ in imgs]
        tol = None
        if tolerance is not None:
            tols = [int(t) for t in tolerance] if hasattr(tolerance, "__len__") else [int(tolerance)] * n
            if len(tols) != n or any(t < 0 or t > 0xFFFFFFFF for t in tols):
                raise KmgError(-1, f"tolerance {tolerance!r}: one uint32, or one per frame")
            tol = (C.c_uint32 * max(n, 1))(*tols)
        src = (C.c_void_p * max(n, 1))(*[im.ctypes.data for im in imgs])
        dst = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
        info = (FrameHold * max(n, 1))(*[FrameHold(*FrameHold.FRESH) for _ in range(max(n, 1))])
        full = (C.c_int * max(n, 1))(*([1] * max(n, 1)))
        report = ClipReport()
        _check(lib().kmg_sequence_output_frames(self._h, n, src, FRAME_DELTA if delta else 0, tol, int(max_resident_bytes), dst, info, full,
                                                C.byref(report)))
        self.last_clip_report = report
        rec = (lambda r: FrameHold.from_buffer_copy(bytes(r))) if tol is not None else (lambda r: FrameDelta.from_buffer_copy(bytes(r)[:32]))
        return [(outs[t], rec(info[t]), bool(full[t])) for t in range(n)]

    def output_local(self, k, mode=ReduceMode.Replace, format=OutputFormat.Index8, width=0, height=0, warm=False):
        """kmg_sequence_output_begin_local: opens a frame output in which every frame gets a palette of its own (no frame needs to
        have been added).  warm: the Lloyd loop of every frame after the first starts from the previous frame's centroids."""
        self._out = self._local = None
        _check(lib().kmg_sequence_output_begin_local(self._h, int(k), int(mode), int(format), int(width), int(height), LOCAL_WARM if warm else 0))
        self._local = (int(k), int(format), int(width), int(height))

    def frame_local(self, image, delta=True, tolerance=None):
        """kmg_sequence_output_frame_local: (map, palette (k, 4) in index order, FrameHold, is_full).  delta=True: the delta map of
        the frame's own map and palette against what is shown (index k = unchanged) -- exact, or with `tolerance` the lossy rule of
        Sequence.frame -- or, is_full, the full map when a shown pixel turns transparent; delta=False: the full map.  An exact frame
        leaves held = held_sse = 0 in the record."""
        if getattr(self, "_local", None) is None:
            raise KmgError(-1, "no output with per-frame palettes is open (Sequence.output_local)")
        k, fmt, w, h = self._local
        img = _image(image)
        if img.shape[:2] != (h, w):
            raise KmgError(-1, f"the frame is {img.shape[1]} x {img.shape[0]}, the output was opened for {w} x {h}")
        tol = None
        if tolerance is not None:
            if int(tolerance) < 0 or int(tolerance) > 0xFFFFFFFF:
                raise KmgError(-1, f"tolerance {tolerance!r} is not a uint32")
            tol = C.byref(C.c_uint32(int(tolerance)))
        out = np.empty((h, w), np.uint8 if fmt == OutputFormat.Index8 else np.uint16)
        pal, cnt = np.empty((k, 4), np.uint8), C.c_uint32()
        hold, full = FrameHold(*FrameHold.FRESH), C.c_int(1)
        _check(lib().kmg_sequence_output_frame_local(self._h, _np_ptr(img), FRAME_DELTA if delta else 0, tol, out.ctypes.data_as(C.c_void_p),
                                                     _np_ptr(pal), C.byref(cnt), C.byref(hold), C.byref(full)))
        return out, pal[:cnt.value].copy(), hold, bool(full.value)

    def end_output(self):
        self._out = self._local = None
        _check(lib().kmg_sequence_output_end(self._h))


class ApplyPlan:
    """kmg_apply_plan_*: the output pass for one centroid table, band by band, without host synchronisation"""

    def __init__(self, processor, centroids4, mode, n_pixels_hint, stream=0, format=None):
        c = np.ascontiguousarray(centroids4, np.float32).reshape(-1, 4)
        self._h = C.c_void_p()
        if format is None:
            _check(lib().kmg_apply_plan_create(processor.handle, _np_ptr(c), c.shape[0], int(mode), int(n_pixels_hint), C.c_void_p(stream),
                                               C.byref(self._h)))
        else:
            _check(lib().kmg_apply_plan_create_format(processor.handle, _np_ptr(c), c.shape[0], int(mode), int(format), int(n_pixels_hint),
                                                      C.c_void_p(stream), C.byref(self._h)))

    def run(self, d_rgba, width, rows, row0, d_out, stream=0):
        _check(lib().kmg_apply_plan_run(self._h, C.c_void_p(d_rgba), width, rows, row0, C.c_void_p(d_out), C.c_void_p(stream)))

    def status(self):
        """kmg_apply_plan_status: waits for the last run; raises if a diffusion run of the plan timed out"""
        _check(lib().kmg_apply_plan_status(self._h))

    def close(self, synchronise=True):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().kmg_apply_plan_destroy(self._h, int(bool(synchronise)))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Lloyd:
    """One Lloyd problem (an image or a row band of it) on one device: kmg_lloyd_* of the C ABI.
    Pointers are raw device addresses (e.g. torch.Tensor.data_ptr()); `stream` a hipStream_t."""

    def __init__(self, processor, k):
        self._p = processor
        self.k = int(k)
        self._h = C.c_void_p()
        _check(lib().kmg_lloyd_create(processor.handle, self.k, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().kmg_lloyd_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_centroids(self, centroids4, stream=0):
        c = np.ascontiguousarray(centroids4, np.float32).reshape(self.k, 4)
        _check(lib().kmg_lloyd_set_centroids(self._h, _np_ptr(c), C.c_void_p(stream)))

    def get_centroids(self, stream=0):
        out = np.empty((self.k, 4), np.float32)
        _check(lib().kmg_lloyd_get_centroids(self._h, _np_ptr(out), C.c_void_p(stream)))
        return out

    def init_centroids(self, d_rgba, width, height, stream=0):
        _check(lib().kmg_lloyd_init_centroids(self._h, C.c_void_p(d_rgba), width, height, C.c_void_p(stream)))

    # sharded (row band) initialisation steps -- what kmg_group_lloyd_init drives (tests/sharded_harness.py sharded_init)
    def init_centroids_seeded(self, d_rgba, width, height, seeds4, stream=0):
        """kmg_lloyd_init_centroids_seeded: centroids 0 .. n - 1 are the (n, 4) or (n, 3) Lab seeds, the others the farthest-point
        picks that follow them; no seed: init_centroids.  Seeds move with the first update unless set_fixed freezes them."""
        s = np.asarray(seeds4, np.float32)
        s = s.reshape(-1, s.shape[-1]) if s.size else np.zeros((0, 4), np.float32)
        c = np.ones((s.shape[0], 4), np.float32)
        c[:, :3] = s[:, :3]
        _check(lib().kmg_lloyd_init_centroids_seeded(self._h, C.c_void_p(d_rgba), int(width), int(height),
                                                     _np_ptr(c) if c.shape[0] else None, c.shape[0], C.c_void_p(stream)))

    def set_fixed(self, n_fixed):
        """kmg_lloyd_set_fixed: every update of this object leaves centroids 0 .. n_fixed - 1 alone and counts them as converged"""
        _check(lib().kmg_lloyd_set_fixed(self._h, int(n_fixed)))

    def set_weighting(self, weighting):
        """kmg_lloyd_set_weighting: WEIGHT_ALPHA (or True) = every later sum of this object weighs a pixel by its alpha byte"""
        _check(lib().kmg_lloyd_set_weighting(self._h, int(weighting)))

    def init_step(self, d_rgba, n_local, first_index, j, d_key, stream=0):
        _check(lib().kmg_lloyd_init_step(self._h, C.c_void_p(d_rgba or None), n_local, first_index, j,
                                         C.c_void_p(d_key), C.c_void_p(stream)))

    def init_pick_band(self, d_rgba, n_local, first_index, d_key, d_colour2, stream=0):
        _check(lib().kmg_lloyd_init_pick_band(self._h, C.c_void_p(d_rgba or None), n_local, first_index,
                                              C.c_void_p(d_key), C.c_void_p(d_colour2), C.c_void_p(stream)))

    def set_centroid_rgba(self, j, d_colour, stream=0):
        _check(lib().kmg_lloyd_set_centroid_rgba(self._h, j, C.c_void_p(d_colour), C.c_void_p(stream)))

    @staticmethod
    def init_first_key(width, height):
        return int(lib().kmg_init_first_key(width, height))

    def assign_accumulate(self, d_rgba, n_pixels, d_labels, d_acc4, stream=0):
        _check(lib().kmg_lloyd_assign_accumulate(self._h, C.c_void_p(d_rgba), n_pixels,
                                                 C.c_void_p(d_labels or None), C.c_void_p(d_acc4 or None),
                                                 C.c_void_p(stream)))

    def assign_partials(self, d_rgba, n_pixels, d_labels, stream=0):
        _check(lib().kmg_lloyd_assign_partials(self._h, C.c_void_p(d_rgba), n_pixels,
                                               C.c_void_p(d_labels or None), C.c_void_p(stream)))

    def labels(self, d_rgba, n_pixels, d_labels, stream=0):
        """labels only, for the current centroid table"""
        _check(lib().kmg_lloyd_labels(self._h, C.c_void_p(d_rgba), n_pixels, C.c_void_p(d_labels), C.c_void_p(stream)))

    def reserve_cus(self, n_cus):
        """leave n_cus compute units without a label-pass workgroup, for a collective that runs beside the pass"""
        _check(lib().kmg_lloyd_reserve_cus(self._h, int(n_cus)))

    def reduce_partials(self, n_pixels, d_acc4, stream=0):
        _check(lib().kmg_lloyd_reduce_partials(self._h, n_pixels, C.c_void_p(d_acc4), C.c_void_p(stream)))

    def bind_image(self, d_rgba, n_pixels, stream=0):
        """build the colour table of this image once; later passes on it use the table"""
        _check(lib().kmg_lloyd_bind_image(self._h, C.c_void_p(d_rgba), n_pixels, C.c_void_p(stream)))

    def prepare(self, d_rgba, n_pixels, want_labels=True, stream=0):
        """one-time per-image preparation; returns the chosen strategy ("scan" or "table")"""
        st = C.c_int()
        _check(lib().kmg_lloyd_prepare(self._h, C.c_void_p(d_rgba), n_pixels, int(bool(want_labels)),
                                       C.byref(st), C.c_void_p(stream)))
        return "table" if st.value == 1 else "scan"

    KERNEL_IDS = {"k_assign": 0, "k_reduce_partials": 1, "k_update": 2, "k_cell_candidates": 3, "k_cube": 4,
                  "k_labels": 5}

    def profile(self, enable=True):
        """start / stop per-launch HIP-event timing: True = every kernel, False = stop, or an iterable
        of kernel names (KERNEL_IDS) to time only those"""
        if enable is True:
            mask = -1
        elif not enable:
            mask = 0
        else:
            mask = 0
            for name in enable:
                mask |= 1 << self.KERNEL_IDS[name]
        _check(lib().kmg_lloyd_profile(self._h, mask))

    def profile_read(self):
        """{kernel name: (total ms, launches)} since the last read; synchronises the events"""
        n = 6
        ms = (C.c_double * n)()
        cnt = (C.c_uint32 * n)()
        _check(lib().kmg_lloyd_profile_read(self._h, ms, cnt))
        return {lib().kmg_kernel_name(i).decode(): (ms[i], cnt[i]) for i in range(n) if cnt[i]}

    def unbind_image(self):
        _check(lib().kmg_lloyd_unbind_image(self._h))

    def debug_check_table(self, stream=0):
        """exhaustive check over all 2^24 colours: (bound violations, arg-mins missing from the cell masks,
        per-colour labels that differ from the brute-force arg-min)"""
        out = (C.c_uint64 * 3)()
        _check(lib().kmg_debug_check_table(self._h, out, C.c_void_p(stream)))
        return int(out[0]), int(out[1]), int(out[2])

    def debug_table_stats(self, stream=0):
        out = (C.c_uint64 * 14)()
        _check(lib().kmg_debug_table_stats(self._h, out, C.c_void_p(stream)))
        names = ["occupied_cells", "candidates_total", "cells_one_candidate", "max_candidates",
                 "cells_one_label", "occupied_sub_cells", "sub_cells_one_label", "distinct_colours",
                 "sub_cells_decided", "sub_cells_scanned", "scan_candidates", "cells_unlisted",
                 "candidates_pruned", "sub_cells_pruned_to_one"]
        return dict(zip(names, (int(v) for v in out)))

    def debug_bound_image(self):
        """(occupied cells, hot cells) of the bound image"""
        out = (C.c_uint64 * 2)()
        _check(lib().kmg_debug_bound_image(self._h, out))
        return int(out[0]), int(out[1])

    def debug_check_pairs(self, stream=0):
        """(mismatching colours, pixels resolved by the LDS pair entries, pixels) of the last table pass"""
        out = (C.c_uint64 * 3)()
        _check(lib().kmg_debug_check_pairs(self._h, out, C.c_void_p(stream)))
        return int(out[0]), int(out[1]), int(out[2])

    def update(self, d_acc4, stream=0):
        _check(lib().kmg_lloyd_update(self._h, C.c_void_p(d_acc4), C.c_void_p(stream)))

    def set_cell_share(self, part, parts, stream=0):
        """cell-sharded cube pass: later assign passes of the bound image visit share `part` of `parts` of its occupied cells"""
        _check(lib().kmg_lloyd_set_cell_share(self._h, int(part), int(parts), C.c_void_p(stream)))

    def accumulate_into(self, d_rgba, n_pixels, d_acc4, stream=0):
        """the cube pass of the bound image ADDS its sums to d_acc4 as it stands (no hand-over launch)"""
        _check(lib().kmg_lloyd_accumulate_into(self._h, C.c_void_p(d_rgba), int(n_pixels), C.c_void_p(d_acc4), C.c_void_p(stream)))

    def labels_from_tables_update(self, d_rgba, n_pixels, d_labels, d_acc4, stream=0):
        """label map from the tables as they stand + kmg_lloyd_update from d_acc4, which is left zero (one launch)"""
        _check(lib().kmg_lloyd_labels_from_tables_update(self._h, C.c_void_p(d_rgba), int(n_pixels), C.c_void_p(d_labels), C.c_void_p(d_acc4),
                                                         C.c_void_p(stream)))

    def labels_from_tables(self, d_rgba, n_pixels, d_labels, stream=0):
        """the label pass with the label tables as they stand, on any pixels whose colours occur in the bound image"""
        _check(lib().kmg_lloyd_labels_from_tables(self._h, C.c_void_p(d_rgba), n_pixels, C.c_void_p(d_labels), C.c_void_p(stream)))

    def histogram_buffer(self):
        """(pointer, bytes) of the bound image's colour histogram (2^24 u32, cell-major colour order)"""
        a, na = C.c_void_p(), C.c_uint64()
        _check(lib().kmg_lloyd_histogram_buffer(self._h, C.byref(a), C.byref(na)))
        return a.value, na.value

    def rebuild_from_histogram(self, n_pixels, stream=0):
        """re-derive the binding from the (all-reduced) histogram, which now counts n_pixels pixels"""
        _check(lib().kmg_lloyd_rebuild_from_histogram(self._h, int(n_pixels), C.c_void_p(stream)))

    def histogram_tensor(self):
        """the bound image's colour histogram as a torch tensor that ALIASES the library's buffer (int32 [2^24]) -- for the
        all-reduce of a cell-sharded loop (kmg_group_lloyd_* with KMG_GROUP_CELLS; tests/sharded_harness.py)"""
        ptr, nbytes = self.histogram_buffer()
        return _alias_tensor(ptr, nbytes // 4, "<i4")

    def table_tensors(self):
        """(per-colour labels uint8 [2^24], cell entries int32 [32768]) of the bound image, k <= 256, as torch tensors that
        ALIAS the library's label tables -- for the all-gather of a cell-sharded loop"""
        lab, nlab, ent, nent = self.table_buffers()
        if nlab != 1 << 24:
            raise KmgError("table_tensors: the cell-sharded loop needs k <= 256")
        n_cells, n_sub = 32768, 32768 * 8
        return _alias_tensor(lab, nlab, "|u1"), _alias_tensor(ent + 2 * (n_sub + n_cells), n_cells, "<i4")

    def table_buffers(self):
        """(per-colour label table pointer, bytes, cell entry table pointer, bytes) of the bound image"""
        a, na, b, nb = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
        _check(lib().kmg_lloyd_table_buffers(self._h, C.byref(a), C.byref(na), C.byref(b), C.byref(nb)))
        return a.value, na.value, b.value, nb.value

    def assign_update(self, d_rgba, n_pixels, d_labels, d_acc4, do_update=True, stream=0):
        """assign (labels optional, sums into d_acc4), then -- do_update -- the centroid update from those sums"""
        _check(lib().kmg_lloyd_assign_update(self._h, C.c_void_p(d_rgba), n_pixels, C.c_void_p(d_labels or None),
                                             C.c_void_p(d_acc4), int(bool(do_update)), C.c_void_p(stream)))

    def iterate(self, d_rgba, n_pixels, d_labels, d_acc4, update_first=True, stream=0):
        """one Lloyd iteration, asynchronous; the label map is complete after flush() (or a device sync)"""
        _check(lib().kmg_lloyd_iterate(self._h, C.c_void_p(d_rgba), n_pixels, C.c_void_p(d_labels or None),
                                       C.c_void_p(d_acc4), int(bool(update_first)), C.c_void_p(stream)))

    def flush(self, stream=0):
        """make `stream` wait for the label passes that iterate() left running on the library's side stream"""
        _check(lib().kmg_lloyd_flush(self._h, C.c_void_p(stream)))

    def converged_count(self, stream=0):
        n = C.c_uint32()
        _check(lib().kmg_lloyd_converged_count(self._h, C.byref(n), C.c_void_p(stream)))
        return n.value

    def run(self, d_rgba, n_pixels, d_labels=0, stream=0):
        it = C.c_uint32()
        _check(lib().kmg_lloyd_run(self._h, C.c_void_p(d_rgba), n_pixels, C.c_void_p(d_labels or None),
                                   C.byref(it), C.c_void_p(stream)))
        return it.value


class _BorrowedProcessor(ImageProcessor):
    """a member processor of a Group: the group owns it"""

    def __init__(self, handle):                      # pylint: disable=super-init-not-called
        self._h = C.c_void_p(handle)

    def close(self):
        self._h = C.c_void_p()


class _BorrowedLloyd(Lloyd):
    """a member kmg_lloyd of a GroupLloyd (profiling, statistics): the group owns it"""

    def __init__(self, handle, k):                   # pylint: disable=super-init-not-called
        self._h = C.c_void_p(handle)
        self.k = int(k)

    def close(self):
        self._h = C.c_void_p()


class Group:
    """kmg_group_*: ImageProcessor::new (core/src/lib.rs:38-65) over a device LIST -- one processor, compute stream and RCCL
    rank per device.  `devices` = HIP ordinals of this process's ranks (None = every visible device).  One process per GPU:
    rank 0 makes `unique_id()`, the host runtime hands it to every process, each passes it with its `first_rank` and `world`.
    palette / find / reduce mirror ImageProcessor's and give the same bytes."""

    def __init__(self, devices=None, flags=0, unique_id=None, first_rank=0, world=None, shrink_max_dim=256, max_iterations=128,
                 check_period=8, convergence=1.0, strategy=None, alpha_cutoff=0):
        o = GroupOptions()
        lib().kmg_default_group_options(C.byref(o))
        if devices is not None:
            devices = [int(d) for d in devices]
            if len(devices) > MAX_DEVICES:
                raise ValueError("too many devices")
            o.n_devices = len(devices)
            for i, d in enumerate(devices):
                o.devices[i] = d
        o.flags = int(flags)
        o.processor.shrink_max_dim = shrink_max_dim
        o.processor.max_iterations = max_iterations
        o.processor.check_period = check_period
        o.processor.convergence = convergence
        o.processor.strategy = _default_strategy if strategy is None else _strategy_value(strategy)
        o.processor.alpha_cutoff = int(alpha_cutoff)     # (kmg_group_create refuses anything but 0: the group has no alpha mode)
        self._h = C.c_void_p()
        if unique_id is None:
            _check(lib().kmg_group_create(C.byref(o), C.byref(self._h)))
        else:
            if world is None:
                raise ValueError("Group(unique_id=...) is one process of a multi-process world: pass world (and first_rank)")
            uid = (C.c_uint8 * UNIQUE_ID_BYTES).from_buffer_copy(bytes(unique_id))
            _check(lib().kmg_group_create_rank(C.byref(o), uid, int(first_rank), int(world), C.byref(self._h)))
        a, b, c, v = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_int()
        _check(lib().kmg_group_info(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(v)))
        self.n_local, self.first_rank, self.world, self.rccl_version = a.value, b.value, c.value, v.value
        self.options = o
        _register(self)

    def set_strategy(self, strategy):
        """kmg_processor_set_strategy on every member processor"""
        if not self._h.value:
            return
        L = lib()
        for i in range(self.n_local):
            _check(L.kmg_processor_set_strategy(L.kmg_group_processor(self._h, i), _strategy_value(strategy)))

    @staticmethod
    def unique_id():
        """ncclGetUniqueId through the library (loads RCCL): 128 bytes for every process of the job"""
        buf = (C.c_uint8 * UNIQUE_ID_BYTES)()
        _check(lib().kmg_group_unique_id(buf))
        return bytes(buf)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().kmg_group_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        return self._h

    def processor(self, i=0):
        return _BorrowedProcessor(lib().kmg_group_processor(self._h, int(i)))

    def stream(self, i=0):
        """local device i's compute stream (hipStream_t as an integer): everything the group enqueues there runs on it"""
        return int(lib().kmg_group_stream(self._h, int(i)) or 0)

    def palette(self, color_count, image, algo=Algorithm.Kmeans):
        img = _image(image)
        h, w = img.shape[:2]
        out = np.empty((max(int(color_count), 1), 4), np.uint8)
        cnt = C.c_uint32()
        _check(lib().kmg_group_palette(self._h, _np_ptr(img), w, h, int(color_count), int(algo), _np_ptr(out), C.byref(cnt)))
        return out[:cnt.value].copy()

    def find(self, image, colors, reduce_mode=ReduceMode.Replace, out=None):
        img = _image(image)
        h, w = img.shape[:2]
        pal = np.ascontiguousarray(colors, np.uint8).reshape(-1, 4)
        out = _result(img, out)
        _check(lib().kmg_group_find(self._h, _np_ptr(img), w, h, _np_ptr(pal), pal.shape[0], int(reduce_mode), _np_ptr(out)))
        return out

    def reduce(self, color_count, image, algo=Algorithm.Kmeans, reduce_mode=ReduceMode.Replace, out=None):
        img = _image(image)
        h, w = img.shape[:2]
        out = _result(img, out)
        _check(lib().kmg_group_reduce(self._h, _np_ptr(img), w, h, int(color_count), int(algo), int(reduce_mode), _np_ptr(out)))
        return out

    def reduce_batch(self, color_count, images, algo=Algorithm.Kmeans, reduce_mode=ReduceMode.Replace):
        """whole images per device, no collective (BASELINE config 4 as placed); returns the list of results"""
        imgs = [_image(im) for im in images]
        outs = [_result(im, None) for im in imgs]          # (large results from the pool of page-locked blocks, as reduce() does)
        n = len(imgs)
        src = (C.c_void_p * n)(*[im.ctypes.data for im in imgs])
        dst = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        ws = (C.c_uint32 * n)(*[im.shape[1] for im in imgs])
        hs = (C.c_uint32 * n)(*[im.shape[0] for im in imgs])
        _check(lib().kmg_group_reduce_batch(self._h, n, src, ws, hs, int(color_count), int(algo), int(reduce_mode), dst))
        return outs


class GroupLloyd:
    """kmg_group_lloyd_*: one Lloyd problem -- or a BATCH of n_images problems, each image tiled over all ranks -- over row bands
    resident on the group's devices (modules.rs:763-840 + ONE RCCL all-reduce of the n_images x k x 4 int64 sums per iteration).
    Pointers are raw device addresses."""

    def __init__(self, group, k, n_images=1):
        self._g = group
        self.k = int(k)
        self.n_images = int(n_images)
        self._h = C.c_void_p()
        if self.n_images == 1:
            _check(lib().kmg_group_lloyd_create(group.handle, self.k, C.byref(self._h)))
        else:
            _check(lib().kmg_group_lloyd_create_batch(group.handle, self.k, self.n_images, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().kmg_group_lloyd_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def bind(self, d_rgba, row0, rows, width, height, d_labels=None, flags=0):
        n = self._g.n_local
        if not (len(d_rgba) == len(row0) == len(rows) == n):
            raise ValueError("one band per local device")
        px = (C.c_void_p * n)(*[int(p) or None for p in d_rgba])
        r0 = (C.c_uint32 * n)(*[int(v) for v in row0])
        rs = (C.c_uint32 * n)(*[int(v) for v in rows])
        lab = (C.c_void_p * n)(*[int(p) or None for p in d_labels]) if d_labels is not None else None
        _check(lib().kmg_group_lloyd_bind(self._h, px, r0, rs, int(width), int(height), lab, int(flags)))

    def bind_batch(self, d_rgba, row0, rows, widths, heights, d_labels=None, flags=0):
        """d_rgba / row0 / rows / d_labels: [image][local device]; widths / heights: per image (or one number for all)"""
        n, m = self._g.n_local, self.n_images
        if isinstance(widths, int):
            widths = [widths] * m
        if isinstance(heights, int):
            heights = [heights] * m
        flat = lambda a: [v for per_image in a for v in per_image]
        if not (len(d_rgba) == len(row0) == len(rows) == m) or any(len(x) != n for x in d_rgba):
            raise ValueError("one band per image and local device")
        px = (C.c_void_p * (n * m))(*[int(p) or None for p in flat(d_rgba)])
        r0 = (C.c_uint32 * (n * m))(*[int(v) for v in flat(row0)])
        rs = (C.c_uint32 * (n * m))(*[int(v) for v in flat(rows)])
        ws = (C.c_uint32 * m)(*[int(v) for v in widths])
        hs = (C.c_uint32 * m)(*[int(v) for v in heights])
        lab = (C.c_void_p * (n * m))(*[int(p) or None for p in flat(d_labels)]) if d_labels is not None else None
        _check(lib().kmg_group_lloyd_bind_batch(self._h, px, r0, rs, ws, hs, lab, int(flags)))

    def set_centroids(self, centroids4, image=None):
        c = np.ascontiguousarray(centroids4, np.float32).reshape(self.k, 4)
        if image is None:
            _check(lib().kmg_group_lloyd_set_centroids(self._h, _np_ptr(c)))
        else:
            _check(lib().kmg_group_lloyd_set_centroids_image(self._h, int(image), _np_ptr(c)))

    def get_centroids(self, image=None):
        out = np.empty((self.k, 4), np.float32)
        if image is None:
            _check(lib().kmg_group_lloyd_get_centroids(self._h, _np_ptr(out)))
        else:
            _check(lib().kmg_group_lloyd_get_centroids_image(self._h, int(image), _np_ptr(out)))
        return out

    def run_batch(self):
        """every image to its own convergence; the iteration each one stopped at"""
        its = (C.c_uint32 * self.n_images)()
        _check(lib().kmg_group_lloyd_run_batch(self._h, its))
        return [int(v) for v in its]

    def init(self):
        _check(lib().kmg_group_lloyd_init(self._h))

    def prime(self):
        _check(lib().kmg_group_lloyd_prime(self._h))

    def step(self):
        _check(lib().kmg_group_lloyd_step(self._h))

    def sync(self):
        _check(lib().kmg_group_lloyd_sync(self._h))

    def run(self):
        it = C.c_uint32()
        _check(lib().kmg_group_lloyd_run(self._h, C.byref(it)))
        return it.value

    def member(self, i=0):
        """(Lloyd of local device i, "table" | "scan")"""
        st = C.c_int()
        h = lib().kmg_group_lloyd_member(self._h, int(i), C.byref(st))
        return _BorrowedLloyd(h, self.k), ("table" if st.value == 1 else "scan")
