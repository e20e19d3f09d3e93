"""data-compressor_amd -- MI355X-native DEGA encode/decode (normalize -> diff -> seg -> bac adaptive) of
CenterForSecureEnergyInformatics/data-compressor, behind a C ABI.

This Python module is only the thin ctypes binding of `libdega_hip.so` (include/dega_hip.h) that tests/ and bench.py use
to drive the library with torch-owned device memory and streams.  The product is the shared library (HIP kernels in
csrc/) and the C host layer in host/ (plugin table mirror of DCLib/inc/enc_dec.h, DCCLI-style driver).

There is NO CPU fallback: if the library is missing, or no GPU is visible, calls raise / return the reference's
ERROR_LIBRARY_INIT (-10).

The directory name contains a hyphen, so import it with
    import importlib.util, sys
    spec = importlib.util.spec_from_file_location("data_compressor_amd", "<repo>/data-compressor_amd/__init__.py")
or simply `from __graft_entry__ import load_package; dca = load_package()`.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DEGA_HIP_LIB", os.path.join(HERE, "libdega_hip.so"))  # override: diagnostic builds only
HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "dega_hip.h")

OK = 0
ERROR_INVALID_VALUE = -1
ERROR_INVALID_FORMAT = -3
ERROR_MEMORY = -6
ERROR_LIBRARY_INIT = -10
ERROR_LIBRARY_CALL = -11

_P = C.c_void_p
_Z = C.c_size_t

_SIGNATURES = {
    "dega_hip_device_count": (C.c_int, []),
    "dega_hip_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "dega_hip_destroy": (None, [_P]),
    "dega_hip_last_error": (C.c_char_p, [_P]),
    "dega_hip_version": (C.c_char_p, []),
    "dega_hip_worst_case_bytes": (_Z, [_Z]),
    "dega_hip_encode_dev": (C.c_int, [_P, _P, _Z, _Z, _Z, C.c_int, C.c_int, _P, _Z, _P, _P, _P]),
    "dega_hip_decode_dev": (C.c_int, [_P, _P, _Z, _P, _Z, _Z, _Z, C.c_int, C.c_int, _P, _P, _P]),
    "dega_hip_decode_var_dev": (C.c_int, [_P, _P, _Z, _P, _Z, _Z, _Z, C.c_int, C.c_int, _P, _P, _P, _P]),
    "dega_hip_normalize_dev": (C.c_int, [_P, _P, _Z, _Z, _Z, C.c_float, C.c_int, _P, _P, _P]),
    "dega_hip_denormalize_dev": (C.c_int, [_P, _P, _Z, _Z, _Z, C.c_float, C.c_int, _P, _P]),
    "dega_hip_compact_offsets_dev": (C.c_int, [_P, _P, _Z, _P, _P]),
    "dega_hip_compact_gather_dev": (C.c_int, [_P, _P, _Z, _P, _Z, _P, _P]),
    "dega_hip_synth_dev": (C.c_int, [_P, _P, _Z, _Z, _Z, C.c_uint64, C.c_uint64, C.c_uint32, _P]),
    "dega_hip_encode_host": (C.c_int, [_P, _P, _Z, _Z, _Z, C.c_int, C.c_int, _P, _Z, _P, _P]),
    "dega_hip_encode_packed_host": (C.c_int, [_P, _P, _Z, _Z, _Z, C.c_int, C.c_int, _P, _Z, _P, _P, _P]),
    "dega_hip_decode_packed_host": (C.c_int, [_P, _P, _P, _P, _Z, _Z, _Z, C.c_int, C.c_int, _P, _P, _P]),
    "dega_hip_decode_host": (C.c_int, [_P, _P, _Z, _P, _Z, _Z, _Z, C.c_int, C.c_int, _P, _P]),
    "dega_hip_decode_var_host": (C.c_int, [_P, _P, _Z, _P, _Z, _Z, _Z, C.c_int, C.c_int, _P, _P, _P]),
    "dega_hip_encode_f32_host": (C.c_int, [_P, _P, _Z, _Z, _Z, C.c_float, C.c_int, C.c_int, _P, _Z, _P, _P]),
    "dega_hip_decode_f32_host": (C.c_int, [_P, _P, _Z, _P, _Z, _Z, _Z, C.c_float, C.c_int, C.c_int, _P, _P]),
    "dega_hip_decode_f32_var_host": (C.c_int, [_P, _P, _Z, _P, _Z, _Z, _Z, C.c_float, C.c_int, C.c_int, _P, _P, _P]),
    "dega_hip_worst_case_bytes64": (_Z, [_Z]),
    "dega_hip_encode64_dev": (C.c_int, [_P, _P, _Z, _Z, _Z, C.c_int, C.c_int, _P, _Z, _P, _P, _P]),
    "dega_hip_decode64_dev": (C.c_int, [_P, _P, _Z, _P, _Z, _Z, _Z, C.c_int, C.c_int, _P, _P, _P]),
    "dega_hip_decode64_var_dev": (C.c_int, [_P, _P, _Z, _P, _Z, _Z, _Z, C.c_int, C.c_int, _P, _P, _P, _P]),
    "dega_hip_encode64_host": (C.c_int, [_P, _P, _Z, _Z, _Z, C.c_int, C.c_int, _P, _Z, _P, _P]),
    "dega_hip_decode64_var_host": (C.c_int, [_P, _P, _Z, _P, _Z, _Z, _Z, C.c_int, C.c_int, _P, _P, _P]),
    "dega_hip_lzmh_worst_case_bytes": (_Z, [_Z]),
    "dega_hip_lzmh_encode_dev": (C.c_int, [_P, _P, _Z, _P, _Z, _P, _Z, _P, _P, _P]),
    "dega_hip_lzmh_decode_dev": (C.c_int, [_P, _P, _Z, _P, _Z, _P, _Z, _P, _P, _P]),
    "dega_hip_lzmh_render_dev": (C.c_int, [_P, _P, _Z, _Z, _Z, _P, _Z, _P, _P, _P]),
    "dega_hip_lzmh_encode_host": (C.c_int, [_P, _P, _Z, _P, _Z, _P, _Z, _P, _P]),
    "dega_hip_lzmh_decode_host": (C.c_int, [_P, _P, _Z, _P, _Z, _P, _Z, _P, _P]),
    "dega_hip_encode_f32_dev": (C.c_int, [_P, _P, _Z, _Z, _Z, C.c_float, C.c_int, C.c_int, _P, _Z, _P, _P, _P]),
    "dega_hip_decode_f32_dev": (C.c_int, [_P, _P, _Z, _P, _Z, _Z, _Z, C.c_float, C.c_int, C.c_int, _P, _P, _P, _P]),
    "dega_hip_encode_job_host": (C.c_int, [_P, _P, _P, _P, _Z, _P, _P, _P]),
    "dega_hip_decode_job_host": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "dega_hip_split_channels": (C.c_int, [_Z, C.c_int, _P]),
    "dega_hip_group_create": (C.c_int, [_P, C.c_int, C.POINTER(_P)]),
    "dega_hip_group_destroy": (None, [_P]),
    "dega_hip_group_size": (C.c_int, [_P]),
    "dega_hip_group_context": (_P, [_P, C.c_int]),
    "dega_hip_group_last_error": (C.c_char_p, [_P]),
    "dega_hip_group_encode": (C.c_int, [_P, _P, _P, _P, _Z, _P, _P, _P]),
    "dega_hip_group_decode": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "dega_hip_encode_state_bytes": (C.c_size_t, [C.c_size_t]),
    "dega_hip_encode_segment_dev": (C.c_int, [_P, _P, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, _P, C.c_size_t, _P, _P, _P, C.c_uint, _P]),
    "dega_hip_group_lzmh_encode": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_size_t, _P, C.c_size_t, _P, _P, _P]),
    "dega_hip_group_lzmh_decode": (C.c_int, [_P, _P, _P, _P, C.c_size_t, _P, C.c_size_t, _P, _P]),
    "dega_hip_pinned_alloc": (_P, [_Z]),
    "dega_hip_pinned_free": (None, [_P]),
    "dega_hip_aggregate_rows": (_Z, [_Z, _Z]),
    "dega_hip_aggregate_dev": (C.c_int, [_P, _P, _Z, _Z, _Z, _Z, _P, _Z, _P]),
    "dega_hip_aggregate_host": (C.c_int, [_P, _P, _Z, _Z, _Z, _Z, _P, _Z]),
    "dega_hip_encode_agg_f32_dev": (C.c_int, [_P, _P, _Z, _Z, _Z, _Z, C.c_float, C.c_int, C.c_int, _P, _Z, _P, _P, _P]),
    "dega_hip_encode_agg_job_host": (C.c_int, [_P, _P, _Z, _P, _P, _Z, _P, _P, _P]),
    "dega_hip_group_encode_agg": (C.c_int, [_P, _P, _Z, _P, _P, _Z, _P, _P, _P]),
    "dega_hip_aggregate_levels_plan": (C.c_int, [_Z, _Z, _P, _Z, C.c_int, _P, _P]),
    "dega_hip_aggregate_levels_dev": (C.c_int, [_P, _P, _Z, _Z, _Z, _P, _Z, _P, _P, _P]),
    "dega_hip_encode_levels_f32_dev": (C.c_int, [_P, _P, _Z, _Z, _Z, _P, _Z, C.c_float, C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    "dega_hip_encode_levels_job_host": (C.c_int, [_P, _P, _P, _Z, _P, _P, _P, _P, _P, _P]),
    "dega_hip_group_encode_levels": (C.c_int, [_P, _P, _P, _Z, _P, _P, _P, _P, _P, _P]),
    "dega_hip_csv_line_max": (_Z, [C.c_uint, _Z]),
    "dega_hip_csv_worst_case_bytes": (_Z, [_Z, C.c_uint, _Z]),
    "dega_hip_csv_write_dev": (C.c_int, [_P, _P, _Z, _Z, _Z, C.c_uint, _Z, C.c_int, _P, _Z, _P, _P, _P]),
    "dega_hip_csv_write_host": (C.c_int, [_P, _P, _Z, _Z, _Z, C.c_uint, _Z, C.c_int, _P, _Z, _P, _P]),
    "dega_hip_lzmh_encode_f32_dev": (C.c_int, [_P, _P, _Z, _Z, _Z, C.c_uint, _Z, C.c_int, _Z, _P, _Z, _P, _P, _P, _P]),
    "dega_hip_lzmh_encode_levels_f32_dev": (C.c_int, [_P, _P, _Z, _Z, _Z, _P, _Z, C.c_uint, _Z, C.c_int, _P, _P, _P, _P, _P, _P, _P]),
    "dega_hip_csv_read_dev": (C.c_int, [_P, _P, _Z, _P, _Z, _Z, C.c_int, _P, _Z, _Z, _P, _P, _P]),
    "dega_hip_csv_read_host": (C.c_int, [_P, _P, _Z, _P, _Z, _Z, C.c_int, _P, _Z, _Z, _P, _P]),
    "dega_hip_csv_read_split_dev": (C.c_int, [_P, _P, _Z, _P, _Z, _Z, C.c_int, _P, _Z, _Z, _P, _P, _Z, _P]),
    "dega_hip_csv_read_split_block_bytes": (_Z, [_Z, _Z]),
    "dega_hip_lzmh_decode_f32_dev": (C.c_int, [_P, _P, _Z, _P, _Z, _Z, _Z, C.c_int, _P, _Z, _Z, _P, _P, _P, _P]),
    "dega_hip_aggregate_levels_var_dev": (C.c_int, [_P, _P, _Z, _Z, _Z, _P, _P, _Z, _P, _P, _P, _P, _P]),
    "dega_hip_encode_f32_var_dev": (C.c_int, [_P, _P, _Z, _Z, _Z, _P, C.c_float, C.c_int, C.c_int, _P, _Z, _P, _P, _P]),
    "dega_hip_encode_levels_f32_var_dev": (C.c_int, [_P, _P, _Z, _Z, _Z, _P, _P, _Z, C.c_float, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P]),
    "dega_hip_csv_write_var_dev": (C.c_int, [_P, _P, _Z, _Z, _Z, _P, C.c_uint, _Z, C.c_int, _P, _Z, _P, _P, _P]),
    "dega_hip_csv_write_split_dev": (C.c_int, [_P, _P, _Z, _Z, _Z, _P, C.c_uint, _Z, C.c_int, _P, _Z, _P, _P, _Z, _P]),
    "dega_hip_csv_write_split_block_rows": (_Z, [_Z, _Z]),
    "dega_hip_lzmh_encode_levels_f32_var_dev": (C.c_int, [_P, _P, _Z, _Z, _Z, _P, _P, _Z, C.c_uint, _Z, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    "dega_hip_encode_var_dev": (C.c_int, [_P, _P, _Z, _Z, _Z, _P, C.c_int, C.c_int, C.c_int, _P, _Z, _P, _P, _P]),
    "dega_hip_encode64_var_dev": (C.c_int, [_P, _P, _Z, _Z, _Z, _P, C.c_int, C.c_int, _P, _Z, _P, _P, _P]),
    "dega_hip_encode_segment_var_dev": (C.c_int, [_P, _P, _Z, _Z, _Z, _P, _Z, _Z, C.c_int, C.c_int, _P, _Z, _P, _P, _P, C.c_uint, _P]),
    "dega_hip_encode_var_job_host": (C.c_int, [_P, _P, _P, _P, _P, _Z, _P, _P, _P]),
    "dega_hip_group_encode_var": (C.c_int, [_P, _P, _P, _P, _P, _Z, _P, _P, _P]),
    "dega_hip_to_time_major_dev": (C.c_int, [_P, _P, _Z, _Z, _Z, _Z, _P, _P, _Z, _P]),
    "dega_hip_to_channel_major_dev": (C.c_int, [_P, _P, _Z, _Z, _Z, _Z, _P, _P, _Z, _P]),
    "dega_hip_axdr_bytes": (_Z, [_Z, C.c_int]),
    "dega_hip_axdr_encode_dev": (C.c_int, [_P, _P, C.c_int, _Z, _Z, _Z, _P, C.c_float, C.c_int, _P, _Z, _P, _P, _P]),
    "dega_hip_axdr_decode_dev": (C.c_int, [_P, _P, _Z, _P, _Z, _Z, _Z, C.c_float, C.c_int, C.c_int, _P, _P, _P, _P]),
    "dega_hip_axdr_encode_levels_f32_dev": (C.c_int, [_P, _P, _Z, _Z, _Z, _P, _P, _Z, C.c_float, C.c_int, _P, _P, _P, _P, _P, _P]),
    "dega_hip_axdr_encode_host": (C.c_int, [_P, _P, C.c_int, _Z, _Z, _Z, _P, C.c_float, C.c_int, _P, _Z, _P, _P]),
    "dega_hip_axdr_decode_host": (C.c_int, [_P, _P, _Z, _P, _Z, _Z, _Z, C.c_float, C.c_int, C.c_int, _P, _P, _P]),
    "dega_hip_profile": (C.c_int, [_P, C.c_int]),
    "dega_hip_profile_read": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.c_int]),
}

SAMPLES_I32, SAMPLES_BE32, SAMPLES_I64, SAMPLES_F32 = 0, 1, 2, 3
SAMPLES_CHANNEL_MAJOR = 0x100  # DEGA_SAMPLES_CHANNEL_MAJOR: OR-ed into Job.samples by layout="channel"


class Job(C.Structure):
    """dega_hip_job of include/dega_hip.h"""
    _fields_ = [("C", _Z), ("T", _Z), ("ld", _Z), ("adaptive", C.c_int), ("valuesize", C.c_int), ("samples", C.c_int), ("factor", C.c_float)]


_lib = None


class DegaError(RuntimeError):
    def __init__(self, code, what):
        super().__init__("%s failed with code %d" % (what, code))
        self.code = code


def library():
    """Load libdega_hip.so (once).  torch is imported first when available so that both share one HIP runtime."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DegaError(ERROR_LIBRARY_INIT, "loading %s (not built: run __graft_entry__.build())" % LIB_PATH)
        try:
            import torch  # noqa: F401  (loads torch's libamdhip64 first; same SONAME, one runtime per process)
        except Exception:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def exported_symbols():
    return sorted(_SIGNATURES)


def worst_case_bytes(T):
    return library().dega_hip_worst_case_bytes(T)


def lzmh_worst_case_bytes(n):
    return library().dega_hip_lzmh_worst_case_bytes(n)


def axdr_bytes(T, valuesize):
    """The bytes of a slab that T fields of `valuesize` bits take, 4 * ceil(T * valuesize / 32) (dega_hip_axdr_bytes; no GPU
    needed); 0 for a value size outside 1..64."""
    return library().dega_hip_axdr_bytes(int(T), int(valuesize))


def csv_line_max(decimals=2, column=1):
    """The longest line `encode csv` can write (dega_hip_csv_line_max; no GPU needed); 0 for options out of range."""
    return library().dega_hip_csv_line_max(int(decimals), int(column))


def csv_worst_case_bytes(T, decimals=2, column=1):
    """A text stride that T readings can never overflow (dega_hip_csv_worst_case_bytes); 0 for options out of range."""
    return library().dega_hip_csv_worst_case_bytes(int(T), int(decimals), int(column))


def csv_read_split_block_bytes(C_, stride):
    """The block size csv_read(split="auto") takes for C_ channels of `stride` bytes (dega_hip_csv_read_split_block_bytes; no
    GPU needed); 0 for a stride the reader refuses."""
    return library().dega_hip_csv_read_split_block_bytes(int(C_), int(stride))


def csv_write_split_block_rows(C_, T):
    """The rows per block csv_write(split="auto") takes for C_ channels of T readings (dega_hip_csv_write_split_block_rows; no
    GPU needed); 0 for a T the counted form refuses."""
    return library().dega_hip_csv_write_split_block_rows(int(C_), int(T))


def _separator(separator_char):
    sep = ord(separator_char) if isinstance(separator_char, (str, bytes)) else int(separator_char)
    assert 0 <= sep <= 255, "separator_char is one byte"
    return sep


AGG_MAX_LEVELS = 8  # DEGA_AGG_MAX_LEVELS


def _level_array(levels):
    levels = [int(n) for n in levels]
    assert all(n >= 0 for n in levels), "num_values cannot be negative"
    return levels, (_Z * max(1, len(levels)))(*levels)


def _count_ptr(count, Cn, device):
    """count: int64 CUDA tensor of at least Cn entries (what csv_read, lzmh_decode_f32 and decode_f32(var=True) return)"""
    import torch
    assert count.dtype == torch.int64 and count.is_cuda and count.is_contiguous() and count.device == device and count.numel() >= Cn, \
        "count must be a contiguous int64 CUDA tensor with one entry per channel"
    return count.data_ptr()


def aggregate_levels_plan(C_, T, levels, wide=True):
    """Which levels share a pass over the base series (dega_hip_aggregate_levels_plan; no GPU needed).
    Returns (pass_of: list of K pass indices, step_of: list of base rows per range, one per pass)."""
    levels, nv = _level_array(levels)
    K = len(levels)
    pass_of = (C.c_int * max(1, K))()
    step_of = (_Z * max(1, K))()
    n = library().dega_hip_aggregate_levels_plan(int(C_), int(T), nv, K, 1 if wide else 0, pass_of, step_of)
    if n < 0:
        raise DegaError(n, "dega_hip_aggregate_levels_plan")
    return [int(pass_of[k]) for k in range(K)], [int(step_of[q]) for q in range(n)]


def _sample_dtype(samples):
    import numpy as np
    return {SAMPLES_I32: np.dtype(np.int32), SAMPLES_BE32: np.dtype(">i4"), SAMPLES_I64: np.dtype(np.int64), SAMPLES_F32: np.dtype(np.float32)}[samples]


def _host_layout(x, layout, samples, channels, T):
    """The assertions of a host job's sample array (as encode_segments makes them for its tensor: dtype, C-contiguity, shape)
    and what the job says about it: (C, T, ld, samples field).  layout "time": x is [T, ld], channels = its first `channels`
    columns; "channel": x is [C, ld], one series per row, T = the first T values of each (default: all ld)."""
    import numpy as np
    assert layout in ("time", "channel"), 'layout is "time" or "channel"'
    assert isinstance(x, np.ndarray) and x.ndim == 2 and x.flags.c_contiguous, "the samples must be a C-contiguous 2-d numpy array"
    assert x.dtype == _sample_dtype(samples), "the array's dtype must be the sample type's: nothing is converted behind the caller's back"
    if layout == "time":
        assert T is None or int(T) == x.shape[0], "T is the number of rows of a time-major array"
        Cn = x.shape[1] if channels is None else int(channels)
        assert 0 <= Cn <= x.shape[1], "channels must be at most the row pitch"
        return Cn, x.shape[0], x.shape[1], int(samples)
    Cn = x.shape[0] if channels is None else int(channels)
    Tn = x.shape[1] if T is None else int(T)
    assert 0 <= Cn <= x.shape[0], "channels must be at most the number of rows of a channel-major array"
    assert 0 <= Tn <= x.shape[1], "T must be at most the pitch between channels"
    return Cn, Tn, x.shape[1], int(samples) | SAMPLES_CHANNEL_MAJOR


class _JobCalls:
    """encode_job / decode_job on numpy arrays: the packed host-pointer surface, shared by Context (one device) and Group
    (every device).  Subclasses provide _enc_fn / _dec_fn / _handle / _check."""

    def encode_job(self, x_tc, adaptive=1, valuesize=32, samples=SAMPLES_I32, factor=100.0, packed_cap=None, channels=None, packed=None, num_values=1,
                   layout="time", T=None, count=None):
        """x_tc: [T, ld] array of the sample type (channels = the first `channels` columns, default all).
        Returns (packed uint8 [total], offsets uint64 [C+1], bits uint64 [C], err int32 [C]).
        num_values != 1 (float32 samples only): every num_values consecutive readings of a channel are summed on the
        device first, as the reference's `encode aggregate` does, and the ceil(T / num_values) sums are coded.
        layout="channel": the array is [C, ld] instead, one series per row (DEGA_SAMPLES_CHANNEL_MAJOR), T = the first T
        values of every row (default all); it goes up as it lies and is transposed on the device.  The array must then
        be C-contiguous and of the sample type (big-endian samples: dtype ">i4"); the results are those of the
        time-major call on its transpose.
        count (numpy uint64 array, one entry per channel: what decode_job(var=True) returns): a ragged batch -- channel c is
        coded from its first count[c] values and what lies behind them influences nothing (dega_hip_encode_var_job_host /
        dega_hip_group_encode_var).  Any sample type, both layouts; num_values must be 1.  The array is taken as it is,
        as for layout="channel": C-contiguous and of the sample type."""
        import numpy as np
        assert layout in ("time", "channel"), 'layout is "time" or "channel"'
        if count is not None:
            assert int(num_values) == 1, "a counted job codes the samples as they are: num_values must be 1"
            Cn, Tn, _, _ = dims = _host_layout(x_tc, layout, samples, channels, T)
            assert isinstance(count, np.ndarray) and count.dtype == np.uint64 and count.ndim == 1 and count.flags.c_contiguous, \
                "count must be a contiguous numpy uint64 array"
            assert count.size == Cn, "count has one entry per channel"
            assert packed is None or (isinstance(packed, np.ndarray) and packed.dtype == np.uint8 and packed.flags.c_contiguous and packed.ndim == 1)
            return self._encode_packed(self._enc_var_fn(), (count.ctypes.data,), "encode_job(count=, layout=%s)" % layout, x_tc, Tn, adaptive, valuesize,
                                       samples, factor, packed_cap, channels, packed, dims)
        if layout == "channel":
            Cn, Tn, _, _ = dims = _host_layout(x_tc, layout, samples, channels, T)
            num_values = int(num_values)
            assert num_values >= 0
            assert packed is None or (isinstance(packed, np.ndarray) and packed.dtype == np.uint8 and packed.flags.c_contiguous and packed.ndim == 1)
            if num_values != 1:
                rows = library().dega_hip_aggregate_rows(Tn, num_values)
                return self._encode_packed(self._enc_agg_fn(), (num_values,), "encode_job(num_values=%d, layout=channel)" % num_values, x_tc, rows,
                                           adaptive, valuesize, samples, factor, packed_cap, channels, packed, dims)
            return self._encode_packed(self._enc_fn(), (), "encode_job(layout=channel)", x_tc, Tn, adaptive, valuesize, samples, factor, packed_cap, channels,
                                       packed, dims)
        if num_values != 1:
            # the layout the library is told is the layout the array has: nothing is converted or copied behind the caller's back
            num_values = int(num_values)
            assert isinstance(x_tc, np.ndarray) and x_tc.ndim == 2 and x_tc.flags.c_contiguous, "x_tc must be a C-contiguous [T, ld] numpy array"
            assert samples != SAMPLES_F32 or x_tc.dtype == np.float32, "float32 samples need a float32 array"
            assert num_values >= 0
            assert channels is None or 0 <= int(channels) <= x_tc.shape[1], "channels must be at most the row pitch"
            assert packed is None or (isinstance(packed, np.ndarray) and packed.dtype == np.uint8 and packed.flags.c_contiguous and packed.ndim == 1)
            rows = library().dega_hip_aggregate_rows(x_tc.shape[0], num_values)
            return self._encode_packed(self._enc_agg_fn(), (num_values,), "encode_job(num_values=%d)" % num_values, x_tc, rows, adaptive, valuesize,
                                       samples, factor, packed_cap, channels, packed)
        if not (isinstance(x_tc, np.ndarray) and x_tc.flags.c_contiguous and x_tc.dtype == _sample_dtype(samples)):
            x_tc = np.ascontiguousarray(x_tc, dtype=_sample_dtype(samples))
        return self._encode_packed(self._enc_fn(), (), "encode_job", x_tc, x_tc.shape[0], adaptive, valuesize, samples, factor, packed_cap, channels, packed)

    def _encode_packed(self, fn, lead, what, x_tc, rows, adaptive, valuesize, samples, factor, packed_cap, channels, packed, dims=None):
        """fn(handle, job, *lead, samples, packed, packed_cap, offsets, bits, err) over x_tc as it is; `rows` values are coded
        per channel.  A packed_cap that was too small is replaced once by the size the library reports in offsets[C].
        dims: (C, T, ld, samples field) of _host_layout where the array is not [T, ld]."""
        import numpy as np
        if dims is None:
            T, pitch = x_tc.shape
            Cn = pitch if channels is None else int(channels)
            dims = (Cn, T, pitch, int(samples))
        Cn = dims[0]
        job = Job(dims[0], dims[1], dims[2], int(adaptive), int(valuesize), dims[3], float(factor))
        if packed_cap is None:
            packed_cap = Cn * (rows * 2 + 64)  # generous for meter data; the call says so if it is not
        offsets = np.zeros(Cn + 1, dtype=np.uint64)
        bits = np.zeros(Cn, dtype=np.uint64)
        err = np.zeros(Cn, dtype=np.int32)
        ret = OK
        for _ in range(2):
            buf = packed if packed is not None and packed.size >= packed_cap else np.empty(max(1, packed_cap), dtype=np.uint8)
            ret = fn(self._handle(), C.byref(job), *lead, x_tc.ctypes.data, buf.ctypes.data, packed_cap, offsets.ctypes.data, bits.ctypes.data, err.ctypes.data)
            if ret != ERROR_MEMORY or int(offsets[Cn]) <= packed_cap:
                break
            packed_cap = int(offsets[Cn])
        self._check(ret, what)
        return buf[: int(offsets[Cn])], offsets, bits, err

    def encode_job_levels(self, x_tc, levels, adaptive=1, valuesize=32, factor=100.0, packed_cap=None, channels=None, layout="time", T=None):
        """encode_job(..., samples=SAMPLES_F32, num_values=N) for every N of `levels` from ONE upload of x_tc (float32 numpy
        [T, ld]; dega_hip_encode_levels_job_host / dega_hip_group_encode_levels).  packed_cap: None, or one size per
        level.  Returns a list of (packed, offsets, bits, err), one per level in the order given.
        layout="channel": x_tc is float32 [C, ld], one series per row, as in encode_job."""
        import numpy as np
        assert isinstance(x_tc, np.ndarray) and x_tc.ndim == 2 and x_tc.flags.c_contiguous and x_tc.dtype == np.float32, \
            "x_tc must be a C-contiguous float32 [T, ld] (layout=\"channel\": [C, ld]) numpy array"
        levels, nv = _level_array(levels)
        K = len(levels)
        Cn, T, pitch, field = _host_layout(x_tc, layout, SAMPLES_F32, channels, T)
        job = Job(Cn, T, pitch, int(adaptive), int(valuesize), field, float(factor))
        rows = [library().dega_hip_aggregate_rows(T, n) for n in levels]
        caps = [Cn * (r * 2 + 64) for r in rows] if packed_cap is None else [int(c) for c in packed_cap]
        assert len(caps) == K, "one packed_cap per level"
        offsets = [np.zeros(Cn + 1, dtype=np.uint64) for _ in range(K)]
        bits = [np.zeros(Cn, dtype=np.uint64) for _ in range(K)]
        err = [np.zeros(Cn, dtype=np.int32) for _ in range(K)]
        ptrs = lambda arrs: (_P * max(1, K))(*[a.ctypes.data for a in arrs])  # noqa: E731
        ret, bufs = OK, []
        for _ in range(2):
            bufs = [np.empty(max(1, c), dtype=np.uint8) for c in caps]
            ret = self._enc_levels_fn()(self._handle(), C.byref(job), nv, K, x_tc.ctypes.data, ptrs(bufs), (_Z * max(1, K))(*caps), ptrs(offsets),
                                        ptrs(bits), ptrs(err))
            need = [int(offsets[k][Cn]) for k in range(K)]
            if ret != ERROR_MEMORY or packed_cap is not None or all(n <= c for n, c in zip(need, caps)):
                break
            caps = [max(n, c) for n, c in zip(need, caps)]
        self._check(ret, "encode_job_levels(%s)" % levels)
        return [(bufs[k][: int(offsets[k][Cn])], offsets[k], bits[k], err[k]) for k in range(K)]

    def decode_job(self, packed, offsets, bits, T, adaptive=1, valuesize=32, samples=SAMPLES_I32, factor=100.0, var=False, out=None, layout="time"):
        """The inverse.  Returns (x [T, C] of the sample type, err) or, with var=True, (x, counts, err).
        layout="channel": x is [C, T] instead (out: a C-contiguous [>= C, ld >= T] array of the sample type, whose padding
        is left alone; the whole array is returned); with var=True the values behind a channel's count are zero."""
        import numpy as np
        assert layout in ("time", "channel"), 'layout is "time" or "channel"'
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        bits = np.ascontiguousarray(bits, dtype=np.uint64)
        Cn = bits.size
        counts = np.zeros(Cn, dtype=np.uint64)
        err = np.zeros(Cn, dtype=np.int32)
        if layout == "channel":
            x = out if out is not None else np.zeros((Cn, T), dtype=_sample_dtype(samples))
            dims = _host_layout(x, layout, samples, Cn, T)
            job = Job(dims[0], dims[1], dims[2], int(adaptive), int(valuesize), dims[3], float(factor))
            ret = self._dec_fn()(self._handle(), C.byref(job), packed.ctypes.data, offsets.ctypes.data, bits.ctypes.data, x.ctypes.data,
                                 counts.ctypes.data if var else None, err.ctypes.data)
            self._check(ret, "decode_job(layout=channel)")
            return (x, counts, err) if var else (x, err)
        x = out if out is not None else np.zeros((T, Cn), dtype=_sample_dtype(samples))
        job = Job(Cn, T, x.shape[1] if x.ndim == 2 else Cn, int(adaptive), int(valuesize), int(samples), float(factor))
        ret = self._dec_fn()(self._handle(), C.byref(job), packed.ctypes.data, offsets.ctypes.data, bits.ctypes.data, x.ctypes.data,
                             counts.ctypes.data if var else None, err.ctypes.data)
        self._check(ret, "decode_job")
        return (x, counts, err) if var else (x, err)


class PinnedArray:
    """numpy view of pinned host memory (dega_hip_pinned_alloc): `.array`; `.free()` when done."""

    def __init__(self, shape, dtype):
        import numpy as np
        count = int(np.prod(shape))
        n = max(1, count * np.dtype(dtype).itemsize)
        self._p = library().dega_hip_pinned_alloc(n)
        if not self._p:
            raise DegaError(ERROR_MEMORY, "dega_hip_pinned_alloc(%d)" % n)
        self._buf = (C.c_uint8 * n).from_address(self._p)
        self.array = np.frombuffer(self._buf, dtype=dtype, count=count).reshape(shape)

    def free(self):
        if self._p:
            self.array = None
            self._buf = None
            library().dega_hip_pinned_free(self._p)
            self._p = None


class Group(_JobCalls):
    """dega_hip_group: every visible GPU (or `devices`), channel ranges per device, host-side concatenate."""

    def __init__(self, devices=None):
        self._h = _P()
        if devices:
            arr = (C.c_int * len(devices))(*devices)
            ret = library().dega_hip_group_create(arr, len(devices), C.byref(self._h))
        else:
            ret = library().dega_hip_group_create(None, 0, C.byref(self._h))
        if ret != OK:
            self._h = None
            raise DegaError(ret, "dega_hip_group_create")

    def size(self):
        return library().dega_hip_group_size(self._h)

    def close(self):
        if self._h:
            library().dega_hip_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        return self._h

    def _enc_fn(self):
        return library().dega_hip_group_encode

    def _dec_fn(self):
        return library().dega_hip_group_decode

    def _enc_var_fn(self):
        return library().dega_hip_group_encode_var

    def _enc_agg_fn(self):
        return library().dega_hip_group_encode_agg

    def _enc_levels_fn(self):
        return library().dega_hip_group_encode_levels

    def _check(self, ret, what):
        if ret != OK:
            raise DegaError(ret, "%s [%s]" % (what, library().dega_hip_group_last_error(self._h).decode()))

    def lzmh_encode_job(self, text, lens, packed=None):
        """text: uint8 [C, stride] host array (stride a multiple of 16; numpy or a PinnedArray's .array), lens: bytes per
        channel.  Returns (packed uint8, offsets uint64 [C + 1], bits uint64 [C], err int32 [C]); channel c's stream is
        packed[offsets[c]:offsets[c + 1]].  The host pipeline on every device of the group (dega_hip_group_lzmh_encode)."""
        import numpy as np
        Cn, stride = text.shape
        lens = np.ascontiguousarray(lens, dtype=np.uint64)
        if packed is None:
            packed = np.empty(int(lens.sum()) * 5 // 4 + 64 * Cn + 64, dtype=np.uint8)
        offsets = np.zeros(Cn + 1, dtype=np.uint64)
        bits = np.zeros(Cn, dtype=np.uint64)
        err = np.zeros(Cn, dtype=np.int32)
        ret = library().dega_hip_group_lzmh_encode(self._h, text.ctypes.data, stride, lens.ctypes.data, Cn, packed.ctypes.data, packed.size,
                                                   offsets.ctypes.data, bits.ctypes.data, err.ctypes.data)
        self._check(ret, "dega_hip_group_lzmh_encode")
        return packed, offsets, bits, err

    def lzmh_decode_job(self, packed, offsets, bits, stride, out=None):
        """The inverse: (text uint8 [C, stride], lens uint64 [C], err int32 [C])."""
        import numpy as np
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        bits = np.ascontiguousarray(bits, dtype=np.uint64)
        Cn = bits.size
        if out is None:
            out = np.zeros((Cn, stride), dtype=np.uint8)
        lens = np.zeros(Cn, dtype=np.uint64)
        err = np.zeros(Cn, dtype=np.int32)
        ret = library().dega_hip_group_lzmh_decode(self._h, packed.ctypes.data, offsets.ctypes.data, bits.ctypes.data, Cn, out.ctypes.data, stride,
                                                   lens.ctypes.data, err.ctypes.data)
        self._check(ret, "dega_hip_group_lzmh_decode")
        return out, lens, err


class Context(_JobCalls):
    """One device context (dega_hip_ctx).  Methods take torch CUDA tensors and enqueue on torch's current stream."""

    def _handle(self):
        return self._h

    def _enc_fn(self):
        return library().dega_hip_encode_job_host

    def _dec_fn(self):
        return library().dega_hip_decode_job_host

    def _enc_var_fn(self):
        return library().dega_hip_encode_var_job_host

    def _enc_agg_fn(self):
        return library().dega_hip_encode_agg_job_host

    def _enc_levels_fn(self):
        return library().dega_hip_encode_levels_job_host

    def __init__(self, device=0):
        self._h = _P()
        self.device = device
        ret = library().dega_hip_create(device, C.byref(self._h))
        if ret != OK:
            self._h = None
            raise DegaError(ret, "dega_hip_create(device=%d)" % device)

    def close(self):
        if self._h:
            library().dega_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return library().dega_hip_last_error(self._h).decode()

    def _check(self, ret, what):
        if ret != OK:
            raise DegaError(ret, "%s [%s]" % (what, self.last_error()))

    @staticmethod
    def _stream():
        import torch
        return _P(torch.cuda.current_stream().cuda_stream)

    # ---- device-resident API (torch tensors) ---------------------------------------------------------------------
    def encode(self, x_tc, adaptive=1, cap=None, out=None, bits=None, err=None, valuesize=32, count=None, channels=None, samples=SAMPLES_I32):
        """x_tc: int32 CUDA tensor [T, ld>=C].  Returns (out uint8 [C, cap], bits int64 [C] (bit lengths), err int32 [C]).
        count (int64 CUDA tensor, one per channel): a ragged batch -- channel c is coded from its first count[c] rows
        (dega_hip_encode_var_dev), valuesize 1..32; channels: the first `channels` columns of the rows (default all);
        samples: SAMPLES_I32, or SAMPLES_BE32 for byte-swapped words.  Returns (out, bits, err, counts) as encode_f32 does."""
        import torch
        T, ld = x_tc.shape
        Cn = ld
        assert x_tc.dtype == torch.int32 and x_tc.is_cuda and x_tc.is_contiguous()
        if count is not None:
            Cn = ld if channels is None else int(channels)
            assert 0 <= Cn <= ld, "channels must be at most the row pitch"
            if cap is None:
                cap = worst_case_bytes(T)
            out = torch.zeros((Cn, cap), dtype=torch.uint8, device=x_tc.device)
            bits = torch.zeros(Cn, dtype=torch.int64, device=x_tc.device)
            err = torch.zeros(Cn, dtype=torch.int32, device=x_tc.device)
            ret = library().dega_hip_encode_var_dev(self._h, x_tc.data_ptr(), Cn, T, ld, _count_ptr(count, Cn, x_tc.device), int(adaptive), int(valuesize),
                                                    int(samples), out.data_ptr(), cap, bits.data_ptr(), err.data_ptr(), self._stream())
            self._check(ret, "dega_hip_encode_var_dev")
            return out, bits, err, count
        assert channels is None and samples == SAMPLES_I32, "channels= and samples= go with count="
        if cap is None:
            cap = worst_case_bytes(T)
        if out is None:
            out = torch.zeros((Cn, cap), dtype=torch.uint8, device=x_tc.device)
        if bits is None:
            bits = torch.zeros(Cn, dtype=torch.int64, device=x_tc.device)
        if err is None:
            err = torch.zeros(Cn, dtype=torch.int32, device=x_tc.device)
        ret = library().dega_hip_encode_dev(self._h, x_tc.data_ptr(), Cn, T, ld, int(adaptive), int(valuesize), out.data_ptr(), cap,
                                            bits.data_ptr(), err.data_ptr(), self._stream())
        self._check(ret, "dega_hip_encode_dev")
        return out, bits, err

    def encode_segments(self, x_tc, cuts, adaptive=1, cap=None, valuesize=32, count=None):
        """The rows of x_tc ([T, C] int32 CUDA tensor) coded in ranges [cuts[k], cuts[k+1]), one launch each, the lanes' state
        kept in device memory in between (dega_hip_encode_segment_dev).  Returns (out, bits, err) of the whole channels.
        count (int64 CUDA tensor, one per channel): a ragged batch, every launch with row0 = cuts[k] and T_total = T
        (dega_hip_encode_segment_var_dev); the streams are those of encode(count=)."""
        import torch
        T, Cn = x_tc.shape
        assert x_tc.dtype == torch.int32 and x_tc.is_cuda and x_tc.is_contiguous() and cuts[0] == 0 and cuts[-1] == T
        count_ptr = None if count is None else _count_ptr(count, Cn, x_tc.device)
        if cap is None:
            cap = worst_case_bytes(T)
        out = torch.zeros((Cn, cap), dtype=torch.uint8, device=x_tc.device)
        bits = torch.zeros(Cn, dtype=torch.int64, device=x_tc.device)
        err = torch.zeros(Cn, dtype=torch.int32, device=x_tc.device)
        state = torch.zeros(library().dega_hip_encode_state_bytes(Cn), dtype=torch.uint8, device=x_tc.device)
        for k in range(len(cuts) - 1):
            flags = (1 if k > 0 else 0) | (2 if k + 2 < len(cuts) else 0)
            rows = x_tc[cuts[k]:cuts[k + 1]]
            ptr = rows.data_ptr() if cuts[k + 1] > cuts[k] else x_tc.data_ptr()
            if count is not None:
                ret = library().dega_hip_encode_segment_var_dev(self._h, ptr, Cn, cuts[k + 1] - cuts[k], Cn, count_ptr, cuts[k], T, int(adaptive),
                                                                int(valuesize), out.data_ptr(), cap, bits.data_ptr(), err.data_ptr(), state.data_ptr(),
                                                                flags, self._stream())
                self._check(ret, "dega_hip_encode_segment_var_dev")
                continue
            ret = library().dega_hip_encode_segment_dev(self._h, ptr, Cn, cuts[k + 1] - cuts[k], Cn, int(adaptive), int(valuesize), out.data_ptr(), cap,
                                                        bits.data_ptr(), err.data_ptr(), state.data_ptr(), flags, self._stream())
            self._check(ret, "dega_hip_encode_segment_dev")
        return out, bits, err

    def decode(self, streams, bits, T, adaptive=1, x_tc=None, err=None, valuesize=32):
        import torch
        Cn, cap = streams.shape
        assert streams.dtype == torch.uint8 and streams.is_cuda and streams.is_contiguous() and bits.dtype == torch.int64
        if x_tc is None:
            x_tc = torch.zeros((T, Cn), dtype=torch.int32, device=streams.device)
        if err is None:
            err = torch.zeros(Cn, dtype=torch.int32, device=streams.device)
        ret = library().dega_hip_decode_dev(self._h, streams.data_ptr(), cap, bits.data_ptr(), Cn, T, x_tc.shape[1], int(adaptive), int(valuesize),
                                            x_tc.data_ptr(), err.data_ptr(), self._stream())
        self._check(ret, "dega_hip_decode_dev")
        return x_tc, err

    @staticmethod
    def _layout_tensor(x, what):
        import torch
        assert isinstance(x, torch.Tensor) and x.dim() == 2 and x.is_cuda and x.is_contiguous() and x.element_size() in (4, 8), \
            "%s must be a contiguous 2-d CUDA tensor of 4- or 8-byte elements" % what

    def to_time_major(self, x_ct, T=None, count=None, ld=None, out=None):
        """x_ct: CUDA tensor [C, stride] of 4- or 8-byte elements, one series per row -> [T, C] with out[t, c] = x_ct[c, t]
        (dega_hip_to_time_major_dev; one kernel on the current stream).  T: the first T values of every row (default all).
        out (optional): a tensor [>= T, ld >= C] of the same dtype, or ld: the row pitch of a new one; columns C .. ld - 1
        are not written.  count (int64 CUDA tensor, one per channel): out[t, c] is zero bits for t >= count[c], whatever
        x_ct holds there.  Returns the [T, C] view of the destination."""
        import torch
        self._layout_tensor(x_ct, "x_ct")
        Cn, stride = x_ct.shape
        T = stride if T is None else int(T)
        assert 0 <= T <= stride, "T must be at most the pitch between channels"
        if out is None:
            out = torch.empty((T, Cn if ld is None else int(ld)), dtype=x_ct.dtype, device=x_ct.device)
        self._layout_tensor(out, "out")
        assert out.dtype == x_ct.dtype and out.device == x_ct.device and (ld is None or int(ld) == out.shape[1])
        assert out.shape[0] >= T and out.shape[1] >= Cn, "out must hold T rows of at least C columns"
        ret = library().dega_hip_to_time_major_dev(self._h, x_ct.data_ptr(), Cn, T, stride, x_ct.element_size(),
                                                   None if count is None else _count_ptr(count, Cn, x_ct.device), out.data_ptr(), out.shape[1], self._stream())
        self._check(ret, "dega_hip_to_time_major_dev")
        return out[:T, :Cn]

    def to_channel_major(self, x_tc, channels=None, count=None, stride=None, out=None):
        """The inverse: x_tc [T, ld] -> [C, T] with out[c, t] = x_tc[t, c] (dega_hip_to_channel_major_dev).  channels: the first
        `channels` columns (default all).  out (optional): a tensor [>= C, stride >= T], or stride: the pitch of a new one;
        values T .. stride - 1 of a row are not written.  count: out[c, t] is zero bits for t >= count[c].  Returns the
        [C, T] view of the destination."""
        import torch
        self._layout_tensor(x_tc, "x_tc")
        T, ld = x_tc.shape
        Cn = ld if channels is None else int(channels)
        assert 0 <= Cn <= ld, "channels must be at most the row pitch"
        if out is None:
            out = torch.empty((Cn, T if stride is None else int(stride)), dtype=x_tc.dtype, device=x_tc.device)
        self._layout_tensor(out, "out")
        assert out.dtype == x_tc.dtype and out.device == x_tc.device and (stride is None or int(stride) == out.shape[1])
        assert out.shape[0] >= Cn and out.shape[1] >= T, "out must hold C rows of at least T values"
        ret = library().dega_hip_to_channel_major_dev(self._h, x_tc.data_ptr(), Cn, T, ld, x_tc.element_size(),
                                                      None if count is None else _count_ptr(count, Cn, x_tc.device), out.data_ptr(), out.shape[1], self._stream())
        self._check(ret, "dega_hip_to_channel_major_dev")
        return out[:Cn, :T]

    def aggregate(self, v_tc, num_values, out=None, channels=None, count=None):
        """float32 CUDA tensor [T, ld] -> [ceil(T / num_values), ld_out]: every num_values consecutive readings of a channel
        summed from left to right in float32, bit for bit what the reference's `encode aggregate` writes
        (dega_hip_aggregate_dev).  channels = the first `channels` columns (default all, as encode_job).  `out` (optional)
        is a float32 CUDA tensor of that many rows and at least `channels` columns; columns beyond are left alone.
        count (int64 CUDA tensor, one per channel): a ragged batch, see aggregate_levels; returns (sums, counts, err)."""
        import torch
        if count is not None:
            sums, counts, err = self.aggregate_levels(v_tc, [num_values], channels=channels, out=None if out is None else [out], count=count)
            return sums[0], counts[0], err
        assert v_tc.dim() == 2 and v_tc.dtype == torch.float32 and v_tc.is_cuda and v_tc.is_contiguous()
        T, ld = v_tc.shape
        Cn = ld if channels is None else int(channels)
        assert 0 <= Cn <= ld, "channels must be at most the row pitch"
        T_out = library().dega_hip_aggregate_rows(T, int(num_values))
        if out is None:
            out = torch.empty((T_out, Cn), dtype=torch.float32, device=v_tc.device)
        assert out.dim() == 2 and out.dtype == torch.float32 and out.is_cuda and out.is_contiguous() and out.device == v_tc.device
        assert out.shape[0] >= T_out and out.shape[1] >= Cn, "out must hold ceil(T / num_values) rows of at least `channels` columns"
        ret = library().dega_hip_aggregate_dev(self._h, v_tc.data_ptr(), Cn, T, ld, int(num_values), out.data_ptr(), out.shape[1], self._stream())
        self._check(ret, "dega_hip_aggregate_dev")
        return out[:T_out]

    def aggregate_levels(self, v_tc, levels, channels=None, out=None, count=None):
        """aggregate(v_tc, N) for every N of `levels` from one pass over v_tc where the plan allows it
        (dega_hip_aggregate_levels_dev): a list of float32 CUDA tensors [ceil(T / N), channels], in the order given, each
        bit for bit what aggregate() gives alone.  `out` (optional): one float32 CUDA tensor per level, as in aggregate().
        count (int64 CUDA tensor, one per channel; what csv_read / lzmh_decode_f32 / decode_f32(var=True) return): a ragged
        batch (dega_hip_aggregate_levels_var_dev) -- channel c is its first count[c] rows, the rows behind them influence
        nothing.  Returns (sums, counts, err): counts[k] int64 [channels] = ceil(count / N_k), the rows of level k's
        column c that hold its sums (rows beyond are unspecified); err int32 [channels], ERROR_INVALID_VALUE where
        count[c] > T."""
        import torch
        assert v_tc.dim() == 2 and v_tc.dtype == torch.float32 and v_tc.is_cuda and v_tc.is_contiguous()
        levels, nv = _level_array(levels)
        K = len(levels)
        T, ld = v_tc.shape
        Cn = ld if channels is None else int(channels)
        assert 0 <= Cn <= ld, "channels must be at most the row pitch"
        rows = [library().dega_hip_aggregate_rows(T, n) for n in levels]
        if out is None:
            out = [torch.empty((r, Cn), dtype=torch.float32, device=v_tc.device) for r in rows]
        assert len(out) == K, "one output per level"
        for o, r in zip(out, rows):
            assert o.dim() == 2 and o.dtype == torch.float32 and o.is_cuda and o.is_contiguous() and o.device == v_tc.device
            assert o.shape[0] >= r and o.shape[1] >= Cn, "every out must hold ceil(T / num_values) rows of at least `channels` columns"
        if count is not None:
            counts = [torch.zeros(Cn, dtype=torch.int64, device=v_tc.device) for _ in range(K)]
            err = torch.zeros(Cn, dtype=torch.int32, device=v_tc.device)
            ret = library().dega_hip_aggregate_levels_var_dev(self._h, v_tc.data_ptr(), Cn, T, ld, _count_ptr(count, Cn, v_tc.device), nv, K,
                                                              (_P * max(1, K))(*[o.data_ptr() for o in out]), (_Z * max(1, K))(*[o.shape[1] for o in out]),
                                                              (_P * max(1, K))(*[t.data_ptr() for t in counts]), err.data_ptr(), self._stream())
            self._check(ret, "dega_hip_aggregate_levels_var_dev")
            return [o[:r] for o, r in zip(out, rows)], counts, err
        ret = library().dega_hip_aggregate_levels_dev(self._h, v_tc.data_ptr(), Cn, T, ld, nv, K, (_P * max(1, K))(*[o.data_ptr() for o in out]),
                                                      (_Z * max(1, K))(*[o.shape[1] for o in out]), self._stream())
        self._check(ret, "dega_hip_aggregate_levels_dev")
        return [o[:r] for o, r in zip(out, rows)]

    def encode_f32_levels(self, v_tc, levels, factor=100.0, adaptive=1, valuesize=32, cap=None, count=None):
        """encode_f32(v_tc, num_values=N) for every N of `levels` (dega_hip_encode_levels_f32_dev): the base series is read
        once per pass of the plan, then one encode launch per level on the same stream.  cap: None, or one per level.
        Returns a list of (out, bits, err), one per level in the order given.
        count (int64 CUDA tensor, one per channel): a ragged batch (dega_hip_encode_levels_f32_var_dev); the list then
        holds (out, bits, err, counts) with counts int64 [C] = ceil(count / N): what decode_f32 needs for that level."""
        import torch
        assert v_tc.dim() == 2 and v_tc.dtype == torch.float32 and v_tc.is_cuda and v_tc.is_contiguous()
        levels, nv = _level_array(levels)
        K = len(levels)
        T, Cn = v_tc.shape
        rows = [library().dega_hip_aggregate_rows(T, n) for n in levels]
        if cap is None:
            cap = [worst_case_bytes(r) if valuesize <= 32 else library().dega_hip_worst_case_bytes64(r) for r in rows]
        cap = [int(c) for c in cap]
        assert len(cap) == K, "one cap per level"
        out = [torch.zeros((Cn, c), dtype=torch.uint8, device=v_tc.device) for c in cap]
        bits = [torch.zeros(Cn, dtype=torch.int64, device=v_tc.device) for _ in range(K)]
        err = [torch.zeros(Cn, dtype=torch.int32, device=v_tc.device) for _ in range(K)]
        ptrs = lambda ts: (_P * max(1, K))(*[t.data_ptr() for t in ts])  # noqa: E731
        if count is not None:
            counts = [torch.zeros(Cn, dtype=torch.int64, device=v_tc.device) for _ in range(K)]
            ret = library().dega_hip_encode_levels_f32_var_dev(self._h, v_tc.data_ptr(), Cn, T, Cn, _count_ptr(count, Cn, v_tc.device), nv, K, float(factor),
                                                               int(adaptive), int(valuesize), ptrs(out), (_Z * max(1, K))(*cap), ptrs(bits), ptrs(counts),
                                                               ptrs(err), self._stream())
            self._check(ret, "dega_hip_encode_levels_f32_var_dev")
            return list(zip(out, bits, err, counts))
        ret = library().dega_hip_encode_levels_f32_dev(self._h, v_tc.data_ptr(), Cn, T, Cn, nv, K, float(factor), int(adaptive), int(valuesize),
                                                       ptrs(out), (_Z * max(1, K))(*cap), ptrs(bits), ptrs(err), self._stream())
        self._check(ret, "dega_hip_encode_levels_f32_dev")
        return list(zip(out, bits, err))

    def aggregate_host(self, v_tc, num_values, out=None, channels=None):
        """The same for a float32 numpy array [T, ld] in host memory (synchronous: upload, sum, download)."""
        import numpy as np
        assert isinstance(v_tc, np.ndarray) and v_tc.ndim == 2 and v_tc.dtype == np.float32 and v_tc.flags.c_contiguous
        T, ld = v_tc.shape
        Cn = ld if channels is None else int(channels)
        assert 0 <= Cn <= ld, "channels must be at most the row pitch"
        T_out = library().dega_hip_aggregate_rows(T, int(num_values))
        if out is None:
            out = np.empty((T_out, Cn), dtype=np.float32)
        assert isinstance(out, np.ndarray) and out.ndim == 2 and out.dtype == np.float32 and out.flags.c_contiguous
        assert out.shape[0] >= T_out and out.shape[1] >= Cn, "out must hold ceil(T / num_values) rows of at least `channels` columns"
        ret = library().dega_hip_aggregate_host(self._h, v_tc.ctypes.data, Cn, T, ld, int(num_values), out.ctypes.data, out.shape[1])
        self._check(ret, "dega_hip_aggregate_host")
        return out[:T_out]

    def encode_f32(self, v_tc, factor=100.0, adaptive=1, cap=None, valuesize=32, num_values=1, count=None):
        """float32 CUDA tensor [T, C] -> streams: Normalize fused into the encode kernel (one launch).
        num_values != 1: the readings are summed in groups of num_values first (dega_hip_encode_agg_f32_dev: the aggregate
        kernel, then the same encode over ceil(T / num_values) rows, on the same stream).
        count (int64 CUDA tensor, one per channel): a ragged batch -- channel c is coded from its first count[c] rows
        (dega_hip_encode_f32_var_dev; with num_values != 1 encode_f32_levels(count=...) with one level).  Returns
        (out, bits, err, counts), counts = the values coded per channel: what decode_f32 needs."""
        import torch
        T, Cn = v_tc.shape
        assert v_tc.dtype == torch.float32 and v_tc.is_cuda and v_tc.is_contiguous()
        if count is not None:
            if num_values != 1:
                return self.encode_f32_levels(v_tc, [num_values], factor, adaptive, valuesize, None if cap is None else [cap], count=count)[0]
            if cap is None:
                cap = worst_case_bytes(T) if valuesize <= 32 else library().dega_hip_worst_case_bytes64(T)
            out = torch.zeros((Cn, cap), dtype=torch.uint8, device=v_tc.device)
            bits = torch.zeros(Cn, dtype=torch.int64, device=v_tc.device)
            err = torch.zeros(Cn, dtype=torch.int32, device=v_tc.device)
            ret = library().dega_hip_encode_f32_var_dev(self._h, v_tc.data_ptr(), Cn, T, Cn, _count_ptr(count, Cn, v_tc.device), float(factor), int(adaptive),
                                                        int(valuesize), out.data_ptr(), cap, bits.data_ptr(), err.data_ptr(), self._stream())
            self._check(ret, "dega_hip_encode_f32_var_dev")
            return out, bits, err, count
        if num_values != 1:
            num_values = int(num_values)
            T_out = library().dega_hip_aggregate_rows(T, num_values)
            if cap is None:
                cap = worst_case_bytes(T_out) if valuesize <= 32 else library().dega_hip_worst_case_bytes64(T_out)
            out = torch.zeros((Cn, cap), dtype=torch.uint8, device=v_tc.device)
            bits = torch.zeros(Cn, dtype=torch.int64, device=v_tc.device)
            err = torch.zeros(Cn, dtype=torch.int32, device=v_tc.device)
            ret = library().dega_hip_encode_agg_f32_dev(self._h, v_tc.data_ptr(), Cn, T, Cn, num_values, float(factor), int(adaptive), int(valuesize),
                                                        out.data_ptr(), cap, bits.data_ptr(), err.data_ptr(), self._stream())
            self._check(ret, "dega_hip_encode_agg_f32_dev")
            return out, bits, err
        if cap is None:
            cap = worst_case_bytes(T) if valuesize <= 32 else library().dega_hip_worst_case_bytes64(T)
        out = torch.zeros((Cn, cap), dtype=torch.uint8, device=v_tc.device)
        bits = torch.zeros(Cn, dtype=torch.int64, device=v_tc.device)
        err = torch.zeros(Cn, dtype=torch.int32, device=v_tc.device)
        ret = library().dega_hip_encode_f32_dev(self._h, v_tc.data_ptr(), Cn, T, Cn, float(factor), int(adaptive), int(valuesize), out.data_ptr(), cap,
                                                bits.data_ptr(), err.data_ptr(), self._stream())
        self._check(ret, "dega_hip_encode_f32_dev")
        return out, bits, err

    def decode_f32(self, streams, bits, T, factor=100.0, adaptive=1, valuesize=32, var=False):
        """var=True: up to T values per channel; returns (v, counts int64 [C], err) -- what the count= keywords take"""
        import torch
        Cn, cap = streams.shape
        v = torch.zeros((T, Cn), dtype=torch.float32, device=streams.device)
        err = torch.zeros(Cn, dtype=torch.int32, device=streams.device)
        if var:
            counts = torch.zeros(Cn, dtype=torch.int64, device=streams.device)
            ret = library().dega_hip_decode_f32_dev(self._h, streams.data_ptr(), cap, bits.data_ptr(), Cn, T, Cn, float(factor), int(adaptive),
                                                    int(valuesize), v.data_ptr(), counts.data_ptr(), err.data_ptr(), self._stream())
            self._check(ret, "dega_hip_decode_f32_dev")
            return v, counts, err
        ret = library().dega_hip_decode_f32_dev(self._h, streams.data_ptr(), cap, bits.data_ptr(), Cn, T, Cn, float(factor), int(adaptive), int(valuesize),
                                                v.data_ptr(), None, err.data_ptr(), self._stream())
        self._check(ret, "dega_hip_decode_f32_dev")
        return v, err

    def normalize(self, v_tc, factor=100.0, valuesize=32):
        import torch
        T, Cn = v_tc.shape
        assert v_tc.dtype == torch.float32 and v_tc.is_cuda and v_tc.is_contiguous()
        x = torch.empty((T, Cn), dtype=torch.int32, device=v_tc.device)
        err = torch.zeros(Cn, dtype=torch.int32, device=v_tc.device)
        ret = library().dega_hip_normalize_dev(self._h, v_tc.data_ptr(), Cn, T, Cn, float(factor), int(valuesize), x.data_ptr(), err.data_ptr(), self._stream())
        self._check(ret, "dega_hip_normalize_dev")
        return x, err

    def denormalize(self, x_tc, factor=100.0, valuesize=32):
        import torch
        T, Cn = x_tc.shape
        v = torch.empty((T, Cn), dtype=torch.float32, device=x_tc.device)
        ret = library().dega_hip_denormalize_dev(self._h, x_tc.data_ptr(), Cn, T, Cn, float(factor), int(valuesize), v.data_ptr(), self._stream())
        self._check(ret, "dega_hip_denormalize_dev")
        return v

    def synth(self, C_, T, seed=1234, c0=0, S=50, device=None, out=None):
        import torch
        if out is None:
            out = torch.empty((T, C_), dtype=torch.int32, device=device or ("cuda:%d" % self.device))
        ret = library().dega_hip_synth_dev(self._h, out.data_ptr(), C_, T, out.shape[1], seed, c0, S, self._stream())
        self._check(ret, "dega_hip_synth_dev")
        return out

    def compact(self, streams, bits):
        """[C][cap] slabs -> (packed uint8 [total], offsets int64 [C+1])."""
        import torch
        Cn, cap = streams.shape
        offsets = torch.zeros(Cn + 1, dtype=torch.int64, device=streams.device)
        self._check(library().dega_hip_compact_offsets_dev(self._h, bits.data_ptr(), Cn, offsets.data_ptr(), self._stream()), "compact_offsets")
        total = int(offsets[-1].item())
        packed = torch.empty(max(total, 1), dtype=torch.uint8, device=streams.device)
        self._check(library().dega_hip_compact_gather_dev(self._h, streams.data_ptr(), cap, offsets.data_ptr(), Cn, packed.data_ptr(), self._stream()), "compact_gather")
        return packed[:total], offsets

    # ---- LZMH (BASELINE config 4) ---------------------------------------------------------------------------------
    def lzmh_encode(self, data, lens, cap=None, out=None, bits=None, err=None):
        """data: uint8 CUDA tensor [C, stride] (stride % 16 == 0), lens: int64 [C] bytes per channel.
        Returns (out uint8 [C, cap], bits int64 [C], err int32 [C])."""
        import torch
        Cn, stride = data.shape
        assert data.dtype == torch.uint8 and data.is_cuda and data.is_contiguous() and lens.dtype == torch.int64
        if cap is None:
            cap = lzmh_worst_case_bytes(stride)
        if out is None:
            out = torch.zeros((Cn, cap), dtype=torch.uint8, device=data.device)
        if bits is None:
            bits = torch.zeros(Cn, dtype=torch.int64, device=data.device)
        if err is None:
            err = torch.zeros(Cn, dtype=torch.int32, device=data.device)
        ret = library().dega_hip_lzmh_encode_dev(self._h, data.data_ptr(), stride, lens.data_ptr(), Cn, out.data_ptr(), cap,
                                                 bits.data_ptr(), err.data_ptr(), self._stream())
        self._check(ret, "dega_hip_lzmh_encode_dev")
        return out, bits, err

    def lzmh_decode(self, streams, bits, stride, out=None, lens=None, err=None):
        """streams: uint8 CUDA tensor [C, cap], bits int64 [C].  Returns (bytes uint8 [C, stride], lens int64 [C], err int32 [C])."""
        import torch
        Cn, cap = streams.shape
        assert streams.dtype == torch.uint8 and streams.is_cuda and streams.is_contiguous() and bits.dtype == torch.int64
        if out is None:
            out = torch.zeros((Cn, stride), dtype=torch.uint8, device=streams.device)
        if lens is None:
            lens = torch.zeros(Cn, dtype=torch.int64, device=streams.device)
        if err is None:
            err = torch.zeros(Cn, dtype=torch.int32, device=streams.device)
        ret = library().dega_hip_lzmh_decode_dev(self._h, streams.data_ptr(), cap, bits.data_ptr(), Cn, out.data_ptr(), stride,
                                                 lens.data_ptr(), err.data_ptr(), self._stream())
        self._check(ret, "dega_hip_lzmh_decode_dev")
        return out, lens, err

    def lzmh_render(self, x_tc, stride, out=None):
        """int32 channels [T, C] -> ASCII "%d.%02d\\n" lines per channel: (text uint8 [C, stride], lens int64 [C], err int32 [C])."""
        import torch
        T, Cn = x_tc.shape
        assert x_tc.dtype == torch.int32 and x_tc.is_cuda and x_tc.is_contiguous()
        if out is None:
            out = torch.zeros((Cn, stride), dtype=torch.uint8, device=x_tc.device)
        lens = torch.zeros(Cn, dtype=torch.int64, device=x_tc.device)
        err = torch.zeros(Cn, dtype=torch.int32, device=x_tc.device)
        ret = library().dega_hip_lzmh_render_dev(self._h, x_tc.data_ptr(), Cn, T, Cn, out.data_ptr(), stride, lens.data_ptr(),
                                                 err.data_ptr(), self._stream())
        self._check(ret, "dega_hip_lzmh_render_dev")
        return out, lens, err

    # ---- encode csv: float32 series as text, alone and in front of LZMH ------------------------------------------------
    def csv_write(self, v_tc, decimals=2, column=1, separator_char=",", stride=None, channels=None, out=None, count=None, split=None):
        """float32 CUDA tensor [T, ld] -> the reference's `encode csv` text per channel (dega_hip_csv_write_dev):
        (text uint8 [channels, stride], lens int64 [channels], err int32 [channels]).  stride (a multiple of 16) defaults
        to csv_worst_case_bytes; a channel whose text + 16 bytes does not fit it reports ERROR_MEMORY and length 0.
        count (int64 CUDA tensor, one per channel): a ragged batch (dega_hip_csv_write_var_dev) -- channel c's text is its
        first count[c] readings; count[c] > T reports ERROR_INVALID_VALUE and length 0.
        split: None is those calls; "auto" or a number of rows per block splits every channel's rows over lanes
        (dega_hip_csv_write_split_dev, with count as well; "auto" leaves the block to csv_write_split_block_rows) -- the same
        lens, err and bytes below lens, for batches of few long channels; bytes at or beyond lens[c] are then left untouched."""
        import torch
        assert v_tc.dim() == 2 and v_tc.dtype == torch.float32 and v_tc.is_cuda and v_tc.is_contiguous()
        T, ld = v_tc.shape
        Cn = ld if channels is None else int(channels)
        assert 0 <= Cn <= ld, "channels must be at most the row pitch"
        if stride is None:
            stride = csv_worst_case_bytes(T, decimals, column)
        stride = int(stride)
        if out is None:
            out = torch.zeros((Cn, stride), dtype=torch.uint8, device=v_tc.device)
        assert out.dim() == 2 and out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and out.device == v_tc.device
        assert out.shape[0] >= Cn and out.shape[1] == stride, "out must be [channels, stride]"
        lens = torch.zeros(Cn, dtype=torch.int64, device=v_tc.device)
        err = torch.zeros(Cn, dtype=torch.int32, device=v_tc.device)
        if split is not None:
            assert split == "auto" or (not isinstance(split, (str, bool)) and int(split) == split and split > 0), "split: None, \"auto\" or rows per block"
            ret = library().dega_hip_csv_write_split_dev(self._h, v_tc.data_ptr(), Cn, T, ld, None if count is None else _count_ptr(count, Cn, v_tc.device),
                                                         int(decimals), int(column), _separator(separator_char), out.data_ptr(), stride, lens.data_ptr(),
                                                         err.data_ptr(), 0 if split == "auto" else int(split), self._stream())
            self._check(ret, "dega_hip_csv_write_split_dev")
            return out[:Cn], lens, err
        if count is not None:
            ret = library().dega_hip_csv_write_var_dev(self._h, v_tc.data_ptr(), Cn, T, ld, _count_ptr(count, Cn, v_tc.device), int(decimals), int(column),
                                                       _separator(separator_char), out.data_ptr(), stride, lens.data_ptr(), err.data_ptr(), self._stream())
            self._check(ret, "dega_hip_csv_write_var_dev")
            return out[:Cn], lens, err
        ret = library().dega_hip_csv_write_dev(self._h, v_tc.data_ptr(), Cn, T, ld, int(decimals), int(column), _separator(separator_char),
                                               out.data_ptr(), stride, lens.data_ptr(), err.data_ptr(), self._stream())
        self._check(ret, "dega_hip_csv_write_dev")
        return out[:Cn], lens, err

    def csv_write_host(self, v_tc, decimals=2, column=1, separator_char=",", stride=None, channels=None):
        """The same for a float32 numpy array [T, ld] in host memory (synchronous: upload, render, download):
        (text uint8 [channels, stride], lens uint64 [channels], err int32 [channels])."""
        import numpy as np
        assert isinstance(v_tc, np.ndarray) and v_tc.ndim == 2 and v_tc.dtype == np.float32 and v_tc.flags.c_contiguous
        T, ld = v_tc.shape
        Cn = ld if channels is None else int(channels)
        assert 0 <= Cn <= ld, "channels must be at most the row pitch"
        if stride is None:
            stride = csv_worst_case_bytes(T, decimals, column)
        stride = int(stride)
        out = np.zeros((Cn, stride), dtype=np.uint8)
        lens = np.zeros(Cn, dtype=np.uint64)
        err = np.zeros(Cn, dtype=np.int32)
        ret = library().dega_hip_csv_write_host(self._h, v_tc.ctypes.data, Cn, T, ld, int(decimals), int(column), _separator(separator_char),
                                                out.ctypes.data, stride, lens.ctypes.data, err.ctypes.data)
        self._check(ret, "dega_hip_csv_write_host")
        return out, lens, err

    def lzmh_encode_f32(self, v_tc, text_stride, decimals=2, column=1, separator_char=",", cap=None, channels=None):
        """`encode csv # encode lzmh` per channel of a float32 CUDA tensor [T, ld] (dega_hip_lzmh_encode_f32_dev): the text
        stays in a scratch of the context, text_stride bytes per channel (a multiple of 16).
        Returns (out uint8 [channels, cap], bits int64, text_len int64, err int32)."""
        import torch
        assert v_tc.dim() == 2 and v_tc.dtype == torch.float32 and v_tc.is_cuda and v_tc.is_contiguous()
        T, ld = v_tc.shape
        Cn = ld if channels is None else int(channels)
        assert 0 <= Cn <= ld, "channels must be at most the row pitch"
        text_stride = int(text_stride)
        if cap is None:
            cap = lzmh_worst_case_bytes(text_stride)
        out = torch.zeros((Cn, cap), dtype=torch.uint8, device=v_tc.device)
        bits = torch.zeros(Cn, dtype=torch.int64, device=v_tc.device)
        text_len = torch.zeros(Cn, dtype=torch.int64, device=v_tc.device)
        err = torch.zeros(Cn, dtype=torch.int32, device=v_tc.device)
        ret = library().dega_hip_lzmh_encode_f32_dev(self._h, v_tc.data_ptr(), Cn, T, ld, int(decimals), int(column), _separator(separator_char),
                                                     text_stride, out.data_ptr(), cap, bits.data_ptr(), text_len.data_ptr(), err.data_ptr(), self._stream())
        self._check(ret, "dega_hip_lzmh_encode_f32_dev")
        return out, bits, text_len, err

    def lzmh_encode_levels_f32(self, v_tc, levels, text_stride, decimals=2, column=1, separator_char=",", cap=None, channels=None, count=None):
        """`encode aggregate num_values=N # encode csv # encode lzmh` for every N of `levels` (dega_hip_lzmh_encode_levels_f32_dev):
        the base series is read once per pass of the plan, then render + LZMH encode per level on the same stream.
        text_stride: one per level (or one for all); cap: None, or one per level.
        Returns a list of (out, bits, text_len, err), one per level in the order given.
        count (int64 CUDA tensor, one per channel): a ragged batch (dega_hip_lzmh_encode_levels_f32_var_dev); the list then
        holds (out, bits, text_len, err, counts), counts int64 [channels] = ceil(count / N)."""
        import torch
        assert v_tc.dim() == 2 and v_tc.dtype == torch.float32 and v_tc.is_cuda and v_tc.is_contiguous()
        levels, nv = _level_array(levels)
        K = len(levels)
        T, ld = v_tc.shape
        Cn = ld if channels is None else int(channels)
        assert 0 <= Cn <= ld, "channels must be at most the row pitch"
        strides = [int(text_stride)] * K if isinstance(text_stride, int) else [int(s) for s in text_stride]
        assert len(strides) == K, "one text_stride per level"
        cap = [lzmh_worst_case_bytes(s) for s in strides] if cap is None else [int(c) for c in cap]
        assert len(cap) == K, "one cap per level"
        out = [torch.zeros((Cn, c), dtype=torch.uint8, device=v_tc.device) for c in cap]
        bits = [torch.zeros(Cn, dtype=torch.int64, device=v_tc.device) for _ in range(K)]
        text_len = [torch.zeros(Cn, dtype=torch.int64, device=v_tc.device) for _ in range(K)]
        err = [torch.zeros(Cn, dtype=torch.int32, device=v_tc.device) for _ in range(K)]
        ptrs = lambda ts: (_P * max(1, K))(*[t.data_ptr() for t in ts])  # noqa: E731
        if count is not None:
            counts = [torch.zeros(Cn, dtype=torch.int64, device=v_tc.device) for _ in range(K)]
            ret = library().dega_hip_lzmh_encode_levels_f32_var_dev(self._h, v_tc.data_ptr(), Cn, T, ld, _count_ptr(count, Cn, v_tc.device), nv, K,
                                                                    int(decimals), int(column), _separator(separator_char), (_Z * max(1, K))(*strides),
                                                                    ptrs(out), (_Z * max(1, K))(*cap), ptrs(bits), ptrs(text_len), ptrs(counts), ptrs(err),
                                                                    self._stream())
            self._check(ret, "dega_hip_lzmh_encode_levels_f32_var_dev")
            return list(zip(out, bits, text_len, err, counts))
        ret = library().dega_hip_lzmh_encode_levels_f32_dev(self._h, v_tc.data_ptr(), Cn, T, ld, nv, K, int(decimals), int(column),
                                                            _separator(separator_char), (_Z * max(1, K))(*strides), ptrs(out), (_Z * max(1, K))(*cap),
                                                            ptrs(bits), ptrs(text_len), ptrs(err), self._stream())
        self._check(ret, "dega_hip_lzmh_encode_levels_f32_dev")
        return list(zip(out, bits, text_len, err))

    # ---- decode csv: text as float32 series, alone and behind LZMH -------------------------------------------------------
    def csv_read(self, text, lens, max_T, column=1, separator_char=",", channels=None, ld=None, out=None, split=None):
        """uint8 CUDA tensor [C, stride] with lens int64 [C] (what csv_write / lzmh_decode return) -> the reference's
        `decode csv` per channel (dega_hip_csv_read_dev): (v float32 [max_T, ld], count int64 [channels], err int32
        [channels]).  A channel with more than max_T values reports ERROR_MEMORY and the room it needs in count; one with
        a selected field of 48 characters or more ERROR_INVALID_FORMAT.  Rows beyond a channel's count are unspecified.
        split: None is that call; "auto" or a block size in bytes (a multiple of 16) splits every channel's text over lanes
        (dega_hip_csv_read_split_dev; "auto" leaves the block size to csv_read_split_block_bytes) -- the same results, for
        batches of few long channels."""
        import torch
        assert text.dim() == 2 and text.dtype == torch.uint8 and text.is_cuda and text.is_contiguous()
        assert lens.dtype == torch.int64 and lens.is_cuda and lens.is_contiguous() and lens.device == text.device
        stride = text.shape[1]
        Cn = text.shape[0] if channels is None else int(channels)
        assert 0 <= Cn <= text.shape[0] and lens.numel() >= Cn, "channels must be at most the rows of text"
        ld = Cn if ld is None else int(ld)
        max_T = int(max_T)
        if out is None:
            out = torch.zeros((max_T, ld), dtype=torch.float32, device=text.device)
        assert out.dim() == 2 and out.dtype == torch.float32 and out.is_cuda and out.is_contiguous() and out.device == text.device
        assert out.shape[0] >= max_T and out.shape[1] == ld, "out must be [max_T, ld]"
        count = torch.zeros(Cn, dtype=torch.int64, device=text.device)
        err = torch.zeros(Cn, dtype=torch.int32, device=text.device)
        if split is not None:
            assert split == "auto" or (not isinstance(split, (str, bool)) and int(split) == split and split > 0), "split: None, \"auto\" or a block size in bytes"
            ret = library().dega_hip_csv_read_split_dev(self._h, text.data_ptr(), stride, lens.data_ptr(), Cn, int(column), _separator(separator_char),
                                                        out.data_ptr(), max_T, ld, count.data_ptr(), err.data_ptr(), 0 if split == "auto" else int(split),
                                                        self._stream())
            self._check(ret, "dega_hip_csv_read_split_dev")
            return out, count, err
        ret = library().dega_hip_csv_read_dev(self._h, text.data_ptr(), stride, lens.data_ptr(), Cn, int(column), _separator(separator_char),
                                              out.data_ptr(), max_T, ld, count.data_ptr(), err.data_ptr(), self._stream())
        self._check(ret, "dega_hip_csv_read_dev")
        return out, count, err

    def csv_read_host(self, text, lens, max_T, column=1, separator_char=",", channels=None, ld=None):
        """The same for a uint8 numpy array [C, stride] in host memory (synchronous: upload, read, download):
        (v float32 [max_T, ld], count uint64 [channels], err int32 [channels])."""
        import numpy as np
        assert isinstance(text, np.ndarray) and text.ndim == 2 and text.dtype == np.uint8 and text.flags.c_contiguous
        lens = np.ascontiguousarray(lens, dtype=np.uint64)
        stride = text.shape[1]
        Cn = text.shape[0] if channels is None else int(channels)
        assert 0 <= Cn <= text.shape[0] and lens.size >= Cn, "channels must be at most the rows of text"
        ld = Cn if ld is None else int(ld)
        max_T = int(max_T)
        out = np.zeros((max_T, ld), dtype=np.float32)
        count = np.zeros(Cn, dtype=np.uint64)
        err = np.zeros(Cn, dtype=np.int32)
        ret = library().dega_hip_csv_read_host(self._h, text.ctypes.data, stride, lens.ctypes.data, Cn, int(column), _separator(separator_char),
                                               out.ctypes.data, max_T, ld, count.ctypes.data, err.ctypes.data)
        self._check(ret, "dega_hip_csv_read_host")
        return out, count, err

    def lzmh_decode_f32(self, streams, bits, text_stride, max_T, column=1, separator_char=",", channels=None, ld=None):
        """`decode lzmh # decode csv` per channel (dega_hip_lzmh_decode_f32_dev), the inverse of lzmh_encode_f32: streams
        uint8 CUDA tensor [C, cap], bits int64 [C]; the text stays in a scratch of the context, text_stride bytes per
        channel (a multiple of 16).  Returns (v float32 [max_T, ld], count int64, text_len int64, err int32); a channel
        whose text outgrows text_stride reports ERROR_MEMORY and count 0."""
        import torch
        assert streams.dim() == 2 and streams.dtype == torch.uint8 and streams.is_cuda and streams.is_contiguous()
        assert bits.dtype == torch.int64 and bits.is_cuda and bits.is_contiguous() and bits.device == streams.device
        cap = streams.shape[1]
        Cn = streams.shape[0] if channels is None else int(channels)
        assert 0 <= Cn <= streams.shape[0] and bits.numel() >= Cn, "channels must be at most the rows of streams"
        ld = Cn if ld is None else int(ld)
        max_T = int(max_T)
        out = torch.zeros((max_T, ld), dtype=torch.float32, device=streams.device)
        count = torch.zeros(Cn, dtype=torch.int64, device=streams.device)
        text_len = torch.zeros(Cn, dtype=torch.int64, device=streams.device)
        err = torch.zeros(Cn, dtype=torch.int32, device=streams.device)
        ret = library().dega_hip_lzmh_decode_f32_dev(self._h, streams.data_ptr(), cap, bits.data_ptr(), Cn, int(text_stride), int(column),
                                                     _separator(separator_char), out.data_ptr(), max_T, ld, count.data_ptr(), text_len.data_ptr(),
                                                     err.data_ptr(), self._stream())
        self._check(ret, "dega_hip_lzmh_decode_f32_dev")
        return out, count, text_len, err

    def lzmh_encode_host(self, strings, cap=None):
        """strings: list of bytes objects (one per channel).  Returns (out uint8 [C, cap], bits uint64 [C], err int32 [C])."""
        import numpy as np
        Cn = len(strings)
        stride = (max([len(s) for s in strings] + [1]) + 15) // 16 * 16
        data = np.zeros((Cn, stride), dtype=np.uint8)
        lens = np.zeros(Cn, dtype=np.uint64)
        for i, s in enumerate(strings):
            data[i, : len(s)] = np.frombuffer(s, dtype=np.uint8)
            lens[i] = len(s)
        if cap is None:
            cap = lzmh_worst_case_bytes(stride)
        out = np.zeros((Cn, cap), dtype=np.uint8)
        bits = np.zeros(Cn, dtype=np.uint64)
        err = np.zeros(Cn, dtype=np.int32)
        ret = library().dega_hip_lzmh_encode_host(self._h, data.ctypes.data, stride, lens.ctypes.data, Cn, out.ctypes.data, cap,
                                                  bits.ctypes.data, err.ctypes.data)
        self._check(ret, "dega_hip_lzmh_encode_host")
        return out, bits, err

    def lzmh_decode_host(self, streams, bits, stride):
        import numpy as np
        streams = np.ascontiguousarray(streams, dtype=np.uint8)
        bits = np.ascontiguousarray(bits, dtype=np.uint64)
        Cn, cap = streams.shape
        out = np.zeros((Cn, stride), dtype=np.uint8)
        lens = np.zeros(Cn, dtype=np.uint64)
        err = np.zeros(Cn, dtype=np.int32)
        ret = library().dega_hip_lzmh_decode_host(self._h, streams.ctypes.data, cap, bits.ctypes.data, Cn, out.ctypes.data, stride,
                                                  lens.ctypes.data, err.ctypes.data)
        self._check(ret, "dega_hip_lzmh_decode_host")
        return out, lens, err

    # ---- A-XDR: packed fields, the study's third chain ---------------------------------------------------------------
    @staticmethod
    def _axdr_torch_dtype(samples):
        import torch
        return {SAMPLES_I32: torch.int32, SAMPLES_I64: torch.int64, SAMPLES_F32: torch.float32}[samples]

    def axdr_encode(self, x_tc, valuesize, factor=100.0, samples=SAMPLES_F32, count=None, channels=None, cap=None, out=None):
        """x_tc: CUDA tensor [T, ld] of float32 readings (samples=SAMPLES_F32, valuesize 1..64), or of int32 (SAMPLES_I32, 1..32)
        / int64 (SAMPLES_I64, 33..64) containers of fields -> every channel's A-XDR stream, one big-endian field of `valuesize`
        bits per reading (dega_hip_axdr_encode_dev).  channels: the first `channels` columns (default all); count (int64 CUDA
        tensor, one per channel): channel c is its first count[c] rows; cap: bytes per slab (default axdr_bytes(T, valuesize));
        out (optional): a uint8 CUDA tensor [>= C, cap] -- only the streams' own bytes of it are written.
        Returns (slabs uint8 [C, cap], bits int64 [C], err int32 [C])."""
        import torch
        assert samples in (SAMPLES_F32, SAMPLES_I32, SAMPLES_I64), "samples is SAMPLES_F32, SAMPLES_I32 or SAMPLES_I64"
        assert x_tc.dim() == 2 and x_tc.dtype == self._axdr_torch_dtype(samples) and x_tc.is_cuda and x_tc.is_contiguous()
        T, ld = x_tc.shape
        Cn = ld if channels is None else int(channels)
        assert 0 <= Cn <= ld, "channels must be at most the row pitch"
        if out is not None:
            assert out.dim() == 2 and out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and out.device == x_tc.device and out.shape[0] >= Cn
            assert cap is None or int(cap) == out.shape[1]
            cap = out.shape[1]
        cap = axdr_bytes(T, valuesize) if cap is None else int(cap)
        if out is None:
            out = torch.zeros((Cn, cap), dtype=torch.uint8, device=x_tc.device)
        bits = torch.zeros(Cn, dtype=torch.int64, device=x_tc.device)
        err = torch.zeros(Cn, dtype=torch.int32, device=x_tc.device)
        ret = library().dega_hip_axdr_encode_dev(self._h, x_tc.data_ptr(), int(samples), Cn, T, ld, None if count is None else _count_ptr(count, Cn, x_tc.device),
                                                 float(factor), int(valuesize), out.data_ptr(), cap, bits.data_ptr(), err.data_ptr(), self._stream())
        self._check(ret, "dega_hip_axdr_encode_dev")
        return out[:Cn], bits, err

    def axdr_decode(self, streams, bits, max_T, valuesize, factor=100.0, samples=SAMPLES_F32, ld=None, out=None):
        """The inverse (dega_hip_axdr_decode_dev): streams uint8 CUDA tensor [C, cap], bits int64 [C] -> up to max_T fields per
        channel as float32 (sign-extended, divided by the factor), int32 or int64 (the field, zero above it).  out
        (optional): a tensor [>= max_T, ld >= C] of the samples' dtype, or ld: the row pitch of a new one.
        Returns (x_tc [max_T, C], count int64 [C], err int32 [C]); rows at or beyond a channel's count are not written."""
        import torch
        assert samples in (SAMPLES_F32, SAMPLES_I32, SAMPLES_I64), "samples is SAMPLES_F32, SAMPLES_I32 or SAMPLES_I64"
        assert streams.dim() == 2 and streams.dtype == torch.uint8 and streams.is_cuda and streams.is_contiguous()
        assert bits.dtype == torch.int64 and bits.is_cuda and bits.is_contiguous() and bits.device == streams.device and bits.numel() >= streams.shape[0]
        Cn, cap = streams.shape
        max_T = int(max_T)
        if out is None:
            out = torch.zeros((max_T, Cn if ld is None else int(ld)), dtype=self._axdr_torch_dtype(samples), device=streams.device)
        assert out.dim() == 2 and out.dtype == self._axdr_torch_dtype(samples) and out.is_cuda and out.is_contiguous() and out.device == streams.device
        assert out.shape[0] >= max_T and out.shape[1] >= Cn and (ld is None or int(ld) == out.shape[1]), "out must hold max_T rows of at least C columns"
        count = torch.zeros(Cn, dtype=torch.int64, device=streams.device)
        err = torch.zeros(Cn, dtype=torch.int32, device=streams.device)
        ret = library().dega_hip_axdr_decode_dev(self._h, streams.data_ptr(), cap, bits.data_ptr(), Cn, max_T, out.shape[1], float(factor), int(valuesize),
                                                 int(samples), out.data_ptr(), count.data_ptr(), err.data_ptr(), self._stream())
        self._check(ret, "dega_hip_axdr_decode_dev")
        return out[:max_T, :Cn], count, err

    def axdr_encode_levels_f32(self, v_tc, levels, valuesize, factor=100.0, count=None):
        """axdr_encode(aggregate(v_tc, N)) for every N of `levels` from one upload (dega_hip_axdr_encode_levels_f32_dev): the
        study's third chain at every granularity.  Returns a list of (slabs, bits, err), one per level in the order given;
        with count (int64 CUDA tensor, one per channel: what csv_read reports) of (slabs, bits, err, counts)."""
        import torch
        assert v_tc.dim() == 2 and v_tc.dtype == torch.float32 and v_tc.is_cuda and v_tc.is_contiguous()
        levels, nv = _level_array(levels)
        K = len(levels)
        T, Cn = v_tc.shape
        cap = [axdr_bytes(library().dega_hip_aggregate_rows(T, n), valuesize) for n in levels]
        out = [torch.zeros((Cn, c), dtype=torch.uint8, device=v_tc.device) for c in cap]
        bits = [torch.zeros(Cn, dtype=torch.int64, device=v_tc.device) for _ in range(K)]
        err = [torch.zeros(Cn, dtype=torch.int32, device=v_tc.device) for _ in range(K)]
        counts = [torch.zeros(Cn, dtype=torch.int64, device=v_tc.device) for _ in range(K)] if count is not None else None
        ptrs = lambda ts: (_P * max(1, K))(*[t.data_ptr() for t in ts])  # noqa: E731
        ret = library().dega_hip_axdr_encode_levels_f32_dev(self._h, v_tc.data_ptr(), Cn, T, Cn, None if count is None else _count_ptr(count, Cn, v_tc.device), nv, K,
                                                            float(factor), int(valuesize), ptrs(out), (_Z * max(1, K))(*cap), ptrs(bits),
                                                            None if counts is None else ptrs(counts), ptrs(err), self._stream())
        self._check(ret, "dega_hip_axdr_encode_levels_f32_dev")
        return list(zip(out, bits, err)) if counts is None else list(zip(out, bits, err, counts))

    def axdr_encode_host(self, x_tc, valuesize, factor=100.0, samples=SAMPLES_F32, count=None, channels=None, cap=None, out=None):
        """axdr_encode for a numpy array [T, ld] in host memory (dega_hip_axdr_encode_host; synchronous, chunks of channels).
        count: uint64, one per channel.  Returns (slabs uint8 [C, cap], bits uint64 [C], err int32 [C])."""
        import numpy as np
        assert samples in (SAMPLES_F32, SAMPLES_I32, SAMPLES_I64), "samples is SAMPLES_F32, SAMPLES_I32 or SAMPLES_I64"
        assert isinstance(x_tc, np.ndarray) and x_tc.ndim == 2 and x_tc.flags.c_contiguous, "the samples must be a C-contiguous 2-d numpy array"
        assert x_tc.dtype == _sample_dtype(samples), "the array's dtype must be the sample type's: nothing is converted behind the caller's back"
        T, ld = x_tc.shape
        Cn = ld if channels is None else int(channels)
        assert 0 <= Cn <= ld, "channels must be at most the row pitch"
        if count is not None:
            count = np.ascontiguousarray(count, dtype=np.uint64)
            assert count.size >= Cn, "one count per channel"
        if out is not None:
            assert isinstance(out, np.ndarray) and out.ndim == 2 and out.dtype == np.uint8 and out.flags.c_contiguous and out.shape[0] >= Cn
            assert cap is None or int(cap) == out.shape[1]
            cap = out.shape[1]
        cap = axdr_bytes(T, valuesize) if cap is None else int(cap)
        if out is None:
            out = np.zeros((Cn, cap), dtype=np.uint8)
        bits = np.zeros(Cn, dtype=np.uint64)
        err = np.zeros(Cn, dtype=np.int32)
        ret = library().dega_hip_axdr_encode_host(self._h, x_tc.ctypes.data, int(samples), Cn, T, ld, None if count is None else count.ctypes.data, float(factor),
                                                  int(valuesize), out.ctypes.data, cap, bits.ctypes.data, err.ctypes.data)
        self._check(ret, "dega_hip_axdr_encode_host")
        return out[:Cn], bits, err

    def axdr_decode_host(self, streams, bits, max_T, valuesize, factor=100.0, samples=SAMPLES_F32, ld=None, out=None):
        """axdr_decode for numpy arrays in host memory (dega_hip_axdr_decode_host; synchronous, chunks of channels).
        Returns (x_tc [max_T, C], count uint64 [C], err int32 [C])."""
        import numpy as np
        assert samples in (SAMPLES_F32, SAMPLES_I32, SAMPLES_I64), "samples is SAMPLES_F32, SAMPLES_I32 or SAMPLES_I64"
        assert isinstance(streams, np.ndarray) and streams.ndim == 2 and streams.dtype == np.uint8 and streams.flags.c_contiguous
        bits = np.ascontiguousarray(bits, dtype=np.uint64)
        Cn, cap = streams.shape
        assert bits.size == Cn, "one bit length per channel"
        max_T = int(max_T)
        if out is None:
            out = np.zeros((max_T, Cn if ld is None else int(ld)), dtype=_sample_dtype(samples))
        assert isinstance(out, np.ndarray) and out.ndim == 2 and out.dtype == _sample_dtype(samples) and out.flags.c_contiguous
        assert out.shape[0] >= max_T and out.shape[1] >= Cn and (ld is None or int(ld) == out.shape[1]), "out must hold max_T rows of at least C columns"
        count = np.zeros(Cn, dtype=np.uint64)
        err = np.zeros(Cn, dtype=np.int32)
        ret = library().dega_hip_axdr_decode_host(self._h, streams.ctypes.data, cap, bits.ctypes.data, Cn, max_T, out.shape[1], float(factor), int(valuesize),
                                                  int(samples), out.ctypes.data, count.ctypes.data, err.ctypes.data)
        self._check(ret, "dega_hip_axdr_decode_host")
        return out[:max_T, :Cn], count, err

    def profile(self, enable=True):
        library().dega_hip_profile(self._h, 1 if enable else 0)

    def profile_read(self, which=0, reset=True):
        avg = C.c_double(0.0)
        n = library().dega_hip_profile_read(self._h, which, C.byref(avg), 1 if reset else 0)
        return n, avg.value

    # ---- host-pointer API (numpy) ---------------------------------------------------------------------------------
    def encode_host(self, x_tc, adaptive=1, cap=None, valuesize=32):
        import numpy as np
        x_tc = np.ascontiguousarray(x_tc, dtype=np.int32)
        T, Cn = x_tc.shape
        if cap is None:
            cap = worst_case_bytes(T)
        out = np.zeros((Cn, cap), dtype=np.uint8)
        bits = np.zeros(Cn, dtype=np.uint64)
        err = np.zeros(Cn, dtype=np.int32)
        ret = library().dega_hip_encode_host(self._h, x_tc.ctypes.data, Cn, T, Cn, int(adaptive), int(valuesize), out.ctypes.data, cap, bits.ctypes.data, err.ctypes.data)
        self._check(ret, "dega_hip_encode_host")
        return out, bits, err

    def encode_packed_host(self, x_tc, adaptive=1, valuesize=32, packed_cap=None):
        """Streams returned packed: (packed uint8 [total], offsets uint64 [C+1], bits uint64 [C], err int32 [C])."""
        import numpy as np
        x_tc = np.ascontiguousarray(x_tc, dtype=np.int32)
        T, Cn = x_tc.shape
        if packed_cap is None:
            packed_cap = Cn * (T * 2 + 64)  # 2 bytes per sample: generous for meter data; the call says so if it is not
        offsets = np.zeros(Cn + 1, dtype=np.uint64)
        bits = np.zeros(Cn, dtype=np.uint64)
        err = np.zeros(Cn, dtype=np.int32)
        for _ in range(2):
            packed = np.empty(max(1, packed_cap), dtype=np.uint8)
            ret = library().dega_hip_encode_packed_host(self._h, x_tc.ctypes.data, Cn, T, Cn, int(adaptive), int(valuesize), packed.ctypes.data,
                                                        packed_cap, offsets.ctypes.data, bits.ctypes.data, err.ctypes.data)
            if ret != ERROR_MEMORY or int(offsets[Cn]) <= packed_cap:
                break
            packed_cap = int(offsets[Cn])
        self._check(ret, "dega_hip_encode_packed_host")
        return packed[: int(offsets[Cn])], offsets, bits, err

    def decode_packed_host(self, packed, offsets, bits, T, adaptive=1, valuesize=32, var=False):
        """The inverse of encode_packed_host.  Returns (x int32 [T, C], err) or, with var=True, (x, counts, err)."""
        import numpy as np
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        bits = np.ascontiguousarray(bits, dtype=np.uint64)
        Cn = bits.size
        x = np.zeros((T, Cn), dtype=np.int32)
        counts = np.zeros(Cn, dtype=np.uint64)
        err = np.zeros(Cn, dtype=np.int32)
        ret = library().dega_hip_decode_packed_host(self._h, packed.ctypes.data, offsets.ctypes.data, bits.ctypes.data, Cn, T, Cn, int(adaptive),
                                                    int(valuesize), x.ctypes.data, counts.ctypes.data if var else None, err.ctypes.data)
        self._check(ret, "dega_hip_decode_packed_host")
        return (x, counts, err) if var else (x, err)

    def decode_host(self, streams, bits, T, adaptive=1, valuesize=32):
        import numpy as np
        streams = np.ascontiguousarray(streams, dtype=np.uint8)
        bits = np.ascontiguousarray(bits, dtype=np.uint64)
        Cn, cap = streams.shape
        x = np.zeros((T, Cn), dtype=np.int32)
        err = np.zeros(Cn, dtype=np.int32)
        ret = library().dega_hip_decode_host(self._h, streams.ctypes.data, cap, bits.ctypes.data, Cn, T, Cn, int(adaptive), int(valuesize), x.ctypes.data, err.ctypes.data)
        self._check(ret, "dega_hip_decode_host")
        return x, err

    def decode_var_host(self, streams, bits, max_T, adaptive=1, valuesize=32):
        """Decode streams of unknown length: returns (x [max_T, C], counts uint64 [C], err)."""
        import numpy as np
        streams = np.ascontiguousarray(streams, dtype=np.uint8)
        bits = np.ascontiguousarray(bits, dtype=np.uint64)
        Cn, cap = streams.shape
        x = np.zeros((max_T, Cn), dtype=np.int32)
        counts = np.zeros(Cn, dtype=np.uint64)
        err = np.zeros(Cn, dtype=np.int32)
        ret = library().dega_hip_decode_var_host(self._h, streams.ctypes.data, cap, bits.ctypes.data, Cn, max_T, Cn, int(adaptive), int(valuesize),
                                                 x.ctypes.data, counts.ctypes.data, err.ctypes.data)
        self._check(ret, "dega_hip_decode_var_host")
        return x, counts, err

    def encode64_host(self, x_tc, valuesize, adaptive=1, cap=None):
        """valuesize 33..64: x_tc int64 [T, C] (the low valuesize bits count)."""
        import numpy as np
        x_tc = np.ascontiguousarray(x_tc, dtype=np.int64)
        T, Cn = x_tc.shape
        if cap is None:
            cap = library().dega_hip_worst_case_bytes64(T)
        out = np.zeros((Cn, cap), dtype=np.uint8)
        bits = np.zeros(Cn, dtype=np.uint64)
        err = np.zeros(Cn, dtype=np.int32)
        ret = library().dega_hip_encode64_host(self._h, x_tc.ctypes.data, Cn, T, Cn, int(adaptive), int(valuesize), out.ctypes.data, cap,
                                               bits.ctypes.data, err.ctypes.data)
        self._check(ret, "dega_hip_encode64_host")
        return out, bits, err

    def decode64_var_host(self, streams, bits, max_T, valuesize, adaptive=1):
        import numpy as np
        streams = np.ascontiguousarray(streams, dtype=np.uint8)
        bits = np.ascontiguousarray(bits, dtype=np.uint64)
        Cn, cap = streams.shape
        x = np.zeros((max_T, Cn), dtype=np.int64)
        counts = np.zeros(Cn, dtype=np.uint64)
        err = np.zeros(Cn, dtype=np.int32)
        ret = library().dega_hip_decode64_var_host(self._h, streams.ctypes.data, cap, bits.ctypes.data, Cn, max_T, Cn, int(adaptive), int(valuesize),
                                                   x.ctypes.data, counts.ctypes.data, err.ctypes.data)
        self._check(ret, "dega_hip_decode64_var_host")
        return x, counts, err

    def encode_f32_host(self, v_tc, factor=100.0, adaptive=1, cap=None, valuesize=32):
        import numpy as np
        v_tc = np.ascontiguousarray(v_tc, dtype=np.float32)
        T, Cn = v_tc.shape
        if cap is None:
            cap = worst_case_bytes(T) if valuesize <= 32 else library().dega_hip_worst_case_bytes64(T)
        out = np.zeros((Cn, cap), dtype=np.uint8)
        bits = np.zeros(Cn, dtype=np.uint64)
        err = np.zeros(Cn, dtype=np.int32)
        ret = library().dega_hip_encode_f32_host(self._h, v_tc.ctypes.data, Cn, T, Cn, float(factor), int(adaptive), int(valuesize), out.ctypes.data, cap, bits.ctypes.data, err.ctypes.data)
        self._check(ret, "dega_hip_encode_f32_host")
        return out, bits, err

    def decode_f32_host(self, streams, bits, T, factor=100.0, adaptive=1, valuesize=32):
        import numpy as np
        streams = np.ascontiguousarray(streams, dtype=np.uint8)
        bits = np.ascontiguousarray(bits, dtype=np.uint64)
        Cn, cap = streams.shape
        v = np.zeros((T, Cn), dtype=np.float32)
        err = np.zeros(Cn, dtype=np.int32)
        ret = library().dega_hip_decode_f32_host(self._h, streams.ctypes.data, cap, bits.ctypes.data, Cn, T, Cn, float(factor), int(adaptive), int(valuesize), v.ctypes.data, err.ctypes.data)
        self._check(ret, "dega_hip_decode_f32_host")
        return v, err


def synth_reference(C_, T, seed=1234, c0=0, S=50):
    """numpy restatement of dega_synth_kernel (csrc/dega_kernels.hpp) -- the workload definition of SURVEY.md 8d."""
    import numpy as np
    M = (1 << 64) - 1

    def mix(z):
        z = (z + 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    x = np.zeros((T, C_), dtype=np.int32)
    for c in range(C_):
        key = mix((seed ^ (((c0 + c) * 0xD1342543DE82EF95) & M)) & M)
        v = 10000 + mix(key) % 50000
        for t in range(T):
            if t > 0:
                v += mix((key + t) & M) % (2 * S + 1) - S
                v = min(max(v, 0), 2**31 - 1)
            x[t, c] = v
    return x
