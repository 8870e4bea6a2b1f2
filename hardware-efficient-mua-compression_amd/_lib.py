"""ctypes binding of libmuahuff.so (include/muahuff.h).  Fails loudly: there is no CPU path."""
import ctypes as ct
import os

from ._loader import HERE, MH_OK, Library, MuaHuffError, _int, _u32, _u64, _vp  # noqa: F401

SO = os.path.join(HERE, "libmuahuff.so")

ERR_ARG, ERR_EMPTY_CHANNEL, ERR_SCLV, ERR_CAPACITY, ERR_HIP, ERR_NO_DEVICE, ERR_STREAM = -1, -2, -3, -4, -5, -6, -7

MODE_NOSORT, MODE_APPROX = 0, 1
WIN_REF_HALF, WIN_REF_HALF_TRUNC, WIN_AFTER_CAL, WIN_FULL = 0, 1, 2, 3
WIN_REV2_SEGMENTS = 0x100  # OR-ed into a window rule: the segment directory of container format revision 2 (no head segments)

PIECE, LANES, ROWS = 16, 64, 16
SUB = PIECE * ROWS
CHUNK = SUB * LANES
HDR_WORDS = LANES // 2


class PlanInfo(ct.Structure):
    _fields_ = [(n, ct.c_uint32) for n in ("C", "S", "h", "mode", "window", "K", "seg_chunks", "maxlen")] + \
               [(n, ct.c_uint64) for n in ("n_segments", "payload_cap_words", "window_samples", "n_skipped")]


# every symbol include/muahuff.h declares, with its prototype
PROTOTYPES = {
    "mh_version": (_int, []),
    "mh_last_error": (ct.c_char_p, []),
    "mh_device_info": (_int, [_int, ct.POINTER(_int), ct.POINTER(_u64), ct.c_char_p, _int, ct.c_char_p, _int]),
    "mh_codebook": (_int, [_vp, _int, _vp, _vp]),
    "mh_approx_sort_perm": (_int, [_int, _int, _vp]),
    "mh_plan_create": (_int, [ct.POINTER(_vp), _vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _u32, _u32]),
    "mh_plan_create_packed": (_int, [ct.POINTER(_vp), _vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _u32, _u32, _u32, _u64]),
    "mh_plan_destroy": (_int, [_vp]),
    "mh_plan_info": (_int, [_vp, ct.POINTER(PlanInfo)]),
    "mh_plan_segments": (_int, [_vp, _vp, _vp, _vp, _vp]),
    "mh_measure": (_int, [_vp] * 10),
    "mh_encode": (_int, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mh_encode_preset": (_int, [_vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "mh_plan_query": (_int, [_vp, _u32, _u32, _u32, _u32, _u32, _vp, _u32, _u32, ct.POINTER(PlanInfo), _vp, _vp, _vp, _vp, _u64]),
    "mh_decode": (_int, [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "mh_decode_packed": (_int, [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "mh_decode_status": (_int, [_vp, ct.POINTER(_u32), _vp]),
    "mh_validate_stream": (_int, [_vp, _u32, _u32, _u32, _u32, _u32, _vp, _u32, _u32, _vp, _u64, _vp, _u64, _vp, _vp]),
    "mh_decode_range": (_int, [_vp, _vp, _u64, _vp, _vp, _u32, _u64, _u64, _vp, _vp, _vp, _u64, _vp]),
    "mh_decode_rebin": (_int, [_vp, _vp, _u64, _vp, _vp, _u32, _u64, _u64, _u32, _int, _vp, _vp, _vp, _u64, _vp]),
    "mh_validate_segments": (_int, [_vp, _u32, _u32, _u32, _u32, _u32, _vp, _u32, _u32, _vp, _u64, _vp, _vp, _u64, _vp,
                                    _u64, _vp, _vp]),
    "mh_power_draws": (_int, [_vp, _u32, _vp, _u32, _u64, ct.c_double, ct.c_double, ct.c_double, _vp, _u64, _vp]),
    "mh_reduce_rows": (_int, [_vp, _vp, _u64, _vp, _vp, _vp]),
    "mh_compact": (_int, [_vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "mh_synth_poisson": (_int, [_vp, _vp, _vp, _u32, _u64, _vp, _u64, _vp]),
    "mh_rebin": (_int, [_vp, _vp, _vp, _u32, _u64, _u32, _int, _vp, _vp, _vp]),
    "mh_deinterleave": (_int, [_vp, _u64, _u32, _vp, _vp, _vp]),
    "mh_deinterleave_packed": (_int, [_vp, _u64, _u32, _u32, _vp, _vp, _u64, _vp]),
    "mh_interleave": (_int, [_vp, _vp, _u64, _u32, _vp, _vp]),
    "mh_interleave_packed": (_int, [_vp, _vp, _u64, _u32, _u32, _u64, _vp, _vp]),
    "mh_sweep_create": (_int, [ct.POINTER(_vp), _vp, _vp, _u32, _vp, _u32]),
    "mh_sweep_destroy": (_int, [_vp]),
    "mh_sweep_info": (_int, [_vp, ct.POINTER(_u32), _vp]),
    "mh_sweep_run": (_int, [_vp, _vp, _vp, _vp]),
}

_library = Library(globals(), "libmuahuff.so", "mh_last_error")
lib, check = _library.lib, _library.check


def use_library(path):
    """Load the kernels from another build of libmuahuff.so (same-box A/B runs in tools/).  Must be
    called before the first use; there is no environment override."""
    global SO
    if _library.handle is not None:
        raise RuntimeError("libmuahuff.so is already loaded")
    SO = str(path)


def device_info(device=0):
    cu, mem = _int(0), _u64(0)
    name, arch = ct.create_string_buffer(256), ct.create_string_buffer(256)
    check(lib().mh_device_info(device, ct.byref(cu), ct.byref(mem), name, 256, arch, 256))
    return dict(cu_count=cu.value, hbm_bytes=mem.value, name=name.value.decode(), arch=arch.value.decode())
