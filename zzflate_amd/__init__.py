"""zzflate_amd -- MI355X-native DEFLATE encoder behind zzflate's entry points.

Host-side mirror of the reference interface (zzflate/zzflate.h:8-19) over the C ABI of
libzzflate_amd.so (include/zzflate_amd.h). Names follow the reference: ``Format``, ``Config``,
``ZzFlateEncode``, ``ZzFlateEncodeToCallback``, ``adler32x``, ``combine``, ``crc32``.

There is no CPU encode path: importing works without a GPU (so that the ABI can be inspected), but
every encode call raises ``ZzFlateError`` when no HIP device is usable.
"""
import ctypes
import enum
import os
from dataclasses import dataclass

from . import build as _build

__all__ = [
    "Format", "Config", "ZzFlateError", "ZzFlateEncode", "ZzFlateEncodeToCallback", "adler32x", "combine",
    "crc32", "crc32_combine", "bound", "Context", "lib", "DEFAULT_PACKET", "generate_host", "header", "trailer",
    "MEMBERS_BLOCK", "members_bound", "members_header", "gzi_bytes", "packet_checksums_host",
    "POINTS_CHUNK", "points_index_bound", "points_thin",
    "MP_START", "MP_END", "members_index_from_points",
]

DEFAULT_PACKET = 32768
POINTS_SPACING = 131072          # decoded bytes between two points of a point index (ZZ_POINTS_SPACING_DEFAULT)
POINTS_CHUNK = 16384             # compressed bytes per searched chunk of Context.points_index (ZZ_POINTS_CHUNK_DEFAULT)
MEMBERS_BLOCK = 65280            # input bytes per member of a blocked gzip file (bgzip's)
MEMBERS_NO_EOF = 1
MEMBERS_EXTENDED = 2                 # zz_encode_members_device's flags: levels 4..6 through the call's own switch
BATCH_EXTENDED = 1                   # zz_encode_batch_flags_device's flags: the same for batches
_ERR = (1 << 64) - 1


class Format(enum.IntEnum):  # zzflate.h:8
    Zlib = 0
    Gzip = 1
    Deflate = 2


@dataclass
class Config:  # zzflate.h:10-15
    format: Format = Format.Zlib
    level: int = 1
    threaded: bool = True


class _CConfig(ctypes.Structure):
    _fields_ = [("format", ctypes.c_int32), ("level", ctypes.c_uint8), ("threaded", ctypes.c_uint8)]


class ZzFlateError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"zzflate_amd error {code}: {msg}")
        self.code = code


def _load():
    # PyTorch wheels bundle their own HIP/HSA runtime (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7). Two
    # HIP runtimes in one process do not work ("no ROCm-capable device"), so when torch is installed it is
    # imported first: the library's NEEDED libamdhip64.so.7 then binds to the runtime torch already loaded.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = _build.build()          # returns at once when the library is newer than every source under csrc/ and include/
    path = os.environ.get("ZZFLATE_AMD_LIB", path)      # diagnostics: an experimental build of the same sources
    L = ctypes.CDLL(path)
    u64, u32, i32, vp = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p
    pu64 = ctypes.POINTER(ctypes.c_uint64)
    sig = {
        "zz_ctx_create": (i32, [i32, ctypes.POINTER(vp)]),
        "zz_ctx_destroy": (None, [vp]),
        "zz_ctx_workspace_bytes": (u64, [vp]),
        "zz_ctx_enable_timing": (None, [vp, i32]),
        "zz_ctx_set_warm_window": (i32, [vp, u32]),
        "zz_ctx_set_extended_levels": (i32, [vp, i32]),
        "zz_ctx_last_kernel_ms": (ctypes.c_double, [vp]),
        "zz_bound": (u64, [u64, i32, i32, u32]),
        "zz_encode": (i32, [vp, pu64, vp, u64, ctypes.POINTER(_CConfig)]),
        "zz_encode_callback": (i32, [vp, u64, ctypes.POINTER(_CConfig), vp, vp]),
        "zz_set_packet_size": (i32, [u32]),
        "zz_get_packet_size": (u32, []),
        "zz_encode_device": (i32, [vp, vp, u64, vp, u64, pu64, i32, i32, u32, vp]),
        "zz_encode_device_async": (i32, [vp, vp, u64, vp, u64, i32, i32, u32, vp]),
        "zz_encode_batch_device": (i32, [vp, u64, vp, vp, vp, vp, vp, i32, i32, u32, vp]),
        "zz_encode_batch_flags_device": (i32, [vp, u64, vp, vp, vp, vp, vp, i32, i32, u32, i32, vp]),
        "zz_encode_members_device": (i32, [vp, vp, u64, vp, u64, pu64, i32, u32, u32, i32, vp, u64, vp]),
        "zz_encode_members_bound": (u64, [u64, u32, u32, i32]),
        "zz_members_header": (i32, [u32, vp]),
        "zz_ctx_last_encode_members_stats": (i32, [vp, pu64, pu64]),
        "zz_encode_finish": (i32, [vp, pu64]),
        "zz_encode_stream_device": (i32, [vp, vp, u64, vp, u64, pu64, i32, i32, vp]),
        "zz_encode_ranges_device": (i32, [vp, vp, u64, vp, u64, pu64, i32, i32, u32, vp]),
        "zz_encode_stream_chunks_device": (i32, [vp, vp, u64, vp, u64, pu64, i32, i32, pu64, u32, ctypes.POINTER(u32), vp]),
        "zz_encode_shard_device": (i32, [vp, vp, u64, u64, i32, vp, u64, pu64, ctypes.POINTER(u32), i32, i32, u32, vp]),
        "zz_encode_shard_device_async": (i32, [vp, vp, u64, u64, i32, vp, u64, i32, i32, u32, vp]),
        "zz_encode_shard_finish": (i32, [vp, pu64, ctypes.POINTER(u32), i32]),
        "zz_encode_multi_device": (i32, [ctypes.POINTER(vp), i32, ctypes.POINTER(vp), pu64, pu64, vp, u64, pu64, i32, i32, u32]),
        "zz_verify_last_device": (i32, [vp, pu64, pu64, vp]),
        "zz_packet_extent_device": (i32, [vp, u64, pu64, pu64, vp]),
        "zz_packet_index_device": (i32, [vp, vp, u64, pu64, vp]),
        "zz_decode_device": (i32, [vp, vp, u64, vp, u64, pu64, i32, u32, vp, u64, vp]),
        "zz_points_index_host": (i32, [vp, u64, i32, u64, vp, u64, pu64, pu64]),
        "zz_decode_points_device": (i32, [vp, vp, u64, vp, u64, pu64, i32, vp, u64, vp]),
        "zz_points_index_bound": (u64, [u64, u64]),
        "zz_points_index_device": (i32, [vp, vp, u64, i32, u64, u64, vp, u64, pu64, pu64, vp]),
        "zz_ctx_last_points_index_stats": (i32, [vp, pu64, pu64, ctypes.POINTER(u32)]),
        "zz_decode_batch_device": (i32, [vp, u64, vp, vp, vp, vp, vp, vp, i32, vp]),
        "zz_decode_range_device": (i32, [vp, vp, u64, i32, u32, vp, u64, u64, u64, vp, u64, pu64, vp]),
        "zz_ctx_last_decode_range_stats": (i32, [vp, pu64, pu64, ctypes.POINTER(u32), pu64]),
        "zz_decode_ranges_device": (i32, [vp, vp, u64, i32, u32, vp, u64, u64, vp, vp, vp, vp, vp, vp, vp]),
        "zz_packet_checksums_device": (i32, [vp, vp, u64, u32, i32, vp, u64, pu64, vp]),
        "zz_decode_range_checked_device": (i32, [vp, vp, u64, i32, u32, vp, u64, vp, u64, u64, u64, vp, u64, pu64, vp]),
        "zz_decode_ranges_checked_device": (i32, [vp, vp, u64, i32, u32, vp, u64, vp, u64, u64, vp, vp, vp, vp, vp, vp, vp]),
        "zz_ctx_last_decode_ranges_stats": (i32, [vp, pu64, ctypes.POINTER(u32), pu64, ctypes.POINTER(u32)]),
        "zz_decode_members_device": (i32, [vp, vp, u64, vp, u64, pu64, vp]),
        "zz_ctx_last_decode_members_stats": (i32, [vp, pu64, pu64, ctypes.POINTER(i32)]),
        "zz_members_index_device": (i32, [vp, vp, u64, vp, u64, pu64, vp]),
        "zz_members_find_device": (i32, [vp, vp, u64, u64, vp, u64, pu64, vp]),
        "zz_decode_members_found_device": (i32, [vp, vp, u64, vp, u64, pu64, vp]),
        "zz_ctx_last_members_find_stats": (i32, [vp, pu64, pu64, pu64, ctypes.POINTER(u32)]),
        "zz_members_points_device": (i32, [vp, vp, u64, u64, u64, vp, u64, pu64, pu64, vp]),
        "zz_ctx_last_members_points_stats": (i32, [vp, pu64, pu64, pu64, pu64, ctypes.POINTER(u32)]),
        "zz_members_points_to_index": (i32, [vp, u64, vp, u64, pu64]),
        "zz_decode_members_points_device": (i32, [vp, vp, u64, vp, u64, pu64, vp, u64, u64, vp]),
        "zz_ctx_last_decode_members_points_stats": (i32, [vp, pu64, pu64, pu64, ctypes.POINTER(u32), pu64, ctypes.POINTER(u32), ctypes.POINTER(i32)]),
        "zz_decode_members_ranges_device": (i32, [vp, vp, u64, vp, u64, u64, vp, vp, vp, vp, vp, vp, vp]),
        "zz_ctx_last_decode_members_ranges_stats": (i32, [vp, pu64, ctypes.POINTER(u32)]),
        "zz_points_windows_host": (i32, [vp, u64, i32, vp, u64, vp, vp]),
        "zz_decode_points_ranges_device": (i32, [vp, vp, u64, i32, vp, u64, vp, vp, u64, vp, vp, vp, vp, vp, vp, vp]),
        "zz_points_windows_device": (i32, [vp, vp, u64, i32, vp, u64, vp, u64, vp, vp, vp, u64, u64, vp]),
        "zz_ctx_last_points_windows_stats": (i32, [vp, pu64, pu64, ctypes.POINTER(u32)]),
        "zz_points_thin": (i32, [vp, u64, u64, vp, u64, pu64]),
        "zz_ctx_last_decode_points_ranges_stats": (i32, [vp, pu64, ctypes.POINTER(u32)]),
        "zz_ctx_last_decode_path": (i32, [vp]),
        "zz_ctx_last_decode_stats": (i32, [vp, pu64, ctypes.POINTER(u32)]),
        "zz_ctx_last_decode_index_device": (i32, [vp, vp, u64, pu64, vp]),
        "zz_header": (i32, [i32, vp]),
        "zz_trailer": (i32, [i32, u32, u64, vp]),
        "zz_adler32": (u32, [u32, vp, u64]),
        "zz_adler32_combine": (u32, [u32, u32, u64]),
        "zz_crc32": (u32, [vp, u64, u32]),
        "zz_crc32_combine": (u32, [u32, u32, u64]),
        "zz_generate_device": (i32, [vp, i32, u64, u64, vp, u64, vp]),
        "zz_generate_host": (i32, [i32, u64, u64, vp, u64]),
        "zz_debug_reset_devices": (None, []),
        "zz_debug_host_staging_bytes": (u64, []),
        "zz_debug_lds_atomic_order": (i32, [vp, u32, pu64, pu64]),
        "zz_debug_force_lds_order": (None, [i32]),
        "zz_debug_peer_state": (i32, [i32, i32]),
        "zz_debug_last_pulls": (None, [ctypes.POINTER(i32), ctypes.POINTER(i32)]),
        "zz_debug_lds_order_verdict": (i32, [i32]),
        "zz_debug_code_lengths": (i32, [vp, u32, vp, vp, vp, vp, vp, vp]),
        "zz_debug_wg_scan": (i32, [vp, i32, u32, u64, vp, vp, vp]),
        "zz_last_error": (ctypes.c_char_p, []),
        "zz_version": (ctypes.c_char_p, []),
        "zz_build_flags": (ctypes.c_char_p, []),
        "zz_debug_force_lds_violation": (None, [i32]),
        "zz_debug_reset_lds_order": (None, [i32]),
        "zz_debug_l1_kernel": (i32, [vp]),
        "zz_debug_l2_kernel": (i32, [vp]),
    }
    # (diagnostic hooks an older experimental build named by ZZFLATE_AMD_LIB may lack: A/B runs of tools/abn.sh)
    optional = {"zz_build_flags", "zz_debug_force_lds_violation", "zz_debug_reset_lds_order", "zz_debug_l1_kernel", "zz_debug_l2_kernel",
                "zz_debug_wg_scan"}
    for name, (res, args) in sig.items():
        if name in optional and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    return L


lib = _load()
_CALLBACK = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8), ctypes.c_uint64)


def _check(rc):
    if rc != 0:
        raise ZzFlateError(rc, lib.zz_last_error().decode())


def _cfg(config):
    return _CConfig(int(config.format), int(config.level), 1 if config.threaded else 0)


def bound(n, format=Format.Zlib, level=1, packet_size=DEFAULT_PACKET):
    return lib.zz_bound(n, int(format), int(level), packet_size)


def ZzFlateEncode(source, config, dest_capacity=None):
    """zzflate.h:17 -- returns the encoded bytes. ``dest_capacity`` plays the role of ``*destLen`` on
    entry; a destination that is too small raises (the C entry point sets ``*destLen = ~0``)."""
    import numpy as np
    src = source if isinstance(source, bytes) else bytes(source)
    cap = bound(len(src), config.format, config.level, lib.zz_get_packet_size()) if dest_capacity is None else dest_capacity
    dest = np.empty(max(cap, 1), dtype=np.uint8)           # not zero-filled: the library writes it
    n = ctypes.c_uint64(cap)
    c = _cfg(config)
    rc = lib.zz_encode(dest.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n), src, len(src), ctypes.byref(c))
    _check(rc)
    return dest[: n.value].tobytes()


def ZzFlateEncodeToCallback(source, config, callback):
    """zzflate.h:19 -- ``callback(chunk: bytes)`` is called for the header, each stream chunk and the trailer."""
    src = bytes(source)
    failure = []

    def tramp(_user, ptr, nbytes):
        # an exception must not vanish inside the ctypes trampoline: keep the first one, stop forwarding, re-raise below
        if not failure:
            try:
                callback(ctypes.string_at(ptr, nbytes))
            except BaseException as e:          # noqa: BLE001
                failure.append(e)
        return 0

    cb = _CALLBACK(tramp)
    c = _cfg(config)
    rc = lib.zz_encode_callback(src, len(src), ctypes.byref(c), ctypes.cast(cb, ctypes.c_void_p), None)
    if failure:
        raise failure[0]
    _check(rc)


def adler32x(start, data):  # adler.cpp:17-43
    b = bytes(data)
    return lib.zz_adler32(start, b, len(b))


def combine(first, second, len_second):  # adler.cpp:5-15
    return lib.zz_adler32_combine(first, second, len_second)


def crc32(data, start=0):  # crc.h:7
    b = bytes(data)
    return lib.zz_crc32(b, len(b), start)


def crc32_combine(crc1, crc2, len2):
    return lib.zz_crc32_combine(crc1, crc2, len2)


def header(format):
    buf = ctypes.create_string_buffer(10)
    n = lib.zz_header(int(format), buf)
    return buf.raw[:n]


def trailer(format, cks_total, n):
    buf = ctypes.create_string_buffer(8)
    k = lib.zz_trailer(int(format), cks_total, n, buf)
    return buf.raw[:k]


def packet_checksums_host(data, format=Format.Zlib, packet_size=DEFAULT_PACKET):
    """The packet checksum sidecar of ``data`` by Python's zlib: one value per packet of ``packet_size`` decoded bytes (one for
    empty data) -- ``zlib.adler32`` for Format.Zlib, ``zlib.crc32`` for Gzip and Deflate. What ``Context.packet_checksums``
    computes on the device."""
    import zlib
    data = bytes(data)
    f = zlib.adler32 if int(format) == int(Format.Zlib) else zlib.crc32
    return [f(data[k: k + packet_size]) for k in range(0, max(len(data), 1), packet_size)]


def points_index_host(data, format=Format.Zlib, spacing=POINTS_SPACING):
    """The point index of the zlib / gzip / raw stream ``data`` (bytes-like, host memory), made in one sequential pass on the
    host: ``(points, decoded_length)`` with ``points`` an ``(entries, 2)`` int64 CPU tensor of (bit offset of a block header
    behind the container header, decoded bytes in front of it); the first row is (0, 0), the last (end of the final block,
    decoded length). A point is taken at the first block boundary at or behind every multiple of ``spacing`` decoded bytes
    (1: every block). The stream is checked, trailer included: ZzFlateError (E_DATA, E_UNSUPPORTED) otherwise. What
    ``Context.decode_points`` takes."""
    import torch
    if isinstance(spacing, bool) or not isinstance(spacing, int):
        raise TypeError("spacing must be an int")
    if spacing < 1:
        raise ValueError("spacing must be at least 1")
    data = bytes(data)
    entries, n = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = lib.zz_points_index_host(data, len(data), int(format), spacing, None, 0, ctypes.byref(entries), ctypes.byref(n))
    if rc != E_NOSPACE:
        _check(rc)
    points = torch.zeros((entries.value, 2), dtype=torch.int64)
    _check(lib.zz_points_index_host(data, len(data), int(format), spacing, points.data_ptr(), entries.value, ctypes.byref(entries),
                                    ctypes.byref(n)))
    return points, n.value


def points_index_bound(src_len, chunk_bytes=POINTS_CHUNK):
    """Rows that always suffice for ``Context.points_index`` of a stream of ``src_len`` bytes: its chunks plus one."""
    return lib.zz_points_index_bound(src_len, chunk_bytes)


POINTS_WINDOW = 32768                                   # ZZ_POINTS_WINDOW: bytes of a window slot


def _points_tensor(points, where):
    import torch
    if not isinstance(points, torch.Tensor) or points.dtype != torch.int64 or points.dim() != 2 or points.shape[1] != 2 or not points.is_contiguous():
        raise TypeError("points must be a contiguous int64 tensor of shape [segments + 1, 2] (as points_index_host() returns)")
    if points.shape[0] < 2:
        raise ValueError("a point index has at least two rows")
    if where == "cpu" and points.device.type != "cpu":
        raise ValueError("points must be a CPU tensor")


def points_windows_host(data, points, format=Format.Zlib):
    """The sidecar that lets a segment of the point index ``points`` of the stream ``data`` decode alone, made in one more
    sequential pass on the host: ``(windows, sums)`` -- a uint8 CPU tensor ``[segments, 32768]`` (slot k: the decoded bytes in
    front of segment k, right-aligned; what lies in front of them is zero here and unspecified by the format) and an int32 CPU
    tensor ``[segments]`` (adler32 of a zlib stream's segment, crc32 of a gzip or raw one, as the int32 of the same bits). The
    index is verified against the stream: ZzFlateError (E_DATA, E_UNSUPPORTED) otherwise. Moved to the device, what
    ``Context.decode_points_ranges`` takes."""
    import torch
    _points_tensor(points, "cpu")
    data = bytes(data)
    segments = points.shape[0] - 1
    windows = torch.zeros((segments, POINTS_WINDOW), dtype=torch.uint8)
    sums = torch.zeros(segments, dtype=torch.int32)
    _check(lib.zz_points_windows_host(data, len(data), int(format), points.data_ptr(), points.shape[0], windows.data_ptr(), sums.data_ptr()))
    return windows, sums


def points_thin(points, spacing):
    """The point index ``points`` (an ``(entries, 2)`` int64 CPU tensor) thinned to ``spacing`` decoded bytes by the builders' own
    rule: row 0 and the last row stay, an inner row stays iff it is the first at or behind the next multiple of ``spacing``. A
    dense index (``Context.points_index``, spacing 1) thinned to ``s`` is the index at spacing ``s``. Returns a CPU tensor."""
    import torch
    _points_tensor(points, "cpu")
    if isinstance(spacing, bool) or not isinstance(spacing, int):
        raise TypeError("spacing must be an int")
    if spacing < 1:
        raise ValueError("spacing must be at least 1")
    out = torch.zeros((points.shape[0], 2), dtype=torch.int64)
    entries = ctypes.c_uint64(0)
    _check(lib.zz_points_thin(points.data_ptr(), points.shape[0], spacing, out.data_ptr(), out.shape[0], ctypes.byref(entries)))
    return out[: entries.value].clone()


MP_START = 1 << 63                                      # ZZ_MP_START, ZZ_MP_END: the flags in a member point index's in_bit
MP_END = 1 << 62                                        # (an int64 tensor holds a START row's in_bit as a negative number)


def members_index_from_points(points):
    """The index ``Context.decode_members_ranges`` takes -- ``members_find``'s pairs (file offset, decoded offset), members + 1 of
    them -- from the START / END rows of the member point index ``points`` (``Context.members_points``' CPU tensor). Returns an
    ``(members + 1, 2)`` int64 CPU tensor; move it to the device for the reads. Raises ZzFlateError (E_DATA) where the rows are
    not START, inner rows, END per member."""
    import torch
    _points_tensor(points, "cpu")
    out = torch.zeros((points.shape[0], 2), dtype=torch.int64)
    entries = ctypes.c_uint64(0)
    _check(lib.zz_members_points_to_index(points.data_ptr(), points.shape[0], out.data_ptr(), out.shape[0], ctypes.byref(entries)))
    return out[: entries.value].clone()


def members_bound(n, block_size=MEMBERS_BLOCK, packet_size=DEFAULT_PACKET, eof=True):
    """The largest file ``Context.encode_members`` can write for ``n`` input bytes (every member stored)."""
    b = lib.zz_encode_members_bound(n, block_size, packet_size, 0 if eof else MEMBERS_NO_EOF)
    if b == _ERR:
        raise ZzFlateError(E_ARG, "block size and packet size: a block's stored member must fit 65536 bytes")
    return b


def members_header(member_bytes):
    """The 18-byte header of a blocked member of ``member_bytes`` bytes in all (header, body, CRC-32, ISIZE)."""
    buf = ctypes.create_string_buffer(18)
    k = lib.zz_members_header(member_bytes, buf)
    if k < 0:
        _check(k)
    return buf.raw[:k]


def gzi_bytes(offsets, n, block_size=MEMBERS_BLOCK):
    """bgzip's ``.gzi`` index of a file ``Context.encode_members`` wrote from ``n`` input bytes: a little-endian u64 count, then
    the pairs (compressed offset, uncompressed offset) of every member but the first. ``offsets`` is the host copy of the
    call's offsets array (members + 1 entries)."""
    import struct
    offsets = [int(v) for v in offsets]
    members = len(offsets) - 1
    if members < 0 or members != -(-n // block_size):
        raise ValueError(f"{len(offsets)} offsets do not describe {n} bytes in blocks of {block_size}")
    out = [struct.pack("<Q", max(members - 1, 0))]
    for i in range(1, members):
        out.append(struct.pack("<QQ", offsets[i], i * block_size))
    return b"".join(out)


def members_index_from_offsets(offsets, n, block_size=MEMBERS_BLOCK, eof=True):
    """The index ``Context.decode_members_ranges`` takes, by arithmetic, for a file ``Context.encode_members`` wrote from ``n``
    input bytes: a list of (file offset, decoded offset) pairs, one per member and one behind the last. ``offsets`` is the host
    copy of the call's offsets array (data members + 1 entries); member i begins at decoded offset ``min(i * block_size, n)``;
    with ``eof`` one more pair follows for the 28-byte empty last member."""
    offsets = [int(v) for v in offsets]
    members = len(offsets) - 1
    if members < 0 or members != -(-n // block_size):
        raise ValueError(f"{len(offsets)} offsets do not describe {n} bytes in blocks of {block_size}")
    pairs = [(offsets[i], min(i * block_size, n)) for i in range(members + 1)]
    if eof:
        pairs.append((offsets[members] + 28, n))
    return pairs


def generate_host(kind, seed, first_byte, n):
    buf = ctypes.create_string_buffer(max(n, 1))
    _check(lib.zz_generate_host(kind, seed, first_byte, buf, n))
    return buf.raw[:n]


GEN_TEXT, GEN_RANDOM, GEN_LOG, GEN_MIX = 0, 1, 2, 3
# which path a decode finished on (Context.last_decode_path)
DECODE_INDEXED, DECODE_DISCOVERED, DECODE_SERIAL, DECODE_POINTS = 1, 2, 3, 4
# which path a members decode finished on (Context.last_decode_members_stats)
MEMBERS_BLOCKED, MEMBERS_WALKED, MEMBERS_SERIAL = 1, 2, 3
E_NOSPACE, E_ARG, E_UNSUPPORTED, E_DATA = -2, -4, -5, -6


class Context:
    """Device context: workspace + timing. Buffers are torch tensors (uint8, on the context's device) or
    raw device pointers; PyTorch is only the allocator here."""

    def __init__(self, device=0):
        h = ctypes.c_void_p()
        _check(lib.zz_ctx_create(device, ctypes.byref(h)))
        self._h = h
        self.device = device

    def close(self):
        if self._h:
            lib.zz_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _ptr(t):
        return t if isinstance(t, int) else t.data_ptr()

    def _stream(self):
        try:
            import torch
            return torch.cuda.current_stream(self.device).cuda_stream     # this context's device, not torch's current one
        except Exception:
            return 0

    def set_warm_window(self, nbytes):
        """Levels >= 1: hash the last ``nbytes`` (0..32768) in front of every packet into its table before parsing it, so
        that matches may reach across packet boundaries (0 = cold packets = the reference's threaded stream)."""
        _check(lib.zz_ctx_set_warm_window(self._h, nbytes))

    def set_extended_levels(self, on=True):
        """Accept levels 4, 5, 6 (beyond the reference, which rejects them): hash chains of depth 2 / 4 / 8 over a window of
        8 / 32 / 32 KiB, one-step lazy matching, package-merge code lengths. Off by default, so that level > 3
        stays the reference's error."""
        _check(lib.zz_ctx_set_extended_levels(self._h, 1 if on else 0))

    def enable_timing(self, on=True):
        lib.zz_ctx_enable_timing(self._h, 1 if on else 0)

    def last_kernel_ms(self):
        return lib.zz_ctx_last_kernel_ms(self._h)

    def workspace_bytes(self):
        return lib.zz_ctx_workspace_bytes(self._h)

    def encode(self, src, n, dst, cap, format=Format.Zlib, level=1, packet_size=DEFAULT_PACKET, stream=None):
        """Whole stream on the device; returns the number of bytes written to ``dst``."""
        out = ctypes.c_uint64(0)
        st = self._stream() if stream is None else stream
        _check(lib.zz_encode_device(self._h, self._ptr(src), n, self._ptr(dst), cap, ctypes.byref(out), int(format),
                                    int(level), packet_size, st))
        return out.value

    def _item(self, t):
        """(data_ptr, nbytes) of a batch item: a contiguous uint8 tensor on this context's device, or such a pair"""
        import torch
        if isinstance(t, torch.Tensor):
            if t.dtype != torch.uint8 or not t.is_contiguous():
                raise TypeError("items must be contiguous uint8 tensors or (data_ptr, nbytes) pairs")
            if t.device.type != "cuda" or t.device.index != self.device:
                raise ValueError(f"items must live on this context's device (cuda:{self.device}), not {t.device}")
            return t.data_ptr(), t.numel()
        p, nb = t
        return int(p), int(nb)

    def encode_batch(self, srcs, dsts, format=Format.Zlib, level=1, packet_size=DEFAULT_PACKET, caps=None, stream=None):
        """Many independent streams in one call: item i = ``srcs[i]`` becomes its own complete stream in ``dsts[i]``, the bytes
        ``encode`` would write for it alone. Items are uint8 tensors on this context's device (their whole length) or
        ``(data_ptr, nbytes)`` pairs; ``caps`` defaults to each destination's size. Returns the list of lengths, ``None``
        for an item that did not fit its destination (the others are complete). Levels 0..3, cold packets; levels 4..6:
        ``encode_batch_extended``."""
        return self._encode_batch(srcs, dsts, format, level, packet_size, caps, stream, 0)

    def encode_batch_extended(self, srcs, dsts, format=Format.Zlib, level=6, packet_size=DEFAULT_PACKET, caps=None, stream=None):
        """``encode_batch`` with the call's own switch for the extended levels set (``BATCH_EXTENDED``): levels 0..6, whatever
        ``set_extended_levels`` says -- that stays ``encode``'s switch. At levels 4..6 an item is the stream ``encode`` writes
        for it alone with the extended levels on; a packet's window is the bytes of its own item in front of it (at most
        8 KiB at level 4, 32 KiB at levels 5 and 6) and never reaches in front of the item. Levels 0..3 are ``encode_batch``."""
        return self._encode_batch(srcs, dsts, format, level, packet_size, caps, stream, BATCH_EXTENDED)

    def _encode_batch(self, srcs, dsts, format, level, packet_size, caps, stream, flags):
        import torch
        if len(srcs) != len(dsts):
            raise ValueError(f"{len(srcs)} sources but {len(dsts)} destinations")
        if caps is not None and len(caps) != len(dsts):
            raise ValueError(f"{len(caps)} capacities for {len(dsts)} destinations")
        k = len(srcs)
        if k == 0:
            return []

        split = self._item
        s = [split(t) for t in srcs]
        d = [split(t) for t in dsts]
        cp = [nb for _, nb in d] if caps is None else [int(c) for c in caps]
        dev = f"cuda:{self.device}"
        # the five device arrays (pointers and sizes as int64: the C side reads them as pointers and uint64)
        table = torch.tensor([[p for p, _ in s], [nb for _, nb in s], [p for p, _ in d], cp], dtype=torch.int64).to(dev)
        out = torch.empty(k, dtype=torch.int64, device=dev)
        st = self._stream() if stream is None else stream
        rc = lib.zz_encode_batch_flags_device(self._h, k, table[0].data_ptr(), table[1].data_ptr(), table[2].data_ptr(),
                                              table[3].data_ptr(), out.data_ptr(), int(format), int(level), packet_size, flags, st)
        if rc not in (0, E_NOSPACE):
            _check(rc)
        return [None if v == -1 else v for v in out.cpu().tolist()]

    def decode_batch(self, srcs, dsts, format=Format.Zlib, caps=None, stream=None):
        """Many independent streams back to their bytes in one call: item i = ``srcs[i]`` (one complete zlib / gzip / raw
        stream, from ``encode_batch`` or anywhere else) is decoded into ``dsts[i]``. Items as ``encode_batch`` takes them;
        ``caps`` defaults to each destination's size. Returns ``(lens, status)``: ``lens[i]`` the decoded length or ``None``,
        ``status[i]`` 0, E_DATA, E_NOSPACE or E_UNSUPPORTED -- an item's own failure does not raise, and leaves the others
        complete. One wavefront decodes one item: fast for thousands of items, slow for one large one (use ``decode``)."""
        import torch
        if len(srcs) != len(dsts):
            raise ValueError(f"{len(srcs)} sources but {len(dsts)} destinations")
        if caps is not None and len(caps) != len(dsts):
            raise ValueError(f"{len(caps)} capacities for {len(dsts)} destinations")
        k = len(srcs)
        if k == 0:
            return [], []
        s = [self._item(t) for t in srcs]
        d = [self._item(t) for t in dsts]
        cp = [nb for _, nb in d] if caps is None else [int(c) for c in caps]
        dev = f"cuda:{self.device}"
        table = torch.tensor([[p for p, _ in s], [nb for _, nb in s], [p for p, _ in d], cp], dtype=torch.int64).to(dev)
        out = torch.empty(k, dtype=torch.int64, device=dev)
        status = torch.empty(k, dtype=torch.int32, device=dev)
        st = self._stream() if stream is None else stream
        rc = lib.zz_decode_batch_device(self._h, k, table[0].data_ptr(), table[1].data_ptr(), table[2].data_ptr(),
                                        table[3].data_ptr(), out.data_ptr(), status.data_ptr(), int(format), st)
        if rc not in (0, E_NOSPACE, E_DATA):
            _check(rc)
        return [None if v == -1 else v for v in out.cpu().tolist()], status.cpu().tolist()

    def encode_members(self, src, n, dst, cap, level=1, block_size=MEMBERS_BLOCK, packet_size=DEFAULT_PACKET, eof=True, offsets=None,
                       stream=None):
        """One blocked gzip (BGZF) file from ``src[:n]``: members of ``block_size`` input bytes back to back, each announcing its
        length, then bgzip's empty last member (``eof=False`` omits it: pieces that ``cat`` will join). bgzip, samtools, tabix,
        ``gzip.decompress`` and ``decode_members`` (in parallel) read it. A member is the raw-deflate stream ``encode_batch``
        writes for its block, or the block's level-0 stream where that is shorter. ``offsets``: an int64 tensor on this
        context's device that receives members + 1 file offsets (``gzi_bytes`` turns its host copy into a ``.gzi`` index).
        Returns the file's length; raises ZzFlateError (E_NOSPACE: it does not fit ``cap``, nothing is written). Levels 0..3;
        levels 4..6 (bgzip's default is 6): ``encode_members_extended``."""
        return self._encode_members(src, n, dst, cap, level, block_size, packet_size, eof, offsets, stream, 0)

    def encode_members_extended(self, src, n, dst, cap, level=6, block_size=MEMBERS_BLOCK, packet_size=DEFAULT_PACKET, eof=True,
                                offsets=None, stream=None):
        """``encode_members`` with the call's own switch for the extended levels set (``MEMBERS_EXTENDED``): levels 0..6, whatever
        ``set_extended_levels`` says. At levels 4..6 a member's body is its block's raw-deflate stream at that level -- no match
        reaches in front of the block -- or the block's level-0 stream where that is shorter. The same readers read the file."""
        return self._encode_members(src, n, dst, cap, level, block_size, packet_size, eof, offsets, stream, MEMBERS_EXTENDED)

    def _encode_members(self, src, n, dst, cap, level, block_size, packet_size, eof, offsets, stream, flags):
        out = ctypes.c_uint64(0)
        st = self._stream() if stream is None else stream
        op, on = None, 0
        if offsets is not None:
            import torch
            if not isinstance(offsets, torch.Tensor) or offsets.dtype != torch.int64 or offsets.dim() != 1 or not offsets.is_contiguous():
                raise TypeError("offsets must be a contiguous one-dimensional int64 tensor")
            if offsets.device.type != "cuda" or offsets.device.index != self.device:
                raise ValueError(f"offsets must live on this context's device (cuda:{self.device}), not {offsets.device}")
            op, on = offsets.data_ptr(), offsets.numel()
        _check(lib.zz_encode_members_device(self._h, self._ptr(src), n, self._ptr(dst), cap, ctypes.byref(out), int(level), block_size,
                                            packet_size, (0 if eof else MEMBERS_NO_EOF) | flags, op, on, st))
        return out.value

    def last_encode_members_stats(self):
        """(members, members that took the stored fallback) of the last ``encode_members``; (0, 0) after a refused call."""
        m, stored = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _check(lib.zz_ctx_last_encode_members_stats(self._h, ctypes.byref(m), ctypes.byref(stored)))
        return m.value, stored.value

    def encode_async(self, src, n, dst, cap, format=Format.Zlib, level=1, packet_size=DEFAULT_PACKET, stream=None):
        """Enqueue ``encode`` on ``stream`` without waiting; ``finish()`` returns the byte count. One call per context at a
        time: use two contexts on two streams to keep two calls in flight."""
        st = self._stream() if stream is None else stream
        _check(lib.zz_encode_device_async(self._h, self._ptr(src), n, self._ptr(dst), cap, int(format), int(level), packet_size, st))

    def finish(self):
        out = ctypes.c_uint64(0)
        _check(lib.zz_encode_finish(self._h, ctypes.byref(out)))
        return out.value

    def encode_stream(self, src, n, dst, cap, format=Format.Zlib, level=1, stream=None):
        """The reference's sequential whole-buffer stream (threaded=false) into a caller-owned buffer of ``cap`` bytes
        (at level 1 the capacity decides the block lengths, encoder.cpp:331-337)."""
        out = ctypes.c_uint64(0)
        st = self._stream() if stream is None else stream
        _check(lib.zz_encode_stream_device(self._h, self._ptr(src), n, self._ptr(dst), cap, ctypes.byref(out), int(format),
                                           int(level), st))
        return out.value

    def encode_ranges(self, src, n, dst, cap, count, format=Format.Zlib, level=2, stream=None):
        """The reference's own threaded=true split for a machine with ``count`` hardware threads (zzflate.cpp:67-78,97-155):
        ``count`` ranges of ceil(n / count) bytes, one encoder (here: one wavefront) each. Levels 0, 2, 3."""
        out = ctypes.c_uint64(0)
        st = self._stream() if stream is None else stream
        _check(lib.zz_encode_ranges_device(self._h, self._ptr(src), n, self._ptr(dst), cap, ctypes.byref(out), int(format),
                                           int(level), int(count), st))
        return out.value

    def encode_stream_chunks(self, src, n, dst, cap, format=Format.Zlib, level=1, stream=None):
        """The sequential stream as ZzFlateEncodeToCallback produces it (library-owned 1,000,000-byte chunks decide the
        level-1 block lengths); returns (bytes written, [chunk sizes the reference's callback would see])."""
        out = ctypes.c_uint64(0)
        sizes = (ctypes.c_uint64 * 8192)()
        nch = ctypes.c_uint32(0)
        st = self._stream() if stream is None else stream
        _check(lib.zz_encode_stream_chunks_device(self._h, self._ptr(src), n, self._ptr(dst), cap, ctypes.byref(out), int(format),
                                                  int(level), sizes, 8192, ctypes.byref(nch), st))
        return out.value, list(sizes[: nch.value])

    def encode_shard(self, src, n, dst, cap, halo=0, is_last=True, checksum=Format.Zlib, level=1,
                     packet_size=DEFAULT_PACKET, stream=None):
        """One shard (contiguous packet range) of a stream; returns (bytes, checksum partial)."""
        out = ctypes.c_uint64(0)
        cks = ctypes.c_uint32(0)
        st = self._stream() if stream is None else stream
        _check(lib.zz_encode_shard_device(self._h, self._ptr(src), n, halo, 1 if is_last else 0, self._ptr(dst), cap,
                                          ctypes.byref(out), ctypes.byref(cks), int(checksum), int(level), packet_size, st))
        return out.value, cks.value

    def encode_shard_async(self, src, n, dst, cap, halo=0, is_last=True, checksum=Format.Zlib, level=1,
                           packet_size=DEFAULT_PACKET, stream=None):
        """Enqueue one shard and return; `finish_shard` waits for it. src, dst and the stream must stay alive."""
        st = self._stream() if stream is None else stream
        _check(lib.zz_encode_shard_device_async(self._h, self._ptr(src), n, halo, 1 if is_last else 0, self._ptr(dst), cap,
                                                int(checksum), int(level), packet_size, st))

    def finish_shard(self, checksum=Format.Zlib):
        out = ctypes.c_uint64(0)
        cks = ctypes.c_uint32(0)
        _check(lib.zz_encode_shard_finish(self._h, ctypes.byref(out), ctypes.byref(cks), int(checksum)))
        return out.value, cks.value

    def verify_last(self, stream=None):
        """Inflates every packet of the last encode / encode_shard call's output on the device and compares with its
        input (both tensors must still be alive): returns (bad packets, lowest bad packet or None)."""
        bad, first = ctypes.c_uint64(0), ctypes.c_uint64(0)
        st = self._stream() if stream is None else stream
        _check(lib.zz_verify_last_device(self._h, ctypes.byref(bad), ctypes.byref(first), st))
        return bad.value, (None if bad.value == 0 else first.value)

    def packet_extent(self, k, stream=None):
        """(offset behind the container header, bytes) of packet k in the stream the last encode / encode_shard call wrote."""
        off, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
        st = self._stream() if stream is None else stream
        _check(lib.zz_packet_extent_device(self._h, k, ctypes.byref(off), ctypes.byref(nb), st))
        return off.value, nb.value

    def packet_index(self, stream=None):
        """The packet index of the last encode / encode_shard call: an int64 tensor of npk + 1 offsets on this context's
        device, counted from the first DEFLATE byte; the last one is the stream's length. Store it beside the stream to
        decode it in parallel later."""
        import torch
        entries = ctypes.c_uint64(0)
        st = self._stream() if stream is None else stream
        rc = lib.zz_packet_index_device(self._h, None, 0, ctypes.byref(entries), st)
        if rc not in (0, E_NOSPACE) or entries.value == 0:
            _check(rc)
        idx = torch.empty(entries.value, dtype=torch.int64, device=f"cuda:{self.device}")
        _check(lib.zz_packet_index_device(self._h, idx.data_ptr(), entries.value, ctypes.byref(entries), st))
        return idx

    def packet_checksums(self, data, n, format=Format.Zlib, packet_size=DEFAULT_PACKET, stream=None):
        """The packet checksum sidecar of ``data[:n]`` (the input of an encode call, or decoded bytes): an int32 tensor on this
        context's device holding the 32-bit patterns of ``max(1, ceil(n / packet_size))`` checksums, ``zlib.adler32`` of each
        packet for Format.Zlib and ``zlib.crc32`` otherwise (``packet_checksums_host``). Store it beside the stream and its
        packet index; ``decode_range_checked`` and ``decode_ranges_checked`` take it as ``checksums``."""
        import torch
        entries = ctypes.c_uint64(0)
        st = self._stream() if stream is None else stream
        npk = max(1, (n + packet_size - 1) // packet_size) if packet_size > 0 else 1
        cks = torch.empty(npk, dtype=torch.int32, device=f"cuda:{self.device}")
        _check(lib.zz_packet_checksums_device(self._h, self._ptr(data) if n else None, n, packet_size, int(format), cks.data_ptr(), npk,
                                              ctypes.byref(entries), st))
        return cks

    def _sidecar(self, checksums, total_len):
        import torch
        if total_len is None:
            raise TypeError("checksums need total_len, the stream's decoded length")
        if (not isinstance(checksums, torch.Tensor) or checksums.dtype != torch.int32 or checksums.dim() != 1
                or not checksums.is_contiguous()):
            raise TypeError("checksums must be a contiguous one-dimensional int32 tensor (as packet_checksums() returns)")
        if checksums.device.type != "cuda" or checksums.device.index != self.device:
            raise ValueError(f"checksums must live on this context's device (cuda:{self.device}), not {checksums.device}")
        return checksums.data_ptr(), int(total_len)

    def decode(self, src, src_len, dst, cap, format=Format.Zlib, packet_size=DEFAULT_PACKET, index=None, stream=None):
        """Decode the zlib / gzip / raw stream ``src[:src_len]`` into ``dst`` (``cap`` bytes); returns the decoded length.
        ``packet_size`` 1..32768 with ``index`` (an int64 tensor from ``packet_index``): packets decoded in parallel;
        without ``index``: packet starts found on the device first; ``packet_size`` 0: any stream, serially. Any valid
        stream decodes whatever they say. Raises ZzFlateError (code E_DATA, E_NOSPACE, E_UNSUPPORTED) otherwise."""
        out = ctypes.c_uint64(0)
        st = self._stream() if stream is None else stream
        ip, ne = None, 0
        if index is not None:
            import torch
            if not isinstance(index, torch.Tensor) or index.dtype != torch.int64 or index.dim() != 1 or not index.is_contiguous():
                raise TypeError("index must be a contiguous one-dimensional int64 tensor (as packet_index() returns)")
            if index.device.type != "cuda" or index.device.index != self.device:
                raise ValueError(f"index must live on this context's device (cuda:{self.device}), not {index.device}")
            ip, ne = index.data_ptr(), index.numel()
        _check(lib.zz_decode_device(self._h, self._ptr(src), src_len, self._ptr(dst), cap, ctypes.byref(out), int(format),
                                    packet_size, ip, ne, st))
        return out.value

    def decode_points(self, src, src_len, dst, cap, points, format=Format.Zlib, stream=None):
        """``decode`` for any stream that comes with a point index (``points_index_host``): the segments between its points are
        decoded in parallel, one wavefront each, straight into ``dst``. ``points`` is an ``(entries, 2)`` int64 CPU tensor. The
        index decides speed, not the result: one that does not describe the stream sends the call to the serial path
        (``last_decode_path()`` tells DECODE_POINTS from DECODE_SERIAL). Returns the decoded length; raises ZzFlateError as
        ``decode`` does."""
        import torch
        if (not isinstance(points, torch.Tensor) or points.dtype != torch.int64 or points.dim() != 2 or points.shape[1] != 2
                or not points.is_contiguous()):
            raise TypeError("points must be a contiguous (entries, 2) int64 tensor (as points_index_host() returns)")
        if points.device.type != "cpu":
            raise ValueError(f"points must live in host memory, not on {points.device}")
        out = ctypes.c_uint64(0)
        st = self._stream() if stream is None else stream
        _check(lib.zz_decode_points_device(self._h, self._ptr(src), src_len, self._ptr(dst), cap, ctypes.byref(out), int(format),
                                           points.data_ptr(), points.shape[0], st))
        return out.value

    def points_index(self, src, src_len, format=Format.Zlib, chunk_bytes=POINTS_CHUNK, spacing=1, stream=None):
        """The point index of the zlib / gzip / raw stream ``src[:src_len]`` (device memory), built on the device: non-final
        dynamic block headers are searched for in every chunk of ``chunk_bytes`` compressed bytes, the stretches between them
        are measured without writing a byte, and those reached from the stream's first bit become rows. Returns ``(points,
        decoded_length)`` with ``points`` an ``(entries, 2)`` int64 CPU tensor, exactly what ``decode_points`` takes. The
        checksum is NOT checked here (no byte is produced): ``decode_points`` gives the verdict on the stream."""
        import torch
        st = self._stream() if stream is None else stream
        bound = points_index_bound(src_len, chunk_bytes)
        points = torch.zeros((max(bound, 2), 2), dtype=torch.int64)
        entries, n = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _check(lib.zz_points_index_device(self._h, self._ptr(src), src_len, int(format), chunk_bytes, spacing, points.data_ptr(),
                                          points.shape[0], ctypes.byref(entries), ctypes.byref(n), st))
        return points[: entries.value].clone(), n.value

    def last_points_index_stats(self):
        """(candidates, dropped candidates, rounds) of the last ``points_index``."""
        cand, dropped, rounds = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
        _check(lib.zz_ctx_last_points_index_stats(self._h, ctypes.byref(cand), ctypes.byref(dropped), ctypes.byref(rounds)))
        return cand.value, dropped.value, rounds.value

    def decode_found(self, src, src_len, dst, cap, format=Format.Zlib, chunk_bytes=POINTS_CHUNK, stream=None):
        """``decode`` for a stream met for the first time: ``points_index`` on the device, then ``decode_points`` with it.
        Results and path reporting are ``decode_points``'s."""
        points, _ = self.points_index(src, src_len, format, chunk_bytes, 1, stream)
        return self.decode_points(src, src_len, dst, cap, points, format, stream)

    def points_windows(self, src, src_len, points, format=Format.Zlib, fine_points=None, dst=None, cap=None, stage_bytes=0, stream=None):
        """``points_windows_host`` on the device, for a stream in device memory: ``(windows, sums)`` on this context's device -- uint8
        ``[segments, 32768]`` and int32 ``[segments]``, byte for byte what the host builder returns for the CPU tensor ``points``
        and exactly what ``decode_points_ranges`` takes. ``fine_points``: a CPU tensor of rows to decode with, a superset of
        ``points`` (the dense index that ``points`` was thinned from: the decode wants dense rows, the sidecar sparse ones).
        ``dst`` (``cap`` bytes, default its size): also leave the decoded stream there. ``stage_bytes``: decoded bytes per batch
        (0: 64 MiB), which bounds the workspace. The index is verified, never repaired: ZzFlateError (E_DATA, E_UNSUPPORTED,
        E_ARG, E_NOSPACE) otherwise."""
        import torch
        _points_tensor(points, "cpu")
        fp, fn = None, 0
        if fine_points is not None:
            _points_tensor(fine_points, "cpu")
            fp, fn = fine_points.data_ptr(), fine_points.shape[0]
        if isinstance(stage_bytes, bool) or not isinstance(stage_bytes, int):
            raise TypeError("stage_bytes must be an int")
        if stage_bytes < 0:
            raise ValueError("stage_bytes must not be negative")
        dp = None
        if dst is not None:
            if not isinstance(dst, torch.Tensor) or dst.dtype != torch.uint8 or not dst.is_contiguous():
                raise TypeError("dst must be a contiguous uint8 tensor")
            dp, cap = self._ptr(dst), (dst.numel() if cap is None else cap)
        elif cap:
            raise TypeError("cap needs dst")
        segments = points.shape[0] - 1
        dev = torch.device("cuda", self.device)
        windows = torch.empty((segments, POINTS_WINDOW), dtype=torch.uint8, device=dev)
        sums = torch.empty(segments, dtype=torch.int32, device=dev)
        st = self._stream() if stream is None else stream
        _check(lib.zz_points_windows_device(self._h, self._ptr(src), src_len, int(format), points.data_ptr(), points.shape[0], fp, fn,
                                            windows.data_ptr(), sums.data_ptr(), dp, cap or 0, stage_bytes, st))
        return windows, sums

    def last_points_windows_stats(self):
        """(decode batches, pending bytes, most rounds of a batch) of the last ``points_windows``."""
        batches, pending, rounds = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
        _check(lib.zz_ctx_last_points_windows_stats(self._h, ctypes.byref(batches), ctypes.byref(pending), ctypes.byref(rounds)))
        return batches.value, pending.value, rounds.value

    def open_found(self, src, src_len, format=Format.Zlib, chunk_bytes=POINTS_CHUNK, spacing=POINTS_SPACING, dst=None, cap=None,
                   stream=None):
        """A foreign stream in device memory opened for ``decode_points_ranges`` with no host pass over its bytes:
        ``points_index`` (dense) on the device, ``points_thin`` to ``spacing``, ``points_windows`` with the dense rows to decode
        with. Returns ``(points, windows, sums, decoded_length)``, all three tensors on this context's device. With ``dst`` the
        stream is also decoded whole in the same call."""
        import torch
        dense, n = self.points_index(src, src_len, format, chunk_bytes, 1, stream)
        points = points_thin(dense, spacing)
        windows, sums = self.points_windows(src, src_len, points, format, dense, dst, cap, 0, stream)
        return points.to(torch.device("cuda", self.device)), windows, sums, n

    def decode_range(self, src, src_len, dst, cap, first, nbytes, format=Format.Zlib, packet_size=DEFAULT_PACKET, index=None,
                     stream=None):
        """Decoded bytes ``[first, first + nbytes)`` of the packet-mode stream ``src[:src_len]`` into ``dst`` (``cap`` bytes);
        returns how many there are (the range is clipped at the stream's end). ``index`` is the stream's packet index (an int64
        tensor from ``packet_index`` or ``last_decode_index``) and is required; ``packet_size`` is the one the stream was written
        with. Only the packets the range touches and a look-back in front of them are decoded; the trailer's checksum is NOT
        checked (it covers bytes this call never decodes); ``decode_range_checked`` checks what
        it returns. Raises ZzFlateError (E_ARG, E_DATA, E_NOSPACE, E_UNSUPPORTED)."""
        return self._decode_range(src, src_len, dst, cap, first, nbytes, format, packet_size, index, stream, None, None)

    def decode_range_checked(self, src, src_len, dst, cap, first, nbytes, checksums, total_len, format=Format.Zlib,
                             packet_size=DEFAULT_PACKET, index=None, stream=None):
        """``decode_range`` with what it returns verified: ``checksums`` is the stream's sidecar (``packet_checksums``, one entry
        per packet), ``total_len`` its decoded length. The sidecar is first held to the stream's trailer, then every packet the
        range returns bytes from is summed on the device and compared with its entry: E_DATA on any mismatch."""
        if checksums is None:
            raise TypeError("decode_range_checked needs the stream's packet checksums (packet_checksums())")
        return self._decode_range(src, src_len, dst, cap, first, nbytes, format, packet_size, index, stream, checksums, total_len)

    def _decode_range(self, src, src_len, dst, cap, first, nbytes, format, packet_size, index, stream, checksums, total_len):
        import torch
        if index is None:
            raise TypeError("decode_range needs the stream's packet index (packet_index() or last_decode_index())")
        if not isinstance(index, torch.Tensor) or index.dtype != torch.int64 or index.dim() != 1 or not index.is_contiguous():
            raise TypeError("index must be a contiguous one-dimensional int64 tensor (as packet_index() returns)")
        if index.device.type != "cuda" or index.device.index != self.device:
            raise ValueError(f"index must live on this context's device (cuda:{self.device}), not {index.device}")
        out = ctypes.c_uint64(0)
        st = self._stream() if stream is None else stream
        if checksums is not None:
            cp, tl = self._sidecar(checksums, total_len)
            if checksums.numel() != index.numel() - 1:
                raise ValueError(f"{checksums.numel()} checksums for an index of {index.numel() - 1} packets")
            _check(lib.zz_decode_range_checked_device(self._h, self._ptr(src), src_len, int(format), packet_size, index.data_ptr(),
                                                      index.numel(), cp, tl, first, nbytes, self._ptr(dst), cap, ctypes.byref(out), st))
            return out.value
        _check(lib.zz_decode_range_device(self._h, self._ptr(src), src_len, int(format), packet_size, index.data_ptr(),
                                          index.numel(), first, nbytes, self._ptr(dst), cap, ctypes.byref(out), st))
        return out.value

    def last_decode_range_stats(self):
        """(first packet decoded, packets decoded in the final attempt, attempts, pending bytes of the final attempt) of the last
        successful ``decode_range``."""
        fp, npk, pend, tries = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
        _check(lib.zz_ctx_last_decode_range_stats(self._h, ctypes.byref(fp), ctypes.byref(npk), ctypes.byref(tries), ctypes.byref(pend)))
        return fp.value, npk.value, tries.value, pend.value

    def decode_ranges(self, src, src_len, firsts, nbytes, dsts, caps=None, format=Format.Zlib, packet_size=DEFAULT_PACKET,
                      index=None, stream=None):
        """Many reads of one stored stream in one call: read r = decoded bytes ``[firsts[r], firsts[r] + nbytes[r])`` of the
        packet-mode stream ``src[:src_len]`` into ``dsts[r]``, what ``decode_range`` gives it alone. ``dsts`` are items as
        ``decode_batch`` takes them; ``caps`` defaults to ``min(nbytes[r], destination size)``; ``index`` is required. Returns
        ``(lens, status)``: ``lens[r]`` the bytes read (clipped at the stream's end) or ``None``, ``status[r]`` 0, E_ARG,
        E_NOSPACE, E_DATA or E_UNSUPPORTED -- a read's own failure does not raise and leaves the others complete; a failure of
        the call (arguments, container header, an index that is not this stream's) raises. The trailer's checksum is NOT
        checked; ``decode_ranges_checked`` checks what it returns."""
        return self._decode_ranges(src, src_len, firsts, nbytes, dsts, caps, format, packet_size, index, stream, None, None)

    def decode_ranges_checked(self, src, src_len, firsts, nbytes, dsts, checksums, total_len, caps=None, format=Format.Zlib,
                              packet_size=DEFAULT_PACKET, index=None, stream=None):
        """``decode_ranges`` with what it returns verified; ``checksums`` and ``total_len`` as ``decode_range_checked`` takes
        them. A sidecar that does not fold to the trailer raises E_DATA (nothing is written); a packet that does not match its
        entry fails the reads that return bytes from it (status E_DATA) and leaves the others complete."""
        if checksums is None:
            raise TypeError("decode_ranges_checked needs the stream's packet checksums (packet_checksums())")
        return self._decode_ranges(src, src_len, firsts, nbytes, dsts, caps, format, packet_size, index, stream, checksums, total_len)

    def _decode_ranges(self, src, src_len, firsts, nbytes, dsts, caps, format, packet_size, index, stream, checksums, total_len):
        import torch
        if index is None:
            raise TypeError("decode_ranges needs the stream's packet index (packet_index() or last_decode_index())")
        if not isinstance(index, torch.Tensor) or index.dtype != torch.int64 or index.dim() != 1 or not index.is_contiguous():
            raise TypeError("index must be a contiguous one-dimensional int64 tensor (as packet_index() returns)")
        if index.device.type != "cuda" or index.device.index != self.device:
            raise ValueError(f"index must live on this context's device (cuda:{self.device}), not {index.device}")
        k = len(firsts)
        if len(nbytes) != k or len(dsts) != k:
            raise ValueError(f"{k} starts but {len(nbytes)} lengths and {len(dsts)} destinations")
        if caps is not None and len(caps) != k:
            raise ValueError(f"{len(caps)} capacities for {k} reads")
        side = None
        if checksums is not None:
            side = self._sidecar(checksums, total_len)
            if checksums.numel() != index.numel() - 1:
                raise ValueError(f"{checksums.numel()} checksums for an index of {index.numel() - 1} packets")
        if k == 0:
            return [], []
        d = [self._item(t) for t in dsts]
        cp = [min(int(n), nb) for n, (_, nb) in zip(nbytes, d)] if caps is None else [int(c) for c in caps]
        dev = f"cuda:{self.device}"
        mask = (1 << 64) - 1

        def i64(v):                                    # uint64 values travel as the int64 of the same bits
            v = int(v) & mask
            return v - (1 << 64) if v >> 63 else v
        table = torch.tensor([[i64(v) for v in firsts], [i64(v) for v in nbytes], [i64(p) for p, _ in d], [i64(v) for v in cp]],
                             dtype=torch.int64).to(dev)
        out = torch.empty(k, dtype=torch.int64, device=dev)
        status = torch.empty(k, dtype=torch.int32, device=dev)
        st = self._stream() if stream is None else stream
        if side is not None:
            rc = lib.zz_decode_ranges_checked_device(self._h, self._ptr(src), src_len, int(format), packet_size, index.data_ptr(),
                                                     index.numel(), side[0], side[1], k, table[0].data_ptr(), table[1].data_ptr(),
                                                     table[2].data_ptr(), table[3].data_ptr(), out.data_ptr(), status.data_ptr(), st)
        else:
            rc = lib.zz_decode_ranges_device(self._h, self._ptr(src), src_len, int(format), packet_size, index.data_ptr(), index.numel(),
                                             k, table[0].data_ptr(), table[1].data_ptr(), table[2].data_ptr(), table[3].data_ptr(),
                                             out.data_ptr(), status.data_ptr(), st)
        if rc != 0 and not lib.zz_last_error().startswith(b"reads: "):
            _check(rc)                                 # the call itself failed (the library words a read's own failure "reads: ...")
        status = status.cpu().tolist()
        return [None if sv != 0 else v for v, sv in zip(out.cpu().tolist(), status)], status

    def last_decode_ranges_stats(self):
        """(stage packets decoded over all attempts, attempts, reads that needed more than one attempt, waves) of the last
        ``decode_ranges``."""
        npk, retried, tries, waves = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
        _check(lib.zz_ctx_last_decode_ranges_stats(self._h, ctypes.byref(npk), ctypes.byref(tries), ctypes.byref(retried), ctypes.byref(waves)))
        return npk.value, tries.value, retried.value, waves.value

    def decode_members(self, src, src_len, dst, cap, stream=None):
        """Decode the file of gzip members ``src[:src_len]`` -- one member or many back to back: ``cat a.gz b.gz``, bgzip / BAM
        (BGZF) -- into ``dst`` (``cap`` bytes); returns the decoded length, the members' bytes one after the other. Members that
        announce their length (BGZF's ``BC`` subfield) are decoded in parallel, one wavefront each; any other file serially, at
        a few MB/s. The result is the same either way. Raises ZzFlateError (E_DATA: an invalid member, padding, an empty file;
        E_NOSPACE: the bytes do not fit ``cap``)."""
        out = ctypes.c_uint64(0)
        st = self._stream() if stream is None else stream
        _check(lib.zz_decode_members_device(self._h, self._ptr(src), src_len, self._ptr(dst), cap, ctypes.byref(out), st))
        return out.value

    def last_decode_members_stats(self):
        """(members, header-like offsets found, path) of the last ``decode_members``; path is MEMBERS_BLOCKED (chain verified
        in parallel), MEMBERS_WALKED (chain walked by one lane) or MEMBERS_SERIAL."""
        m, cand, path = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0)
        _check(lib.zz_ctx_last_decode_members_stats(self._h, ctypes.byref(m), ctypes.byref(cand), ctypes.byref(path)))
        return m.value, cand.value, path.value

    def members_index(self, src, src_len, stream=None):
        """The index of the blocked gzip (BGZF) file ``src[:src_len]``, made on the device from the file alone: an int64 tensor of
        shape ``[members + 1, 2]`` on this context's device -- (file offset, decoded offset) of every member's first byte, then
        (the offset behind the last member, the decoded length). Nothing is decoded: the decoded offsets are the members' own
        claims, which ``decode_members_ranges`` checks. Raises ZzFlateError (E_UNSUPPORTED: the file is not blocked --
        ``decode_members`` decodes it; E_DATA: an empty file)."""
        import torch
        entries = ctypes.c_uint64(0)
        st = self._stream() if stream is None else stream
        rc = lib.zz_members_index_device(self._h, self._ptr(src), src_len, None, 0, ctypes.byref(entries), st)
        if rc != E_NOSPACE:
            _check(rc)
        idx = torch.empty((entries.value, 2), dtype=torch.int64, device=f"cuda:{self.device}")
        _check(lib.zz_members_index_device(self._h, self._ptr(src), src_len, idx.data_ptr(), entries.value, ctypes.byref(entries), st))
        return idx

    def members_find(self, src, limit_bytes=0, src_len=None, stream=None):
        """The index of ANY file of gzip members ``src`` (a uint8 tensor on this context's device; ``src_len`` defaults to its
        length) -- ``cat a.gz b.gz``, append-mode logs, WARC: members that announce no length. Every place where a gzip header
        stands is measured as a member without writing a byte, in parallel, and the chain from offset 0 picks the members.
        Returns ``members_index``'s tensor, ``[members + 1, 2]`` int64 on this context's device, with measured decoded offsets;
        ``decode_members_ranges`` reads through it. ``limit_bytes`` (0: 1 MiB) bounds what a false start may cost before it is
        given up; the result does not depend on it. Checksums are not judged here: a read or a decode does that. Raises
        ZzFlateError (E_DATA: the file is no chain of members, or empty)."""
        import torch
        n = src.numel() if src_len is None else src_len
        entries = ctypes.c_uint64(0)
        st = self._stream() if stream is None else stream
        rc = lib.zz_members_find_device(self._h, self._ptr(src), n, limit_bytes, None, 0, ctypes.byref(entries), st)
        if rc != E_NOSPACE:
            _check(rc)
        idx = torch.empty((entries.value, 2), dtype=torch.int64, device=f"cuda:{self.device}")
        _check(lib.zz_members_find_device(self._h, self._ptr(src), n, limit_bytes, idx.data_ptr(), entries.value, ctypes.byref(entries), st))
        return idx

    def decode_members_found(self, src, cap=None, src_len=None, dst=None, stream=None):
        """``decode_members`` for files whose members announce no length: the members are found as ``members_find`` finds them
        and decoded in parallel, one wavefront each. The verdict and the bytes are ``decode_members``' for every input; only the
        speed differs. Returns the decoded bytes, a uint8 tensor on this context's device: a view of ``dst`` (``cap`` defaults to
        its length) when that is given, else of a new tensor of ``cap`` bytes -- ``cap=None`` measures the file first
        (``members_find``) and takes its decoded length. Raises ZzFlateError (E_DATA, E_NOSPACE) as ``decode_members`` does."""
        import torch
        n = src.numel() if src_len is None else src_len
        if dst is not None:
            if not isinstance(dst, torch.Tensor) or dst.dtype != torch.uint8 or not dst.is_contiguous():
                raise TypeError("dst must be a contiguous uint8 tensor")
            cap = dst.numel() if cap is None else cap
        else:
            if cap is None:
                cap = int(self.members_find(src, 0, n, stream)[-1, 1])
            dst = torch.empty(cap, dtype=torch.uint8, device=f"cuda:{self.device}")
        out = ctypes.c_uint64(0)
        st = self._stream() if stream is None else stream
        _check(lib.zz_decode_members_found_device(self._h, self._ptr(src), n, dst.data_ptr(), cap, ctypes.byref(out), st))
        return dst[:out.value]

    def last_members_find_stats(self):
        """(members, candidates, dropped candidates, rounds) of the last ``members_find`` or ``decode_members_found``."""
        m, cand, dropped, rounds = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
        _check(lib.zz_ctx_last_members_find_stats(self._h, ctypes.byref(m), ctypes.byref(cand), ctypes.byref(dropped), ctypes.byref(rounds)))
        return m.value, cand.value, dropped.value, rounds.value

    def members_points(self, src, chunk_bytes=POINTS_CHUNK, spacing=1, src_len=None, stream=None):
        """The member point index of ANY file of gzip members ``src`` (a uint8 tensor on this context's device; ``src_len``
        defaults to its length): ``members_find``'s members AND ``points_index``'s block starts inside them, found together: the
        cuts at which a file of few large members can be decoded with many wavefronts per member. Returns ``(points, decoded_length)`` with
        ``points`` an ``(entries, 2)`` int64 CPU tensor of rows (in_bit, out_byte), bits counted from the file's first byte:
        per member a START row (``MP_START`` set in in_bit), its inner rows, an END row (``MP_END``).
        ``members_index_from_points`` gives ``members_find``'s index from it. ``spacing`` > 1
        thins inner rows only. Checksums and distances are NOT judged here (no byte is produced). Raises ZzFlateError (E_DATA:
        the file is no chain of members, or empty)."""
        import torch
        n = src.numel() if src_len is None else src_len
        entries, total = ctypes.c_uint64(0), ctypes.c_uint64(0)
        st = self._stream() if stream is None else stream
        rc = lib.zz_members_points_device(self._h, self._ptr(src), n, chunk_bytes, spacing, None, 0, ctypes.byref(entries), ctypes.byref(total), st)
        if rc != E_NOSPACE:
            _check(rc)
        points = torch.zeros((entries.value, 2), dtype=torch.int64)
        _check(lib.zz_members_points_device(self._h, self._ptr(src), n, chunk_bytes, spacing, points.data_ptr(), points.shape[0],
                                            ctypes.byref(entries), ctypes.byref(total), st))
        return points[: entries.value], total.value

    def last_members_points_stats(self):
        """(members, header candidates, block candidates, dropped candidates, rounds) of the last ``members_points``."""
        m, hc, bc, dropped, rounds = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
        _check(lib.zz_ctx_last_members_points_stats(self._h, ctypes.byref(m), ctypes.byref(hc), ctypes.byref(bc), ctypes.byref(dropped),
                                                    ctypes.byref(rounds)))
        return m.value, hc.value, bc.value, dropped.value, rounds.value

    def decode_members_points(self, src, points=None, cap=None, src_len=None, dst=None, batch_bytes=0, stream=None):
        """``decode_members`` for files of LARGE members -- ``cat lane1.fq.gz lane2.fq.gz``, rotated logs joined with cat -- through
        a member point index: many wavefronts per member, where ``decode_members_found`` has one. ``points`` are ``members_points``'
        rows, an ``(entries, 2)`` int64 CPU tensor (or anything ``torch.as_tensor`` makes one of); ``None``: the call makes the
        index itself. The rows are never trusted: the verdict and the bytes are ``decode_members``' for every input and every row
        array, true, thinned or lying; only the speed differs. ``batch_bytes`` is the most decoded bytes in a batch (0: 64 MiB).
        Returns the decoded bytes, a uint8 tensor on this context's device: a view of ``dst`` (``cap`` defaults to its length) when
        that is given, else of a new tensor of ``cap`` bytes -- ``cap=None`` takes the decoded length from ``members_points``
        (which is then also the index used when ``points`` is None). Raises ZzFlateError (E_DATA, E_NOSPACE) as ``decode_members``
        does, TypeError for rows that are no ``(entries, 2)`` int64 array."""
        import torch
        n = src.numel() if src_len is None else src_len
        if dst is not None:
            if not isinstance(dst, torch.Tensor) or dst.dtype != torch.uint8 or not dst.is_contiguous():
                raise TypeError("dst must be a contiguous uint8 tensor")
            cap = dst.numel() if cap is None else cap
        if points is not None:
            points = torch.as_tensor(points)
            if points.dtype != torch.int64 or points.dim() != 2 or points.shape[1] != 2 or points.device.type != "cpu":
                raise TypeError("points must be an (entries, 2) int64 CPU tensor")
            points = points.contiguous()
        if dst is None:
            if cap is None:
                made, cap = self.members_points(src, POINTS_CHUNK, 1, n, stream)
                points = made if points is None else points
            dst = torch.empty(cap, dtype=torch.uint8, device=f"cuda:{self.device}")
        out = ctypes.c_uint64(0)
        st = self._stream() if stream is None else stream
        rows, entries = (None, 0) if points is None else (points.data_ptr(), points.shape[0])
        _check(lib.zz_decode_members_points_device(self._h, self._ptr(src), n, dst.data_ptr(), cap, ctypes.byref(out), rows, entries,
                                                   batch_bytes, st))
        return dst[:out.value]

    def last_decode_members_points_stats(self):
        """(members the rows name, members proven in front of the serial tail, segments dealt, batches, pending bytes, rounds,
        serial) of the last ``decode_members_points``; serial is 1 if the serial path ran (from the first member not proven)."""
        m, proven, segs, pend = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        batches, rounds, serial = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_int(0)
        _check(lib.zz_ctx_last_decode_members_points_stats(self._h, ctypes.byref(m), ctypes.byref(proven), ctypes.byref(segs),
                                                           ctypes.byref(batches), ctypes.byref(pend), ctypes.byref(rounds), ctypes.byref(serial)))
        return m.value, proven.value, segs.value, batches.value, pend.value, rounds.value, serial.value

    def _reads(self, call, firsts, nbytes, dsts, caps, stream):
        """the read arrays of decode_members_ranges and decode_points_ranges on the device, the call, and (lens, status) back"""
        import torch
        k = len(firsts)
        if len(nbytes) != k or len(dsts) != k:
            raise ValueError(f"{k} starts but {len(nbytes)} lengths and {len(dsts)} destinations")
        if caps is not None and len(caps) != k:
            raise ValueError(f"{len(caps)} capacities for {k} reads")
        if k == 0:
            return [], []
        d = [self._item(t) for t in dsts]
        cp = [min(int(n), nb) for n, (_, nb) in zip(nbytes, d)] if caps is None else [int(c) for c in caps]
        dev = f"cuda:{self.device}"
        mask = (1 << 64) - 1

        def i64(v):                                    # uint64 values travel as the int64 of the same bits
            v = int(v) & mask
            return v - (1 << 64) if v >> 63 else v
        table = torch.tensor([[i64(v) for v in firsts], [i64(v) for v in nbytes], [i64(p) for p, _ in d], [i64(v) for v in cp]],
                             dtype=torch.int64).to(dev)
        out = torch.empty(k, dtype=torch.int64, device=dev)
        status = torch.empty(k, dtype=torch.int32, device=dev)
        st = self._stream() if stream is None else stream
        rc = call(k, table[0].data_ptr(), table[1].data_ptr(), table[2].data_ptr(), table[3].data_ptr(), out.data_ptr(), status.data_ptr(), st)
        if rc != 0 and not lib.zz_last_error().startswith(b"reads: "):
            _check(rc)                                 # the call itself was refused (the library words a read's own failure "reads: ...")
        status = status.cpu().tolist()
        return [None if sv != 0 else v for v, sv in zip(out.cpu().tolist(), status)], status

    def decode_members_ranges(self, src, src_len, index, firsts, nbytes, dsts, caps=None, stream=None):
        """Many reads of one blocked gzip (BGZF) file in one call: read r = decoded bytes ``[firsts[r], firsts[r] + nbytes[r])``
        of the file ``src[:src_len]`` into ``dsts[r]``. ``index`` is an int64 tensor of shape ``[members + 1, 2]`` on this
        context's device (``members_index``, or ``members_index_from_offsets`` moved there); ``dsts`` are items as
        ``decode_batch`` takes them; ``caps`` defaults to ``min(nbytes[r], destination size)``. Returns ``(lens, status)``:
        ``lens[r]`` the bytes read (clipped at the file's decoded length) or ``None``, ``status[r]`` 0, E_ARG, E_NOSPACE, E_DATA
        or E_UNSUPPORTED -- a read's own failure does not raise and leaves the others complete; an index that is not an index
        gives every read E_DATA; only a refused call (arguments) raises. Every member a read touches is decoded whole and
        checked completely: CRC-32, ISIZE and the length the index gives it."""
        import torch
        if not isinstance(index, torch.Tensor) or index.dtype != torch.int64 or index.dim() != 2 or index.shape[1] != 2 or not index.is_contiguous():
            raise TypeError("index must be a contiguous int64 tensor of shape [members + 1, 2] (as members_index() returns)")
        if index.device.type != "cuda" or index.device.index != self.device:
            raise ValueError(f"index must live on this context's device (cuda:{self.device}), not {index.device}")
        def call(k, firsts, nbytes, dsts, caps, out, status, st):
            return lib.zz_decode_members_ranges_device(self._h, self._ptr(src), src_len, index.data_ptr(), index.shape[0],
                                                       k, firsts, nbytes, dsts, caps, out, status, st)
        return self._reads(call, firsts, nbytes, dsts, caps, stream)

    def last_decode_members_ranges_stats(self):
        """(members decoded, each once; waves) of the last ``decode_members_ranges``."""
        m, waves = ctypes.c_uint64(0), ctypes.c_uint32(0)
        _check(lib.zz_ctx_last_decode_members_ranges_stats(self._h, ctypes.byref(m), ctypes.byref(waves)))
        return m.value, waves.value

    def decode_points_ranges(self, src, src_len, points, windows, sums, firsts, nbytes, dsts, caps=None, format=Format.Zlib, stream=None):
        """Many reads of one zlib / gzip / raw stream this library need not have written, in one call: read r = decoded bytes
        ``[firsts[r], firsts[r] + nbytes[r])`` of the stream ``src[:src_len]`` into ``dsts[r]``. ``points`` (int64
        ``[segments + 1, 2]``), ``windows`` (uint8 ``[segments, 32768]``) and ``sums`` (int32 ``[segments]``) are
        ``points_index_host`` and ``points_windows_host``'s tensors moved to this context's device; ``dsts``, ``caps`` and the
        result ``(lens, status)`` are ``decode_members_ranges``'. Every segment a read touches is decoded whole against its
        window and held to its checksum, and the checksums to the stream's trailer: a wrong index or sidecar gives E_DATA, never
        wrong bytes; one that fails as a whole gives every read E_DATA. Only a refused call (arguments, a preset dictionary) raises."""
        import torch
        _points_tensor(points, "cuda")
        segments = points.shape[0] - 1
        if not isinstance(windows, torch.Tensor) or windows.dtype != torch.uint8 or tuple(windows.shape) != (segments, POINTS_WINDOW) or not windows.is_contiguous():
            raise TypeError(f"windows must be a contiguous uint8 tensor of shape [{segments}, {POINTS_WINDOW}] (as points_windows_host() returns)")
        if not isinstance(sums, torch.Tensor) or sums.dtype != torch.int32 or tuple(sums.shape) != (segments,) or not sums.is_contiguous():
            raise TypeError(f"sums must be a contiguous int32 tensor of shape [{segments}] (as points_windows_host() returns)")
        for name, t in (("points", points), ("windows", windows), ("sums", sums)):
            if t.device.type != "cuda" or t.device.index != self.device:
                raise ValueError(f"{name} must live on this context's device (cuda:{self.device}), not {t.device}")
        def call(k, firsts, nbytes, dsts, caps, out, status, st):
            return lib.zz_decode_points_ranges_device(self._h, self._ptr(src), src_len, int(format), points.data_ptr(), points.shape[0],
                                                      windows.data_ptr(), sums.data_ptr(), k, firsts, nbytes, dsts, caps, out, status, st)
        return self._reads(call, firsts, nbytes, dsts, caps, stream)

    def decode_points_range(self, src, src_len, points, windows, sums, first, nbytes, dst, cap=None, format=Format.Zlib, stream=None):
        """One read through ``decode_points_ranges``: the bytes read (clipped at the decoded length); raises ZzFlateError on failure."""
        lens, status = self.decode_points_ranges(src, src_len, points, windows, sums, [first], [nbytes], [dst],
                                                 None if cap is None else [cap], format=format, stream=stream)
        if status[0] != 0:
            raise ZzFlateError(status[0], lib.zz_last_error().decode())
        return lens[0]

    def last_decode_points_ranges_stats(self):
        """(segments decoded, each once; waves) of the last ``decode_points_ranges``."""
        m, waves = ctypes.c_uint64(0), ctypes.c_uint32(0)
        _check(lib.zz_ctx_last_decode_points_ranges_stats(self._h, ctypes.byref(m), ctypes.byref(waves)))
        return m.value, waves.value

    def last_decode_path(self):
        """DECODE_INDEXED, DECODE_DISCOVERED, DECODE_SERIAL or DECODE_POINTS: the path the last decode finished on (0: none)."""
        return lib.zz_ctx_last_decode_path(self._h)

    def last_decode_index(self, stream=None):
        """The packet index the last decode recovered by discovery (an int64 tensor like packet_index()), or None when
        the last decode took another path."""
        import torch
        if self.last_decode_path() != DECODE_DISCOVERED:
            return None
        entries = ctypes.c_uint64(0)
        st = self._stream() if stream is None else stream
        lib.zz_ctx_last_decode_index_device(self._h, None, 0, ctypes.byref(entries), st)
        idx = torch.empty(entries.value, dtype=torch.int64, device=f"cuda:{self.device}")
        _check(lib.zz_ctx_last_decode_index_device(self._h, idx.data_ptr(), entries.value, ctypes.byref(entries), st))
        return idx

    def last_decode_stats(self):
        """(pending bytes, pointer-jumping rounds) of the last decode's parallel path."""
        pend, rounds = ctypes.c_uint64(0), ctypes.c_uint32(0)
        _check(lib.zz_ctx_last_decode_stats(self._h, ctypes.byref(pend), ctypes.byref(rounds)))
        return pend.value, rounds.value

    def generate(self, kind, seed, first_byte, buf, n, stream=None):
        st = self._stream() if stream is None else stream
        _check(lib.zz_generate_device(self._h, kind, seed, first_byte, self._ptr(buf), n, st))


def encode_multi(ctxs, srcs, ns, dst, cap, format=Format.Zlib, level=1, packet_size=DEFAULT_PACKET, halos=None):
    """zz_encode_multi_device: shard i = srcs[i][:ns[i]] on the device of ctxs[i]; the whole stream (header, shards in
    order, trailer) lands in `dst` on the device of ctxs[0]. One process, no torch.distributed. Returns the byte count."""
    k = len(ctxs)
    vp = ctypes.c_void_p
    cs = (vp * k)(*[c._h for c in ctxs])
    ps = (vp * k)(*[Context._ptr(t) for t in srcs])
    nn = (ctypes.c_uint64 * k)(*ns)
    hh = (ctypes.c_uint64 * k)(*(halos or [0] * k))
    out = ctypes.c_uint64(0)
    _check(lib.zz_encode_multi_device(cs, k, ps, nn, hh, Context._ptr(dst), cap, ctypes.byref(out), int(format), int(level), packet_size))
    return out.value
