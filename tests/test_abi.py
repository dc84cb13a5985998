"""The C-ABI library loads and exports every symbol include/zzflate_amd.h declares, plus the reference's
mangled C++ entry points; host-side utilities behave; no compute is attempted without a GPU."""
import ctypes
import os
import re
import subprocess

import pytest

import zzflate_amd as zz
from conftest import ROOT


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "zzflate_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(zz_[a-z0-9_]+)\s*\(", text)) - {"zz_callback"})


def test_exports_every_declared_symbol():
    syms = declared_symbols()
    assert len(syms) >= 20
    L = ctypes.CDLL(zz._build.LIB)
    for s in syms:
        assert hasattr(L, s), s


def test_reference_cxx_symbols_present():
    """zzflate.h:17,19 + adler.cpp + crc.h: same Itanium names as the reference's own objects."""
    out = subprocess.run(["nm", "-D", "--defined-only", zz._build.LIB], capture_output=True, text=True, check=True).stdout
    for s in ("_Z13ZzFlateEncodePhPmPKhmPK6Config", "_Z23ZzFlateEncodeToCallbackPKhmPK6ConfigSt8functionIFbS0_mEE",
              "_Z8adler32xjPKhm", "_Z7combinejjm", "_Z5crc32PKhmj"):
        assert s in out, s


def test_config_layout():
    assert ctypes.sizeof(zz._CConfig) == 8   # zzflate.h:10-15, [probed] in SURVEY 8b
    assert zz._CConfig.level.offset == 4 and zz._CConfig.threaded.offset == 5


def test_container_pieces():
    assert zz.header(zz.Format.Zlib) == bytes([0x78, 0x01])                       # zzflate.cpp:30-36
    assert zz.header(zz.Format.Gzip) == bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff])   # zzflate.cpp:28
    assert zz.header(zz.Format.Deflate) == b""
    assert zz.trailer(zz.Format.Zlib, 0x11223344, 5) == bytes([0x11, 0x22, 0x33, 0x44])
    assert zz.trailer(zz.Format.Gzip, 0x11223344, 0x1_0000_0005) == bytes([0x44, 0x33, 0x22, 0x11, 5, 0, 0, 0])


def test_bound_covers_worst_case():
    for n in (0, 1, 32767, 32768, 32769, 1 << 20):
        for lvl in range(4):
            assert zz.bound(n, zz.Format.Gzip, lvl) >= n + 18
    # the per-packet term against the worst packets in closed form (tests/expansion_cases.py; the oracle's own packets are held to it
    # in tests/test_expansion_cases_cpu.py): nine bits a byte at level 1, the stored fallback above, level 0's len + 10
    import expansion_cases as ec
    for L in ec.LENGTHS:
        assert ec.per_packet(0, L) >= (L + 10 if L > 1 else 6)
        assert ec.per_packet(1, L) >= max(ec.level1_packet_bytes(L, True), ec.level1_packet_bytes(L, False))
        for lvl in range(2, 7):
            assert ec.per_packet(lvl, L) >= ec.stored_packet_bytes(L, False)
        for fmt in zz.Format:
            assert zz.bound(3 * L + 1, fmt, 1, L) >= ec.HEADER[fmt] + 3 * ec.level1_packet_bytes(L, False) + 3 + ec.TRAILER[fmt]


def test_generators_are_deterministic_and_blockwise():
    a = zz.generate_host(zz.GEN_TEXT, 0x5EED0002, 0, 200000)
    b = zz.generate_host(zz.GEN_TEXT, 0x5EED0002, 65536, 100000)
    assert a[65536:165536] == b
    assert zz.generate_host(zz.GEN_RANDOM, 3, 0, 1000) != zz.generate_host(zz.GEN_RANDOM, 4, 0, 1000)
    import zlib
    t = zz.generate_host(zz.GEN_TEXT, 1, 0, 1 << 20)
    r = zz.generate_host(zz.GEN_RANDOM, 1, 0, 1 << 18)
    lg = zz.generate_host(zz.GEN_LOG, 1, 0, 1 << 20)
    assert 0.35 < len(zlib.compress(t, 1)) / len(t) < 0.75
    assert len(zlib.compress(r, 1)) > len(r)
    assert len(zlib.compress(lg, 1)) / len(lg) < 0.5


def test_no_cpu_fallback_without_gpu():
    """Without a HIP device the encode entry points must fail loudly (no silent CPU path)."""
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("GPU present")
    except ImportError:
        pass
    with pytest.raises(zz.ZzFlateError):
        zz.ZzFlateEncode(b"hello", zz.Config())
    with pytest.raises(zz.ZzFlateError):
        zz.Context(0)


def test_lds_order_guard_hook_answers_without_a_device():
    """The run-time guard for the undocumented LDS ordering (zz_api.hip lds_order_ok): a forced verdict is answered from the host
    alone, so the refusal path can be driven from a test; the un-forced probe needs a GPU (tests/test_gpu_parity.py)."""
    L = ctypes.CDLL(zz._build.LIB)
    L.zz_debug_lds_order_verdict.restype = ctypes.c_int
    try:
        L.zz_debug_force_lds_order(ctypes.c_int(0))
        assert L.zz_debug_lds_order_verdict(ctypes.c_int(0)) == 0
        L.zz_debug_force_lds_order(ctypes.c_int(1))
        assert L.zz_debug_lds_order_verdict(ctypes.c_int(0)) == 1
    finally:
        L.zz_debug_force_lds_order(ctypes.c_int(-1))


def test_shipped_library_carries_no_experiment_switch():
    """zz_build_flags() names the switches that change what a build computes or records: cycle stamps (ZZ_PROF) and the test
    build's ZZ_ST_ALWAYS_CAREFUL (the wrong-stream timing experiments it once guarded against are gone from the source). The library
    the package loads must be built without either, and the test build must own up to its one."""
    L = ctypes.CDLL(zz._build.LIB)
    L.zz_build_flags.restype = ctypes.c_char_p
    assert L.zz_build_flags() == b"", L.zz_build_flags()
    assert zz.lib.zz_build_flags() == b"" or os.environ.get("ZZFLATE_AMD_LIB"), zz.lib.zz_build_flags()
    careful = zz._build.CAREFUL_LIB
    if os.path.exists(careful):
        C = ctypes.CDLL(careful)
        C.zz_build_flags.restype = ctypes.c_char_p
        assert C.zz_build_flags().split() == [b"ZZ_ST_ALWAYS_CAREFUL"]


def macros_in_conditionals():
    """the macro names that a #if / #ifdef / #ifndef / #elif of zzflate_amd/csrc/* tests (the compiler's own __... ones left out)"""
    names = set()
    csrc = os.path.join(ROOT, "zzflate_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        text = open(os.path.join(csrc, f)).read().replace("\\\n", " ")
        for m in re.finditer(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b(.*)$", text, flags=re.M):
            expr = re.sub(r"//.*|/\*.*?\*/", "", m.group(1))
            names.update(n for n in re.findall(r"[A-Za-z_]\w*", expr) if n != "defined" and not n.startswith("__"))
    return names


def switches_in_design_md():
    """the names in the first column of DESIGN.md's "Compile-time switches" table; every row also has a default and a builder"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = re.search(r"^### Compile-time switches\n(.*?)(?=^#)", text, flags=re.M | re.S).group(1)
    rows = [r for r in section.splitlines() if r.startswith("|")][2:]        # (behind the head and its rule)
    names = []
    for r in rows:
        cells = [c.strip() for c in r.strip().strip("|").split("|")]
        assert len(cells) == 3 and all(cells), r
        found = re.findall(r"`([A-Za-z_]\w*)`", cells[0])
        assert found, r
        names += found
    assert len(names) == len(set(names)), names
    return set(names)


def test_compile_time_switches_are_the_documented_ones():
    """Every macro the sources test in a conditional is in DESIGN.md's "Compile-time switches" table (name, default, who builds
    it), and the table lists nothing else: an experiment switch is written down or does not go in, and a retired one leaves both."""
    tested, listed = macros_in_conditionals(), switches_in_design_md()
    assert len(tested) >= 10
    assert tested == listed, {"not in DESIGN.md": sorted(tested - listed), "not in the source": sorted(listed - tested)}


def test_product_does_not_touch_oracle():
    """The shipped package must not import, link or open anything under oracle/."""
    pkg = os.path.join(ROOT, "zzflate_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cpp")):
                text = open(os.path.join(root, f)).read()
                assert "zzoracle" not in text and "zzref" not in text and "oracle/" not in text.replace("the oracle", ""), f
    out = subprocess.run(["ldd", zz._build.LIB], capture_output=True, text=True).stdout
    assert "zzoracle" not in out and "zzref" not in out
