"""The database-image entry points (kq_export_map_images / kq_import_map_image) as far as they run without a GPU: the
symbols, the argument checks in front of any device work, and the reader's host-side header walk, which refuses a
malformed image before it looks at the handle."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from kreeq_amd import build, capi
from tests.helpers import ROOT

INVALID = -1
EMPTY_MAP = struct.pack("<Q", 256) + struct.pack("<QQQ", 0xFFFFFFFFFFFFFFF5, 0, 0) * 256        # 6152 bytes


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return capi.load()


def last_error(lib):
    return lib.kq_last_error().decode()


def import_image(lib, image, handle=None, with_counts=True):
    buf = np.frombuffer(image + b"\0", dtype=np.uint8)          # (one byte more than is offered: an empty image still has an address)
    n, t = C.c_uint64(7), C.c_uint64(7)
    rc = lib.kq_import_map_image(handle, 0, buf.ctypes.data_as(C.c_void_p), len(image), C.byref(n) if with_counts else None, C.byref(t))
    return rc, n.value, t.value


def test_symbols_and_abi(lib):
    assert {"kq_export_map_images", "kq_import_map_image"} <= set(capi.SYMBOLS)
    assert hasattr(lib, "kq_export_map_images") and hasattr(lib, "kq_import_map_image")
    assert hasattr(capi.KreeqDB, "export_map_images") and hasattr(capi.KreeqDB, "import_map_image")
    assert lib.kq_abi_version() == 4


def test_export_arguments_checked_before_the_device(lib):
    off = np.zeros(129, dtype=np.uint64)
    n_hc = C.c_uint64(0)
    p_off = off.ctypes.data_as(C.c_void_p)
    assert lib.kq_export_map_images(None, 0, 128, None, 0, None, None, 0, C.byref(n_hc)) == INVALID and "offsets" in last_error(lib)
    assert lib.kq_export_map_images(None, 0, 128, None, 0, p_off, None, 0, None) == INVALID and "n_hc" in last_error(lib)
    assert lib.kq_export_map_images(None, 9, 5, None, 0, p_off, None, 0, C.byref(n_hc)) == INVALID and "reversed" in last_error(lib)
    assert lib.kq_export_map_images(None, 0, 128, None, 0, p_off, None, 0, C.byref(n_hc)) == INVALID and "null handle" in last_error(lib)


def test_import_null_arguments(lib):
    rc, _, _ = import_image(lib, EMPTY_MAP, with_counts=False)
    assert rc == INVALID and "n_entries" in last_error(lib)
    n, t = C.c_uint64(0), C.c_uint64(0)
    assert lib.kq_import_map_image(None, 0, None, 6152, C.byref(n), C.byref(t)) == INVALID


def test_header_walk_runs_in_front_of_the_handle(lib):
    """a well-formed image gets as far as the (null) handle; every header defect is reported first, without a device"""
    assert len(EMPTY_MAP) == 6152
    rc, n, t = import_image(lib, EMPTY_MAP)
    assert rc == INVALID and "null handle" in last_error(lib) and (n, t) == (0, 0)
    cases = {
        "truncated": EMPTY_MAP[:-1],
        "trailing": EMPTY_MAP + b"\0",
        "version": EMPTY_MAP[:8 + 24 * 100] + struct.pack("<Q", 0xFFFFFFFFFFFFFFF4) + EMPTY_MAP[8 + 24 * 100 + 8:],
        "256 submaps": struct.pack("<Q", 255) + EMPTY_MAP[8:],
        # size 1 / capacity 1 announced, but no control bytes, slot or growth word follow
        "truncated ": EMPTY_MAP[:8 + 24 * 255] + struct.pack("<QQQ", 0xFFFFFFFFFFFFFFF5, 1, 1),
        # capacity that is no 2^n - 1
        "inconsistent": EMPTY_MAP[:8 + 24 * 255] + struct.pack("<QQQ", 0xFFFFFFFFFFFFFFF5, 1, 2) + b"\x80" * 19 + b"\0" * 48 + b"\0" * 8,
        "": b"",
    }
    for word, image in cases.items():
        rc, n, t = import_image(lib, image)
        assert rc == INVALID, word
        assert "null handle" not in last_error(lib), word
        assert (word.strip() or "truncated") in last_error(lib), (word, last_error(lib))


def test_header_walk_under_sanitizers(tmp_path, golden_dbs):
    """the walk and its bound checks as a stand-alone program built with -fsanitize=address,undefined, over the golden map
    files and the malformed variants the program derives from them"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "dbimage_walk")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "kreeq_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "native", "dbimage_walk_main.cpp")])
    files = []
    for db in sorted(os.listdir(golden_dbs)):
        d = os.path.join(golden_dbs, db)
        if os.path.isdir(d):
            files += [os.path.join(d, f".map.{m}.bin") for m in (0, 64, 127)]
    assert len(files) == 30
    p = subprocess.run([exe] + files, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert f"{len(files)} files" in p.stdout
