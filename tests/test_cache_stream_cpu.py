"""CPU: the container half of include/mcd_cache.h (csrc/mcd_host.c, libmcd_host.so) -- the activation-cache files built from rows
that arrive in pieces -- and the header's ABI surface.

A cache file is laid out by torch.save with placeholder data (utils._placeholder_archive); mcd_cachefile_* write the rows over the
placeholder, keep the CRC-32 and finalise.  What is asserted: torch.load gives back the source's BYTES (NaN payloads, infinities
and -0.0 included), the archive passes zipfile's CRC check, files exist under their final name only when complete, and
mcd_zip_crc32 is zlib.crc32.  The last test compiles mcd_host.c with a stand-alone C program (tests/native/cache_host_check.c)
under AddressSanitizer and UBSan and runs that program: nothing sanitised is loaded into Python."""
import ctypes
import os
import re
import shutil
import subprocess
import zipfile
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mammo-clip-dissect_amd", "csrc")

# (N, U, pieces): the pieces are uneven and sum to N
CASES = [(5, 3, (2, 3)), (257, 768, (100, 100, 57)), (1, 1, (1,))]


@pytest.fixture(scope="module")
def H(mcd):
    L = mcd._lib.load_cache_host()
    assert L is not None, "libmcd_host.so must be built (make -C mammo-clip-dissect_amd/csrc)"
    return L


def source(n, u):
    """float32 [n, u] as raw bits: random words -- so NaNs of every payload, denormals and both zeros occur at the larger sizes --
    with the special values planted at the front."""
    rng = np.random.default_rng(1000 * n + u)
    bits = rng.integers(0, 2 ** 32, size=(n, u), dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7fc00000, 0xffc00001, 0x7f800001, 0x7fffffff, 0x7f800000, 0xff800000, 0x80000000, 0x00000000, 0x00000001],
                       dtype=np.uint32)
    flat = bits.reshape(-1)
    k = min(flat.size, special.size)
    flat[:k] = special[:k]
    return bits


def open_file(H, utils, path, n, u):
    part = path + ".part"
    data_off, crc_a, crc_b = utils._placeholder_archive(part, n, u)
    h = ctypes.c_void_p()
    rc = H.mcd_cachefile_open(os.fsencode(part), os.fsencode(path), n, u, data_off, crc_a, crc_b, ctypes.byref(h))
    assert rc == 0, H.mcd_cachefile_last_error()
    return h


def append(H, h, bits, row0, n):
    piece = np.ascontiguousarray(bits[row0:row0 + n])
    return H.mcd_cachefile_append(h, piece.ctypes.data, row0, n)


@pytest.mark.parametrize("n,u,pieces", CASES, ids=lambda v: str(v))
def test_file_from_uneven_pieces(H, mcd, tmp_path, n, u, pieces):
    from mammo_clip_dissect_amd.concept_vit import utils
    assert sum(pieces) == n
    bits = source(n, u)
    path = str(tmp_path / "acts.pt")
    h = open_file(H, utils, path, n, u)
    assert not os.path.exists(path) and os.path.exists(path + ".part")
    row0 = 0
    for p in pieces:
        assert append(H, h, bits, row0, p) == 0, H.mcd_cachefile_last_error()
        row0 += p
    assert H.mcd_cachefile_close(h) == 0, H.mcd_cachefile_last_error()
    assert os.listdir(str(tmp_path)) == ["acts.pt"]                                  # no .part left behind
    t = torch.load(path, weights_only=True)
    assert t.dtype == torch.float32 and tuple(t.shape) == (n, u) and t.is_contiguous()
    assert t.numpy().view(np.uint32).tobytes() == bits.tobytes()
    with zipfile.ZipFile(path) as z:
        assert z.testzip() is None
        rec = [i for i in z.infolist() if i.filename.endswith("/data/0")]
        assert len(rec) == 1 and rec[0].CRC == zlib.crc32(bits.tobytes())
    # and the file is what a plain torch.save of the same tensor loads to
    ref = str(tmp_path / "ref.pt")
    torch.save(torch.from_numpy(bits.view(np.float32)), ref)
    assert torch.load(ref, weights_only=True).numpy().view(np.uint32).tobytes() == bits.tobytes()


def test_append_past_the_last_row_is_an_error(H, mcd, tmp_path):
    from mammo_clip_dissect_amd.concept_vit import utils
    n, u = 5, 3
    bits = source(n + 2, u)
    path = str(tmp_path / "acts.pt")
    h = open_file(H, utils, path, n, u)
    assert append(H, h, bits, 0, 2) == 0
    assert append(H, h, bits, 2, 4) != 0                      # 2 + 4 > 5
    assert b"more rows" in H.mcd_cachefile_last_error()
    assert append(H, h, bits, 3, 1) != 0                      # out of order
    assert not os.path.exists(path)
    # the refused pieces wrote nothing and did not move the CRC: the file can still be completed
    assert append(H, h, bits, 2, 3) == 0
    assert H.mcd_cachefile_close(h) == 0
    assert torch.load(path, weights_only=True).numpy().view(np.uint32).tobytes() == bits[:n].tobytes()
    with zipfile.ZipFile(path) as z:
        assert z.testzip() is None


def test_close_before_all_rows_is_an_error(H, mcd, tmp_path):
    from mammo_clip_dissect_amd.concept_vit import utils
    n, u = 5, 3
    bits = source(n, u)
    path = str(tmp_path / "acts.pt")
    h = open_file(H, utils, path, n, u)
    assert append(H, h, bits, 0, 2) == 0
    assert H.mcd_cachefile_close(h) != 0
    assert b"2 of 5 rows" in H.mcd_cachefile_last_error()
    assert os.listdir(str(tmp_path)) == []                   # neither the final name nor the .part file
    h = open_file(H, utils, path, n, u)
    H.mcd_cachefile_abort(h)
    assert os.listdir(str(tmp_path)) == []


def test_open_refuses_what_does_not_fit(H, tmp_path):
    part = str(tmp_path / "short.pt.part")
    with open(part, "wb") as f:
        f.write(b"\0" * 100)
    h = ctypes.c_void_p()
    final = os.fsencode(part[:-5])
    assert H.mcd_cachefile_open(os.fsencode(part), final, 5, 6, 0, 120, 124, ctypes.byref(h)) != 0 and not h.value    # 120 bytes > 100
    assert not os.path.exists(part)
    with open(part, "wb") as f:
        f.write(b"\0" * 200)
    assert H.mcd_cachefile_open(os.fsencode(part), final, 5, 6, 0, 60, 124, ctypes.byref(h)) != 0     # a CRC field inside the data
    assert H.mcd_cachefile_open(os.fsencode(part), final, 5, 0, 0, 120, 124, ctypes.byref(h)) != 0    # width 0
    assert H.mcd_cachefile_open(os.fsencode(str(tmp_path / "absent.part")), final, 5, 6, 0, 120, 124, ctypes.byref(h)) != 0
    assert b"absent.part" in H.mcd_cachefile_last_error()


def test_crc32_is_zlibs(H):
    def crc(buf, start=0):
        b = bytes(buf)
        arr = (ctypes.c_ubyte * max(len(b), 1)).from_buffer_copy(b or b"\0")
        return H.mcd_zip_crc32(start, arr, len(b))
    assert crc(b"") == zlib.crc32(b"") == 0
    assert H.mcd_zip_crc32(0, None, 0) == 0
    assert crc(b"123456789") == zlib.crc32(b"123456789") == 0xCBF43926
    nine = bytes([0, 255, 1, 128, 77, 13, 10, 200, 9])
    for cut in range(len(nine) + 1):
        assert crc(nine[cut:], crc(nine[:cut])) == zlib.crc32(nine)
    rng = np.random.default_rng(5)
    for size in (1, 7, 8, 9, 63, 64, 65, 4099, 1 << 16):
        b = rng.integers(0, 256, size=size, dtype=np.uint8).tobytes()
        assert crc(b) == zlib.crc32(b)
        for off in (1, 3, 5):                                 # every alignment of the first 8-byte step
            assert crc(b[off:]) == zlib.crc32(b[off:])
        assert crc(b[size // 3:], crc(b[:size // 3])) == zlib.crc32(b)
    for case in CASES:
        b = source(case[0], case[1]).tobytes()
        assert crc(b) == zlib.crc32(b)


def test_abi_surface(mcd):
    lib = mcd._lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcd_cache.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mcd_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(list(lib.CACHE_SIGNATURES) + list(lib.CACHE_HOST_SIGNATURES))
    assert re.search(r"int mcd_hook_pool_rows\(const float\* x, int64_t B, int64_t Cout, int64_t HW, int mode, float\* dst, int64_t row0,\s*"
                     r"int64_t col0, int64_t stride_n, int64_t stride_u, float\* rows, int64_t width,\s*mcd_stream_t stream\);", text)
    L, H = lib.load(), lib.load_cache_host()
    assert all(hasattr(L, n) for n in lib.CACHE_SIGNATURES) and L.mcd_abi_version() == 9
    assert all(hasattr(H, n) for n in lib.CACHE_HOST_SIGNATURES)
    assert len(lib.CACHE_SIGNATURES["mcd_hook_pool_rows"][1]) == len(lib.SIGNATURES["mcd_hook_pool"][1]) + 2
    tables = [lib.SIGNATURES, lib.TEXT_SIGNATURES, lib.CLIP_SIGNATURES, lib.TOKEN_SIGNATURES, lib.CACHE_SIGNATURES,
              lib.CACHE_HOST_SIGNATURES, lib.BLASLT_SIGNATURES]
    assert len(set().union(*tables)) == sum(len(t) for t in tables)                 # disjoint
    for header in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if header != "mcd_cache.h":
            other = open(os.path.join(ROOT, "include", header)).read()
            assert not re.search(r"mcd_(hook_pool_rows|cache_stream_\w+|cachefile_\w+|zip_crc32)\s*\(", other), header
    # the GPU library does not link the host library: either loads without the other
    out = subprocess.run(["readelf", "-d", lib.LIB_PATH], capture_output=True, text=True)
    if out.returncode == 0:
        assert "libmcd_host" not in out.stdout


def test_the_stream_route_is_not_taken_without_a_gpu(mcd, monkeypatch):
    """extract_and_save chooses the route in Python; MCD_CACHE_STREAM=0 and a non-GPU device keep the writer thread.  (The route
    itself runs in tests/test_gpu_cache_stream.py.)"""
    import inspect
    from mammo_clip_dissect_amd.concept_vit import utils
    src = inspect.getsource(utils.extract_and_save)
    assert 'os.environ.get("MCD_CACHE_STREAM", "1") != "0"' in src and '.type == "cuda"' in src
    for f in os.listdir(CSRC):                                 # the knob is read in Python, never on a data path in C
        if f.endswith((".hip", ".c", ".cpp", ".h", ".inc")):
            assert "MCD_CACHE_STREAM" not in open(os.path.join(CSRC, f)).read(), f


def test_container_under_sanitizers(tmp_path):
    """mcd_host.c and tests/native/cache_host_check.c (its own main: pieces, errors, CRC, on archives with a hand-made layout)
    compiled with -fsanitize=address,undefined and run as a program of their own.  The sanitizer runtimes are linked statically."""
    cc = shutil.which("gcc")
    assert cc, "gcc is what csrc/Makefile builds libmcd_host.so with"
    exe = str(tmp_path / "cache_host_check")
    cmd = [cc, "-O1", "-g", "-std=c11", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "native", "cache_host_check.c"), os.path.join(CSRC, "mcd_host.c"), "-lm"]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "cache_host_check: OK" in r.stdout and "ERROR" not in r.stderr
    assert os.listdir(str(tmp_path)) == ["cache_host_check"]      # the program removed its files; no .part is left
