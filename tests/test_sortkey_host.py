"""The short-list sort's exact 32-bit key (raster_math.h: sortkey_pack / _pos / _rel / _fits / _is_padding), compiled for the
host by g++ exactly as tests/host_check compiles the rest of that header. select_sort_kernel sorts a tile on this word alone, so
wherever sortkey_fits() holds the order of the keys must BE the order of (depth bits, list position), every real key must lie
below the padding, and the fields must come back out unchanged. No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "host_check", "sortkey_check.cpp")
_HDR = os.path.join(_HERE, "..", "skyfall-gs_amd", "csrc", "raster_math.h")
_BUILD = os.path.join(_HERE, "host_check", "_build")
_FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"]


def _build(name, extra):
    out = os.path.join(_BUILD, name)
    newest = max(os.path.getmtime(_SRC), os.path.getmtime(_HDR))
    if not os.path.exists(out) or os.path.getmtime(out) < newest:
        os.makedirs(_BUILD, exist_ok=True)
        subprocess.check_call(["g++", *_FLAGS, *extra, "-o", out, _SRC])
    return out


@pytest.fixture(scope="module")
def sk():
    lib = C.CDLL(_build("libsortkey.so", ["-O2", "-fPIC", "-shared"]))
    u32, i32, p = C.c_uint32, C.c_int, C.c_void_p
    lib.sk_pad.restype = lib.sk_max_range.restype = u32
    lib.sk_max_range.argtypes = [i32]
    lib.sk_fits.argtypes = [u32, u32, i32]
    lib.sk_pack.argtypes = [p, i32, u32, i32, p]
    lib.sk_unpack.argtypes = [p, i32, i32, p, p, p]
    lib.sk_same_depth.argtypes = [u32, u32, i32]
    return lib


def _bits(z):
    return np.ascontiguousarray(z, dtype=np.float32).view(np.uint32)


def _pack(sk, d, pb):
    d = np.ascontiguousarray(d, dtype=np.uint32)
    k = np.zeros(len(d), np.uint32)
    sk.sk_pack(d.ctypes.data, len(d), int(d.min()), pb, k.ctypes.data)
    return k


def _unpack(sk, k, pb):
    pos, rel, pad = np.zeros(len(k), np.uint32), np.zeros(len(k), np.uint32), np.zeros(len(k), np.int32)
    sk.sk_unpack(k.ctypes.data, len(k), pb, pos.ctypes.data, rel.ctypes.data, pad.ctypes.data)
    return pos, rel, pad


def _assert_orders_as_depth_pos(sk, d, pb):
    d = np.ascontiguousarray(d, dtype=np.uint32)
    assert sk.sk_fits(int(d.min()), int(d.max()), pb)
    k = _pack(sk, d, pb)
    pos, rel, pad = _unpack(sk, k, pb)
    np.testing.assert_array_equal(pos, np.arange(len(d), dtype=np.uint32))
    np.testing.assert_array_equal(rel, d - d.min())
    assert not pad.any() and int(k.max()) < sk.sk_pad()
    # sorting the keys == sorting (depth bits, pos) lexicographically
    np.testing.assert_array_equal(np.argsort(k, kind="stable"), np.lexsort((np.arange(len(d)), d)))
    assert len(np.unique(k)) == len(k)
    return k


@pytest.mark.parametrize("pb", [9, 10])
def test_key_order_is_depth_then_position(sk, pb):
    rng = np.random.default_rng(5 + pb)
    cap = 1 << pb
    for z0, span in ((0.2, 0.05), (7.0, 2.0), (250.0, 100.0), (3000.0, 0.01), (12.5, 0.0)):
        for n in (1, 2, 63, 257, cap):
            z = (z0 + span * rng.random(n)).astype(np.float32)
            if n > 4:
                z[n // 2] = z[1]    # an exact tie: ordered by position, reported by sk_same_depth
            k = _assert_orders_as_depth_pos(sk, _bits(z), pb)
            if n > 4:
                assert sk.sk_same_depth(int(k[1]), int(k[n // 2]), pb)
    # adjacent bit patterns, both ways round in the list
    b = int(_bits([1.5])[0])
    k = _assert_orders_as_depth_pos(sk, [b + 1, b, b + 2, b + 1, b], pb)
    assert not sk.sk_same_depth(int(k[0]), int(k[1]), pb) and sk.sk_same_depth(int(k[0]), int(k[3]), pb)


@pytest.mark.parametrize("pb", [9, 10])
def test_range_limit_and_padding(sk, pb):
    R, cap, pad = sk.sk_max_range(pb), 1 << pb, sk.sk_pad()
    assert R == (1 << (32 - pb)) - 2 and pad == 0xffffffff
    for lo in (int(_bits([0.2])[0]), int(_bits([1.0])[0]), int(_bits([300.0])[0])):
        assert sk.sk_fits(lo, lo, pb) and sk.sk_fits(lo, lo + R - 1, pb) and sk.sk_fits(lo, lo + R, pb)
        assert not sk.sk_fits(lo, lo + R + 1, pb) and not sk.sk_fits(lo, lo + 4 * R, pb)
        # a list AT the limit, its far end in the last position: the largest key there is
        d = np.full(cap, lo + R // 2, np.uint32)
        d[0], d[-1], d[1], d[-2] = lo + R - 1, lo + R, lo, lo + 1
        k = _assert_orders_as_depth_pos(sk, d, pb)
        assert int(k[-1]) == int(k.max()) == pad - cap        # strictly below the padding, by a whole rel step
        both = np.concatenate([k, np.full(3, pad, np.uint32)])
        pos, rel, is_pad = _unpack(sk, both, pb)
        assert is_pad.tolist() == [0] * cap + [1] * 3 and int(rel[:cap].max()) == R < int(rel[-1])
        assert not sk.sk_same_depth(int(k[-1]), pad, pb)
    # the far-camera scenes: a tile's depths within one binade fit; a near-to-far tile does not
    assert sk.sk_fits(int(_bits([250.0])[0]), int(_bits([350.0])[0]), 9)
    assert not sk.sk_fits(int(_bits([1.0])[0]), int(_bits([300.0])[0]), pb)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_standalone_program(flags):
    """the same source with its own main(): pairwise order on edge-case and random lists; once under the host sanitizers"""
    exe = _build("sortkey_check_" + ("san" if len(flags) > 1 else "plain"), ["-DSORTKEY_MAIN", *flags])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "sortkey OK" in r.stdout, r.stdout + r.stderr
