"""integration/streamparse.h and the woven-cloth BRDF, on bytes: streams written by tests/mts_stream_writer_cloth.py with an
IrawanClothBRDF, plain and under the twosided adapter, in both precisions -> a Lambertian entry whose block is zero, and the weave
with every field of the stream, bit for bit where Float is float; two cloths in one table, beside a Lambertian; a truncated
stream; a zero and an oversized tile; the cloth under a Mask and as a composite's child; and a caller without the table, who is
refused as before."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import cloth_cases as CC
import mts_stream_writer as W
import mts_stream_writer_cloth as WC
import mts_stream_writer_mask as WM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def sp(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    so = str(tmp_path_factory.mktemp("harness_cloth") / "libstreamharness_cloth.so")
    subprocess.check_call(["g++", "-std=gnu++11", "-O1", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-shared",
                           "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "integration"),
                           os.path.join(ROOT, "tests", "stream_harness", "harness_cloth.cpp"), "-o", so])
    return C.CDLL(so)


class Parsed:
    pass


def _parse(sp, data, prec=4, with_cloth=1, cap=16):
    types = np.zeros(cap, dtype=np.uint32); params = np.ones((cap, 16), dtype=np.float32)
    bsdf_weave = np.full(cap, -9, dtype=np.int32)
    weaves = np.full((cap, 24), 0xDEAD, dtype=np.uint32); pattern = np.zeros(4096, dtype=np.uint32); yarns = np.zeros(4096, dtype=np.uint32)
    n, nw, own = C.c_uint32(0), C.c_uint32(0), C.c_int(-2)
    msg = C.create_string_buffer(1024)
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    u32p, i32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_float)
    o = Parsed()
    o.rc = sp.sp_parse_bsdf_table_cloth(buf, C.c_size_t(len(data)), prec, with_cloth, types.ctypes.data_as(u32p), params.ctypes.data_as(f32p),
                                        bsdf_weave.ctypes.data_as(i32p), cap, C.byref(n), weaves.ctypes.data_as(u32p), cap, C.byref(nw),
                                        pattern.ctypes.data_as(u32p), yarns.ctypes.data_as(u32p), 4096, C.byref(own), msg, C.c_size_t(1024))
    o.msg, o.own, o.n, o.nw = msg.value.decode(errors="replace"), own.value, n.value, nw.value
    o.types, o.params, o.bsdf_weave, o.weaves, o.pattern, o.yarns = types[:n.value], params[:n.value], bsdf_weave[:n.value], weaves[:nw.value], pattern, yarns
    return o


def _stream(prec, write):
    s = W.Stream(prec)
    write(s)
    return s.bytes()


def _words(mts, w):
    """the 20 leading words of mtsgpu_weave and the pool words the harness hands out for one scenes.Weave"""
    head = []
    for n in mts.abi.WEAVE_SCALARS:
        v = getattr(w, n)
        head.append(np.uint32(v) if n in ("tileWidth", "tileHeight") else np.float32(v).view(np.uint32))
    head += [np.uint32(len(w.pattern)), np.uint32(len(w.yarns))]
    yarns = []
    for y in w.yarns:
        yarns += [np.uint32(int(y.type))] + [np.float32(getattr(y, n)).view(np.uint32) for n in ("psi", "umax", "kappa", "width", "length", "centerU", "centerV")]
        yarns += list(np.float32(y.kd).view(np.uint32)) + list(np.float32(y.ks).view(np.uint32))
    return np.array(head, dtype=np.uint32), np.array(w.pattern, dtype=np.uint32), np.array(yarns, dtype=np.uint32)


@pytest.mark.parametrize("prec", [4, 8])
def test_irawan_plain_and_twosided(sp, mts, prec):
    for name, w in CC.weaves(mts)[3::5]:          # a 2 x 2 tile of two yarns and a 3 x 2 tile of three, noise on, repeat != 1
        head, pat, yarns = _words(mts, w)
        for two in (0, 0x100):
            inner = WC.irawan("c", w)
            o = _parse(sp, _stream(prec, (lambda s: WM.twosided(s, "t", inner)) if two else inner), prec)
            assert o.rc == 0 and o.own == 0 and o.n == 1 and o.nw == 1, (name, two, o.msg)
            assert o.types[0] == (mts.abi.BSDF_LAMBERTIAN | two) and not o.params[0].any(), "a Lambertian entry whose block is zero"
            assert list(o.bsdf_weave) == [0]
            assert np.array_equal(o.weaves[0, :20], head), (name, "the scalars, the tile and the counts")
            assert list(o.weaves[0, 20:]) == [1, 1, 0, 0], "ClothTable::fill sets both pointers"
            assert np.array_equal(o.pattern[:len(pat)], pat) and np.array_equal(o.yarns[:len(yarns)], yarns)


def test_two_cloths_beside_a_lambertian_and_the_refusals(sp, mts):
    ws = CC.weaves(mts)
    a, b = ws[0][1], ws[8][1]
    o1 = _parse(sp, _stream(4, WC.irawan("c", a)))
    assert o1.rc == 0 and o1.own == 0 and list(o1.bsdf_weave) == [0]
    # truncated anywhere: refused, nothing appended
    data = _stream(4, WC.irawan("c", b))
    for cut in (len(data) - 1, len(data) - 17, len(data) // 2, 40):
        o = _parse(sp, data[:cut])
        assert o.rc == 0 and o.own == -1 and o.n == 0 and o.nw == 0 and "IrawanClothBRDF" in o.msg, (cut, o.msg)
    # a yarn count beyond the stream: refused as truncated, not allocated
    o = _parse(sp, _stream(4, WC.irawan("c", a, yarn_count=1 << 40)))
    assert o.own == -1 and o.n == 0 and o.nw == 0
    for kw, why in ((dict(tileWidth=0), "a dimension is zero or above 32768"), (dict(tileHeight=40000), "a dimension is zero or above 32768")):
        o = _parse(sp, _stream(4, WC.irawan("c", a.replace(**kw), pattern=[])))
        assert o.own == -1 and o.n == 0 and why in o.msg, o.msg
    o = _parse(sp, _stream(4, lambda s: WM.mask(s, "m", (0.5, 0.5, 0.5), WC.irawan("c", a))))
    assert o.own == -1 and o.n == 0 and "a Mask around an IrawanClothBRDF is not supported" in o.msg, o.msg
    P = np.zeros(16, dtype=np.float32); P[:3] = 0.5
    o = _parse(sp, _stream(4, WM.composite("k", [0.5, 0.5], [WM.any_bsdf("a", 0, P), WC.irawan("c", a)])))
    assert o.own == -1 and o.n == 0 and "Composite: child 1 is an IrawanClothBRDF" in o.msg and "as a Lambertian" in o.msg, o.msg
    # a composite beside nothing else still keeps one weave index per entry
    o = _parse(sp, _stream(4, WM.composite("k", [0.5, 0.5], [WM.any_bsdf("a", 0, P), WM.any_bsdf("b", 0, P)])))
    assert o.rc == 0 and o.own == 2 and list(o.bsdf_weave) == [-1, -1, -1] and o.nw == 0, o.msg
    o = _parse(sp, _stream(4, WC.irawan("c", a)), with_cloth=0)
    assert o.own == -1 and o.n == 0 and "IrawanClothBRDF" in o.msg, "without the table the class is not on this path: %s" % o.msg
