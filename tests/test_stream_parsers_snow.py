"""integration/streamparse.h and the snow BRDFs, on bytes: streams written by tests/mts_stream_writer_snow.py with a Wiscombe,
plain and under the twosided adapter, in both precisions -> a Lambertian entry with the record mtsgpu_wiscombe_configure makes of
the four fields, bit for bit; a truncated stream; a Wiscombe whose derived values are not finite, under a Mask and as a
composite's child; HanrahanKrueger, refused with what its stream lacks; and a caller without the list, who is refused as before."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mts_stream_writer as W
import mts_stream_writer_mask as WM
import mts_stream_writer_snow as WS
import mts_stream_writer_ward as WW
import ref64_snow as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sp(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    so = str(tmp_path_factory.mktemp("harness_snow") / "libstreamharness_snow.so")
    subprocess.check_call(["g++", "-std=gnu++11", "-O1", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-shared",
                           "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "integration"),
                           os.path.join(ROOT, "tests", "stream_harness", "harness_snow.cpp"), "-o", so])
    return C.CDLL(so)


class Parsed:
    pass


def _parse(sp, mts, data, prec=4, with_snow=1, cap=16, configure=True):
    types = np.zeros(cap, dtype=np.uint32); params = np.zeros((cap, 16), dtype=np.float32)
    snow = np.full((cap, 16), 0xDEAD, dtype=np.uint32); mask_kind = np.full(cap, -9, dtype=np.int32)
    n, own = C.c_uint32(0), C.c_int(-2)
    msg = C.create_string_buffer(1024)
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    u32p, i32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_float)
    f = C.cast(mts.lib().mtsgpu_wiscombe_configure, C.c_void_p) if configure else C.c_void_p(0)
    o = Parsed()
    o.rc = sp.sp_parse_bsdf_table_snow(buf, C.c_size_t(len(data)), prec, with_snow, f, types.ctypes.data_as(u32p), params.ctypes.data_as(f32p),
                                       snow.ctypes.data_as(u32p), mask_kind.ctypes.data_as(i32p), cap, C.byref(n), C.byref(own), msg, C.c_size_t(1024))
    o.msg, o.own, o.n = msg.value.decode(errors="replace"), own.value, n.value
    o.types, o.params, o.snow, o.mask_kind = types[:n.value], params[:n.value], snow[:n.value], mask_kind[:n.value]
    return o


def _stream(prec, write):
    s = W.Stream(prec)
    write(s)
    return s.bytes()


def _record(mts, raw):
    e = mts.snow_configure(mts.abi.SNOW_WISCOMBE, raw)
    return np.concatenate([np.uint32([e.kind, e.reserved]), np.float32(list(e.derived)).view(np.uint32)])


@pytest.mark.parametrize("prec", [4, 8])
def test_wiscombe_plain_and_twosided(sp, mts, prec):
    cases = [dict(), dict(g=0.5, depth=0.1), dict(w0=(0.99, 0.95, 0.9), sigma_t=(1.0, 2.0, 3.0))]
    for kw in cases:
        raw = R.wiscombe_raw(**kw)
        want = _record(mts, raw)
        assert want[0] == mts.abi.SNOW_WISCOMBE and np.array_equal(want[2:].view(np.float32), R.configure32(R.WISCOMBE, raw)[0])
        for two in (0, 0x100):
            inner = WS.wiscombe("w", **kw)
            data = _stream(prec, (lambda s: WM.twosided(s, "t", inner)) if two else inner)
            o = _parse(sp, mts, data, prec)
            assert o.rc == 0 and o.own == 0 and o.n == 1, (kw, two, o.msg)
            assert o.types[0] == mts.abi.BSDF_LAMBERTIAN | two and not o.params[0].any(), "a Lambertian entry whose block is zero"
            assert np.array_equal(o.snow[0], want), (kw, two)
            assert o.mask_kind.tolist() == [0]


def test_entries_without_a_snow_brdf_get_none(sp, mts):
    sd = mts.scenes.SceneDescription("b")
    lam, ward = sd.lambertian(0.5, 0.6, 0.4), sd.ward(0.15, 0.3)
    s = W.Stream(); WW.any_bsdf(s, "b", sd.bsdf_type[lam], sd.bsdf_params[lam])
    o = _parse(sp, mts, s.bytes())
    assert o.rc == 0 and o.n == 1 and not o.snow.any()
    s = W.Stream(); WW.composite(s, "c", [0.5, 0.5], [("a", 0, sd.bsdf_params[lam]), ("b", 8, sd.bsdf_params[ward])])
    o = _parse(sp, mts, s.bytes())
    assert o.rc == 0 and o.own == 2 and o.n == 3 and not o.snow.any()
    half = (0.5, 0.5, 0.5)
    s = W.Stream(); WM.mask(s, "m", half, WM.any_bsdf("n", 0, sd.bsdf_params[lam]))
    o = _parse(sp, mts, s.bytes())
    assert o.rc == 0 and o.mask_kind.tolist() == [1] and not o.snow.any(), "the mask list and the snow list live side by side"


def test_refusals(sp, mts):
    sd = mts.scenes.SceneDescription("b")
    lam = sd.lambertian(0.5)
    P = sd.bsdf_params[lam]

    def refused(data, *words, **kw):
        o = _parse(sp, mts, data, **kw)
        assert o.rc == 1 and o.own == -1 and o.n == 0, o.msg
        for w in words:
            assert w in o.msg, (w, o.msg)
        return o.msg
    good = _stream(4, WS.wiscombe("w"))
    for cut in (1, 5, 13, 25):
        refused(good[:-cut], "while reading a Wiscombe")
    refused(_stream(4, WS.wiscombe("w", g=0.0)), "Wiscombe: configure() leaves a derived value that is not finite (g = 0")
    refused(_stream(8, WS.wiscombe("w", w0=(0.99, float("nan"), 0.99))), "Wiscombe: configure() leaves a derived value that is not finite")
    refused(_stream(4, WM.composite("c", [0.5, 0.5], [WM.any_bsdf("a", 0, P), WS.wiscombe("w")])), "Composite: child 1 is a Wiscombe", "as a Lambertian")
    refused(_stream(4, WM.composite("c", [0.5, 0.5], [lambda s: WM.twosided(s, "t", WS.wiscombe("w")), WM.any_bsdf("a", 0, P)])),
            "Composite: child 0 is a Wiscombe")
    refused(_stream(4, lambda s: WM.mask(s, "m", (0.5, 0.5, 0.5), WS.wiscombe("w"))), "a Mask around a Wiscombe is not supported")
    refused(good, "a snow list without mtsgpu_wiscombe_configure", configure=False)
    # HanrahanKrueger: the message names what the stream lacks
    for data in (_stream(4, WS.hanrahan_krueger("h")), _stream(8, lambda s: WM.twosided(s, "t", WS.hanrahan_krueger("h", 2.0)))):
        msg = refused(data, "HanrahanKrueger: its stream holds only sizeMultiplier, sigmaA and sigmaS", "hanrahan-krueger.cpp:225-230")
        for lacking in ("g", "etaInt", "etaExt", "ssFactor", "drFactor", "diffuseReflectance", "mtsgpu_hk_configure"):
            assert lacking in msg, lacking
    refused(_stream(4, WM.composite("c", [1.0], [WS.hanrahan_krueger("h")])), "Composite: child 0 is a HanrahanKrueger")
    # without the list both are what they were: classes that are not on this path
    for data, cls in ((good, "Wiscombe"), (_stream(4, lambda s: WM.twosided(s, "t", WS.wiscombe("w"))), "Wiscombe"),
                      (_stream(4, WS.hanrahan_krueger("h")), "HanrahanKrueger")):
        msg = refused(data, "BSDF class %s is not on this path" % cls, with_snow=0)
        assert "while reading a %s" % cls in msg
